"""Every attention kernel against float64 softmax attention, one launch at a time through asx_op_attention / asx_op_mha (the
engines' own launch code, csrc/engine_attn.h): Roformer attention2_kernel / attention6_kernel, HTDemucs mha_kernel / mha6_kernel
(self and cross attention), LocalState mha_kernel<DT, true> / hd_local_attn_kernel -- at key-tile tails, long sequences, softmax
edges and the block-exponent edges of the bf16 x 6 / fp16 x 3 forms.

Error measure: per (query, head) row, max |kernel - float64| / max |float64| of that row, worst row taken (tests/attention_ref.py).
The fp32-MFMA variants are held to an absolute bar per class of input; the bf16 x 6 / fp16 x 3 variants to "no worse than K16 x the
fp32 variant on the same input" (with a floor) and the same bar.  test_bars_catch_mutants shows the bars are tight enough to catch a kernel that drops
the last key or the online-max correction between key tiles.
"""
import numpy as np
import pytest

from tests import attention_ref as R

pytestmark = pytest.mark.gpu

ROF_FP32 = ("attn2", "attn2_qw2", "attn2_db")
ROF_16 = ("attn6", "attn6_qw2", "attn6h", "attn6h_qw2")
MHA_FP32 = ("mha", "mha_db")
MHA_16 = ("mha6", "mha6_wide", "mha6h", "mha6h_wide")

# Bars (worst-row error, see the module docstring), about 3-4x the worst measured on an MI355X.  The error of every kernel, fp32 ones
# included, follows the conditioning of the input (fp32 logits of magnitude |s| carry errors ~|s| * 2^-24), so the fp32 bar is set per class:
BAR32 = {
    "plain": 1.5e-5,   # measured 4.0e-6 (mha dh 64, 1344 queries x 2688 keys); 2.2e-6 at T = 801; ~1e-7 below one key tile
    "peaked": 2e-5,    # logits spanning +-60: measured 5.5e-6 (attn2*), 4.9e-6 (mha*)
    "decay6": 2.5e-5,  # LocalState decay logits x 6 (slopes up to 2.5 per step): measured 6.4e-6 (hd_local dh 4, T 1895)
    "q_mag": 2e-4,     # per-query magnitudes 2^-30 .. 2^20 (logits up to ~2^23): measured 5.2e-5 (mha), 4.0e-5 (attn2)
}
# bf16 x 6 / fp16 x 3 kernels: <= max(K16 x the fp32 variant on the same input, FLOOR16) and <= the class bar.  Measured: at most
# 1.62x the fp32 variant (attn6h max_last) where that one is above 1e-7; 1.5e-7 where the fp32 kernel is exact (one key, one-hot rows)
K16, FLOOR16 = 5.0, 5e-7

LENGTHS = (1, 2, 17, 63, 64, 65, 127, 128, 129, 191, 193, 257)
EDGES = ("normal", "peaked", "max_last", "max_first", "equal", "zero_q", "gates", "q_mag", "k_tiles", "v_rise", "v_fall",
         "v_zero_first", "v_spike")


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


def make_case(edge, S, L, Lk, heads, d, seed):
    """Q [S, L, heads, d], K / V [S, Lk, heads, d], gate [S, L, heads] (float32 values) with one of the EDGES applied per sequence."""
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((S, L, heads, d))
    K = rng.standard_normal((S, Lk, heads, d))
    V = rng.standard_normal((S, Lk, heads, d))
    G = 2 * rng.standard_normal((S, L, heads))
    tiles = np.arange(Lk) // R.KEY_TILE
    if edge == "peaked":                       # logits spanning about +-60: near one-hot rows
        Q *= 20 * np.sqrt(8.0 / d)
    elif edge in ("max_last", "max_first"):    # every query's maximum in the last (first) key, far above the rest
        u = rng.standard_normal((S, 1, heads, d))
        Q = u + 0.1 * Q
        K *= 0.1
        K[:, -1 if edge == "max_last" else 0] = 6 * u[:, 0] * np.sqrt(64.0 / d)
    elif edge == "equal":                      # all logits of a row equal: the plain mean of V
        K[:] = K[:, :1]
    elif edge == "zero_q":
        Q[:, ::3] = 0
    elif edge == "gates":                      # saturated sigmoid
        G = np.where(rng.random(G.shape) < 0.5, -30.0, 30.0)
    elif edge == "q_mag":                      # per-query magnitudes 2^-30 .. 2^20
        Q *= np.exp2(rng.integers(-30, 21, (S, L, heads, 1)))
    elif edge == "k_tiles":                    # K tiles 2^16 apart, logits kept O(1)
        K *= np.exp2(16.0 * (tiles % 2))[None, :, None, None]
        Q *= 2.0 ** -16
    elif edge == "v_rise":                     # each V tile 2^8 above the one before
        V *= np.exp2(8.0 * tiles)[None, :, None, None]
    elif edge == "v_fall":
        V *= np.exp2(-8.0 * tiles)[None, :, None, None]
    elif edge == "v_zero_first":
        V[:, :R.KEY_TILE] = 0
    elif edge == "v_spike":                    # one element 2^12 above the rest of its tile
        V[:, Lk // 2, :, 3] = 4096 * np.abs(V).max()
    f = np.float32
    return Q.astype(f), K.astype(f), V.astype(f), G.astype(f)


def pack_rof(Q, K, V, G, B, T, Fb, axis, pad_rows=0, gate_pad=0):
    """per-sequence arrays -> qkv [M, 3 * heads * 64], gate [M, heads + gate_pad] of the token matrix [B, T, Fb] (+ pad_rows)"""
    heads = Q.shape[2]

    def tok(X):   # [S, L, heads, c] -> [B * T * Fb, heads * c]
        c = X.shape[3]
        if axis == "time":    # S = B * Fb, L = T
            return X.reshape(B, Fb, T, heads * c).transpose(0, 2, 1, 3).reshape(B * T * Fb, heads * c)
        return X.reshape(B * T * Fb, heads * c)   # S = B * T, L = Fb
    n = B * T * Fb
    qkv = np.full((n + pad_rows, 3 * heads * 64), np.float32(7.0))
    qkv[:n] = np.concatenate([tok(Q), tok(K), tok(V)], 1)
    gate = np.full((n + pad_rows, heads + gate_pad), np.float32(3.0))
    gate[:n, :heads] = tok(G[..., None])
    return qkv, gate


def check_16(name, e16, e32, bar):
    assert e16 < bar and e16 <= max(K16 * e32, FLOOR16), f"{name}: {e16:.3e} against fp32 variant {e32:.3e}"


def run_rof(eng, qkv, gate, B, T, Fb, axis, variants, exact=False, label=""):
    """every variant on one input; returns {variant: worst-row error}; checks the padding rows stay NaN and the attn6 counters"""
    n = B * T * Fb
    heads = qkv.shape[1] // 192
    ref = R.rof_attention(qkv, gate, B, T, Fb, axis)
    errs = {}
    for v in variants:
        n6, n6h = eng.counter("attn6_launches"), eng.counter("attn6h_launches")
        out, ran = eng.op_attention(qkv, gate, B, T, Fb, axis=axis, exact=exact, variant=v)
        assert ran == v
        assert eng.counter("attn6_launches") - n6 == ("6" in v)
        assert eng.counter("attn6h_launches") - n6h == ("6h" in v)
        assert np.isnan(out[n:]).all(), f"{v} wrote padding rows"
        errs[v] = R.worst_row_error(out[:n], ref, heads)
    print(f"{label}: " + " ".join(f"{v} {e:.2e}" for v, e in errs.items()))
    return errs


def check_rof(errs, bar=BAR32["plain"]):
    for v, e in errs.items():
        if v in ROF_FP32:
            assert e < bar, (v, e)
        else:
            check_16(v, e, errs["attn2"], bar)


@pytest.mark.parametrize("L", LENGTHS + (801,))
def test_rof_lengths_time_axis(eng, L):
    """every Roformer variant along time at key-tile tails (Fb = 5; 801 frames: the ep_317 chunk)"""
    B, Fb, H = 1, 5 if L < 801 else 2, 2
    Q, K, V, G = make_case("normal", B * Fb, L, L, H, 64, seed=L)
    qkv, gate = pack_rof(Q, K, V, G, B, L, Fb, "time", pad_rows=3)
    check_rof(run_rof(eng, qkv, gate, B, L, Fb, "time", ROF_FP32 + ROF_16, label=f"rof time T={L}"))


@pytest.mark.parametrize("B,T,Fb,axis,H,gate_pad", [
    (1, 3, 62, "freq", 2, 0),     # the 62 bands of ep_317
    (2, 4, 65, "freq", 2, 0),
    (1, 2, 129, "freq", 1, 3),
    (1, 65, 62, "time", 1, 0),    # Fb = 62 along time
    (3, 70, 5, "time", 4, 0),     # B > 1, gate_ld == heads (the engine's stride when heads % 4 == 0)
    (2, 130, 3, "time", 3, 5),    # gate_ld > heads
])
def test_rof_geometry(eng, B, T, Fb, axis, H, gate_pad):
    L = T if axis == "time" else Fb
    S = B * (Fb if axis == "time" else T)
    Q, K, V, G = make_case("normal", S, L, L, H, 64, seed=B * 1000 + T + Fb)
    qkv, gate = pack_rof(Q, K, V, G, B, T, Fb, axis, pad_rows=5, gate_pad=gate_pad)
    check_rof(run_rof(eng, qkv, gate, B, T, Fb, axis, ROF_FP32 + ROF_16, label=f"rof {axis} B={B} T={T} Fb={Fb} H={H}"))


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("edge", EDGES)
def test_rof_edges(eng, edge, exact):
    B, T, Fb, H = 1, 257, 2, 2
    Q, K, V, G = make_case(edge, B * Fb, T, T, H, 64, seed=EDGES.index(edge))
    qkv, gate = pack_rof(Q, K, V, G, B, T, Fb, "time")
    check_rof(run_rof(eng, qkv, gate, B, T, Fb, "time", ROF_FP32 + ROF_16, exact=exact, label=f"rof {edge} exact={exact}"),
              BAR32.get(edge, BAR32["plain"]))


# ---- MhaArgs: HTDemucs self / cross attention -------------------------------------------------------------------------------
def pack_mha(Q, K, V, qpad=4, kpad=8):
    """[S, L, heads, d] -> rows S * L with padded leading dimensions (the engine's q / k / v are column slices of one matrix)"""
    S, L, H, d = Q.shape
    Lk = K.shape[1]
    q = np.full((S * L, H * d + qpad), np.float32(5.0))
    q[:, :H * d] = Q.reshape(S * L, H * d)
    k = np.full((S * Lk, H * d + kpad), np.float32(5.0))
    k[:, :H * d] = K.reshape(S * Lk, H * d)
    v = np.full((S * Lk, H * d + kpad + 4), np.float32(5.0))
    v[:, :H * d] = V.reshape(S * Lk, H * d)
    return q, k, v


def run_mha(eng, q, k, v, B, nq, nk, H, dh, variants, decay=None, exact=False, ldo_pad=8, label=""):
    ref = R.mha(q, k, v, B, nq, nk, H, dh, decay=decay)
    errs = {}
    for var in variants:
        out0 = np.full((B * nq, H * dh + ldo_pad), np.nan, np.float32)
        n6, n6h = eng.counter("attn6_launches"), eng.counter("attn6h_launches")
        out, ran = eng.op_mha(q, k, v, B, nq, nk, H, dh, decay=decay, exact=exact, variant=var, out=out0)
        assert ran == var
        assert eng.counter("attn6_launches") - n6 == ("6" in var)
        assert eng.counter("attn6h_launches") - n6h == ("6h" in var)
        assert np.isnan(out[:, H * dh:]).all(), f"{var} wrote the padding columns of ldo"
        errs[var] = R.worst_row_error(out[:, :H * dh], ref, H)
    print(f"{label}: " + " ".join(f"{v} {e:.2e}" for v, e in errs.items()))
    return errs


def check_mha(errs, bar=BAR32["plain"]):
    for v, e in errs.items():
        if v in MHA_FP32 or v == "hd_local":
            assert e < bar, (v, e)
        else:
            check_16(v, e, errs["mha"], bar)


def mha_variants(dh):
    return ("mha", "mha_db") + MHA_16 if dh == 48 else ("mha",) + MHA_16


# (nq, nk): tile tails, cross attention both ways, and the HTDemucs default segment (7.8 s at 44.1 kHz: 336 frames x 8 bins
# = 2688 frequency tokens, 1344 time tokens; engine_ht.h ht_run_transformer)
MHA_SHAPES = [(n, n) for n in LENGTHS] + [(100, 337), (337, 100), (1344, 2688), (2688, 1344)]


@pytest.mark.parametrize("dh", [48, 64])
@pytest.mark.parametrize("nq,nk", MHA_SHAPES)
def test_mha_lengths(eng, nq, nk, dh):
    big = nq * nk > 10 ** 6
    B, H = (1, 1) if big else (2, 2)
    Q, K, V, _ = make_case("normal", B, nq, nk, H, dh, seed=nq * 7 + nk + dh)
    q, k, v = pack_mha(Q, K, V)
    check_mha(run_mha(eng, q, k, v, B, nq, nk, H, dh, mha_variants(dh), label=f"mha dh={dh} nq={nq} nk={nk}"))


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("edge", [e for e in EDGES if e != "gates"])
def test_mha_edges(eng, edge, exact):
    B, H, dh, nq, nk = 2, 2, 48, 129, 257
    Q, K, V, _ = make_case(edge, B, nq, nk, H, dh, seed=100 + EDGES.index(edge))
    q, k, v = pack_mha(Q, K, V)
    check_mha(run_mha(eng, q, k, v, B, nq, nk, H, dh, mha_variants(dh), exact=exact, label=f"mha {edge} exact={exact}"),
              BAR32.get(edge, BAR32["plain"]))


# ---- LocalState (decay form): mha_kernel<DT, true> for dh 16 .. 96, hd_local_attn_kernel for the narrow heads ------------------
@pytest.mark.parametrize("dscale", [0.3, 6.0])
@pytest.mark.parametrize("T", [1, 2, 63, 65, 129, 257, 1895])   # 1895: a LocalState sequence of the apply_model chunks (kernels_hd.h)
@pytest.mark.parametrize("dh", [4, 8, 12, 24, 16, 32, 48, 64, 96])
def test_local_state(eng, dh, T, dscale):
    B = 1 if T > 1000 else 2
    H = 4
    rng = np.random.default_rng(dh * 10000 + T)
    Q, K, V, _ = make_case("normal", B, T, T, H, dh, seed=dh + T)
    q, k, v = pack_mha(Q, K, V, qpad=0, kpad=0) if dh < 16 else pack_mha(Q, K, V)
    decay = (dscale * rng.standard_normal((B * T, 4 * H + 4))).astype(np.float32)
    variants = ("hd_local",) if dh < 16 or dh == 24 else (("mha", "mha_db") if dh == 48 else ("mha",))
    errs = run_mha(eng, q, k, v, B, T, T, H, dh, variants, decay=decay, ldo_pad=0 if variants == ("hd_local",) else 4,
                   label=f"local_state dh={dh} T={T} decay x{dscale}")
    check_mha(errs, BAR32["decay6" if dscale > 1 else "plain"])


# ---- the bars can catch a wrong kernel ----------------------------------------------------------------------------------------
def test_bars_catch_mutants():
    """the two mutants (tests/attention_ref.py) on representative inputs of this file miss float64 by >= 10x every bar"""
    bar = max(BAR32.values())
    Q, K, V, G = make_case("max_last", 2, 129, 129, 2, 64, seed=3)
    qkv, gate = pack_rof(Q, K, V, G, 1, 129, 2, "time")
    ref = R.rof_attention(qkv, gate, 1, 129, 2, "time")
    for m in ("drop_last", "tile_local"):
        e = R.worst_row_error(R.rof_attention(qkv, gate, 1, 129, 2, "time", mutant=m), ref, 2)
        print(f"mutant {m}, Roformer T=129: {e:.2e}")
        assert e >= 10 * bar, (m, e)
    for edge, nq, nk in (("normal", 337, 100), ("max_last", 129, 257)):
        Q, K, V, _ = make_case(edge, 2, nq, nk, 2, 48, seed=5)
        q, k, v = pack_mha(Q, K, V)
        ref = R.mha(q, k, v, 2, nq, nk, 2, 48)
        for m in ("drop_last", "tile_local"):
            e = R.worst_row_error(R.mha(q, k, v, 2, nq, nk, 2, 48, mutant=m), ref, 2)
            print(f"mutant {m}, mha {edge} {nq}/{nk}: {e:.2e}")
            assert e >= 10 * bar, (m, edge, e)
    Q, K, V, _ = make_case("normal", 2, 129, 129, 4, 8, seed=6)
    q, k, v = pack_mha(Q, K, V, qpad=0, kpad=0)
    decay = np.random.default_rng(6).standard_normal((2 * 129, 16)).astype(np.float32)
    ref = R.mha(q, k, v, 2, 129, 129, 4, 8, decay=decay)
    e = R.worst_row_error(R.mha(q, k, v, 2, 129, 129, 4, 8, decay=decay, mutant="drop_last"), ref, 4)
    print(f"mutant drop_last, LocalState T=129: {e:.2e}")
    assert e >= 10 * bar


# ---- determinism, batch invariance, launch rule -----------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ROF_FP32 + ROF_16)
def test_rof_deterministic_and_batch_invariant(eng, variant):
    T, Fb, H = 193, 3, 2
    Q, K, V, G = make_case("normal", 4 * Fb, T, T, H, 64, seed=11)
    qkv4, gate4 = pack_rof(Q, K, V, G, 4, T, Fb, "time")
    qkv1, gate1 = pack_rof(Q[2 * Fb:3 * Fb], K[2 * Fb:3 * Fb], V[2 * Fb:3 * Fb], G[2 * Fb:3 * Fb], 1, T, Fb, "time")
    a, _ = eng.op_attention(qkv4, gate4, 4, T, Fb, variant=variant)
    b, _ = eng.op_attention(qkv4, gate4, 4, T, Fb, variant=variant)
    c, _ = eng.op_attention(qkv1, gate1, 1, T, Fb, variant=variant)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    n = T * Fb
    assert np.array_equal(a[2 * n:3 * n].view(np.uint32), c.view(np.uint32))


@pytest.mark.parametrize("variant,dh,decay", [(v, 48, False) for v in MHA_FP32 + MHA_16] + [("mha", 64, True), ("hd_local", 12, True)])
def test_mha_deterministic_and_batch_invariant(eng, variant, dh, decay):
    nq = nk = 200
    H = 4
    Q, K, V, _ = make_case("normal", 4, nq, nk, H, dh, seed=12)
    dec = np.random.default_rng(12).standard_normal((4 * nq, 16)).astype(np.float32) if decay else None
    pad = (0, 0) if variant == "hd_local" else (4, 8)
    q4, k4, v4 = pack_mha(Q, K, V, *pad)
    q1, k1, v1 = pack_mha(Q[2:3], K[2:3], V[2:3], *pad)
    d1 = dec[2 * nq:3 * nq] if decay else None
    a, _ = eng.op_mha(q4, k4, v4, 4, nq, nk, H, dh, decay=dec, variant=variant)
    b, _ = eng.op_mha(q4, k4, v4, 4, nq, nk, H, dh, decay=dec, variant=variant)
    c, _ = eng.op_mha(q1, k1, v1, 1, nq, nk, H, dh, decay=d1, variant=variant)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a[2 * nq:3 * nq].view(np.uint32), c.view(np.uint32))


def test_auto_follows_engine_rule(eng):
    """"auto" resolves to what the engines launch (engine_rof.h rof_attn_variant, engine_ht.h ht_mha_variant, engine_hd.h
    hd_attn_variant) under the default environment, for each setting of the arithmetic options"""
    Q, K, V, G = make_case("normal", 2, 129, 129, 1, 64, seed=1)
    qkv, gate = pack_rof(Q, K, V, G, 1, 129, 2, "time")
    qkvs, gates = pack_rof(Q[:, :64], K[:, :64], V[:, :64], G[:, :64], 1, 64, 2, "time")
    Qm, Km, Vm, _ = make_case("normal", 1, 129, 64, 1, 64, seed=2)
    q, k, v = pack_mha(Qm, Km, Vm)
    q48, k48, v48 = pack_mha(Qm[..., :48], Km[..., :48], Vm[..., :48])
    expect = {(1, 1): ("attn6h_qw2", "attn6h", "mha6h_wide"), (1, 0): ("attn6_qw2", "attn6", "mha6_wide"), (0, 1): ("attn2", "attn2", "mha")}
    try:
        for (b6, h3), (long_, short, m) in expect.items():
            eng.set_option("gemm_bf16x6", b6)
            eng.set_option("gemm_f16x3", h3)
            assert eng.op_attention(qkv, gate, 1, 129, 2)[1] == long_
            assert eng.op_attention(qkvs, gates, 1, 64, 2)[1] == short
            assert eng.op_mha(q, k, v, 1, 129, 64, 1, 64)[1] == m
            assert eng.op_mha(q48, k48, v48, 1, 129, 64, 1, 48)[1] == m
            assert eng.op_mha(q[:64], k, v, 1, 64, 64, 1, 64)[1] == m.replace("_wide", "")
    finally:
        eng.set_option("gemm_bf16x6", 1)
        eng.set_option("gemm_f16x3", 1)
    dec = np.zeros((129, 16), np.float32)
    Qd, Kd, Vd, _ = make_case("normal", 1, 129, 129, 4, 48, seed=3)
    assert eng.op_mha(*pack_mha(Qd, Kd, Vd), 1, 129, 129, 4, 48, decay=dec)[1] == "mha_db"   # ASX_MHA_DB defaults to on for LocalState
    Qd, Kd, Vd, _ = make_case("normal", 1, 129, 129, 4, 8, seed=3)
    assert eng.op_mha(*pack_mha(Qd, Kd, Vd, 0, 0), 1, 129, 129, 4, 8, decay=dec)[1] == "hd_local"


def test_variants_refused(eng):
    import audio_separator_amd as A
    Q, K, V, _ = make_case("normal", 1, 70, 70, 2, 64, seed=4)
    q, k, v = pack_mha(Q, K, V)
    qo, _, _ = pack_mha(Q, K, V, qpad=2)                     # ldq % 4 != 0
    Q32, K32, V32, _ = make_case("normal", 1, 70, 70, 2, 32, seed=4)
    dec = np.zeros((70, 8), np.float32)
    bad = [
        lambda: eng.op_mha(qo, k, v, 1, 70, 70, 2, 64, variant="mha6"),
        lambda: eng.op_mha(qo, k, v, 1, 70, 70, 2, 64, variant="auto"),
        lambda: eng.op_mha(*pack_mha(Q32, K32, V32), 1, 70, 70, 2, 32, variant="mha"),     # dh 32 without decay: not built
        lambda: eng.op_mha(*pack_mha(Q32, K32, V32), 1, 70, 70, 2, 32, variant="auto"),
        lambda: eng.op_mha(q, k, v, 1, 70, 70, 2, 64, variant="mha_db"),                  # DB is built for dh 48 only
        lambda: eng.op_mha(q, k, v, 1, 70, 70, 2, 64, decay=dec, variant="mha6"),          # no decay form of mha6
        lambda: eng.op_mha(q, k, v, 1, 70, 70, 2, 64, decay=dec, variant="hd_local"),      # dh 64 is not a narrow head
        lambda: eng.op_mha(q, k, v, 1, 70, 70, 2, 64, variant="attn2"),
        lambda: eng.op_mha(q, k, v, 1, 70, 70, 2, 64, variant="nonesuch"),
    ]
    G = np.zeros((2 * 70, 2), np.float32)
    qkv, gate = pack_rof(Q, K, V, np.zeros((1, 70, 2), np.float32), 1, 70, 1, "time")
    bad += [lambda: eng.op_attention(qkv, gate, 1, 70, 1, variant="mha6"),
            lambda: eng.op_attention(qkv, gate, 1, 71, 1, variant="attn2"),             # more tokens than rows
            lambda: eng.op_attention(qkv, G[:70, :1], 1, 70, 1, variant="attn2")]       # gate_ld < heads
    for i, f in enumerate(bad):
        with pytest.raises(A.AsxError):
            f()
            pytest.fail(f"case {i} was launched")
