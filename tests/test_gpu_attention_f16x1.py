"""The single-product Roformer attention (attention6_kernel<QW, true, true>: variants "attn6s" / "attn6s_qw2", engine option "gemm_f16x1") against
its arithmetic contract, one launch at a time through Engine.op_attention.

Reference: float64 softmax attention (tests/attention_ref.py) on round11(Q), round11(K), round11(V) -- the kernel rounds each of them once to
fp16 under a power-of-two block exponent, which for elements in fp16's normal range is a rounding to 11 significant bits (tests/f16x1_ref.py), so
the operand roundings are IN the reference.  Measure: worst (query, head) row, max |kernel - ref| / max |ref| of the row, as in
tests/test_gpu_attention.py.

Bar: BAR32[class] + 2^-11.  What the reference does not carry is the rounding of the probabilities P handed to the PV product: P is scaled by 2^14
behind the running maximum of its key tile and rounded once to fp16, a relative error of at most 2^-11 per probability (half a unit of an 11-bit
significand is 2^-12 at the top of a binade and 2^-11 at its bottom; p >= 2^-28 stays normal, smaller ones err by 2^-39 absolutely).  The row sums
are formed from the unrounded P in fp32.  So an output differs from the reference's by at most sum_j |dp_j| |v_j| / sum_j p_j <= 2^-11 max |V| --
2^-11 on the row-normalised measure -- beyond what the fp32 parts (logits, max, exp, sums, rescale between key tiles: the code of the fp16 x 3 form,
held to BAR32 by tests/test_gpu_attention.py) contribute.  Derived, not tuned.  The sharp check below feeds inputs for which P rounds exactly and
holds the kernel to the plain BAR32 bar: a kernel that rounds an operand twice or to fewer bits fails it by 10x and more."""
import numpy as np
import pytest

from tests import attention_ref as R
from tests import f16x1_ref as F

pytestmark = pytest.mark.gpu

VARIANTS = ("attn6s", "attn6s_qw2")
# the class bars of tests/test_gpu_attention.py (worst-row error of the fp32-grade kernels, per class of input)
BAR32 = {"plain": 1.5e-5, "peaked": 2e-5, "decay6": 2.5e-5, "q_mag": 2e-4}
P_TERM = 2.0 ** -11
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 257)      # key-tile tails and the QW2 switch at 128
EDGES = ("normal", "peaked", "max_last", "max_first", "equal", "zero_q", "gates", "k_tiles", "v_spike")


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


def make_case(edge, S, L, Lk, heads, d, seed):
    """Q [S, L, heads, d], K / V [S, Lk, heads, d], gate [S, L, heads] (float32 values) with one of the EDGES applied per sequence
    (tests/test_gpu_attention.py make_case, the edges used here)."""
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
    elif edge == "k_tiles":                    # K tiles 2^16 apart, logits kept O(1)
        K *= np.exp2(16.0 * (tiles % 2))[None, :, None, None]
        Q *= 2.0 ** -16
    elif edge == "v_spike":                    # one element 2^12 above the rest of its tile
        V[:, Lk // 2, :, 3] = 4096 * np.abs(V).max()
    f = np.float32
    return Q.astype(f), K.astype(f), V.astype(f), G.astype(f)


def pack_rof(Q, K, V, G, B, T, Fb, axis, pad_rows=0, gate_pad=0):
    """per-sequence arrays -> qkv [M, 3 * heads * 64], gate [M, heads + gate_pad] of the token matrix [B, T, Fb] (+ pad_rows)"""
    heads = Q.shape[2]

    def tok(X):
        c = X.shape[3]
        if axis == "time":
            return X.reshape(B, Fb, T, heads * c).transpose(0, 2, 1, 3).reshape(B * T * Fb, heads * c)
        return X.reshape(B * T * Fb, heads * c)
    n = B * T * Fb
    qkv = np.full((n + pad_rows, 3 * heads * 64), np.float32(7.0))
    qkv[:n] = np.concatenate([tok(Q), tok(K), tok(V)], 1)
    gate = np.full((n + pad_rows, heads + gate_pad), np.float32(3.0))
    gate[:n, :heads] = tok(G[..., None])
    return qkv, gate


def run(eng, qkv, gate, B, T, Fb, axis, exact=False, label=""):
    """both variants on one input against the contract reference: {variant: worst-row error}; checks the padding rows and the counters"""
    n = B * T * Fb
    heads = qkv.shape[1] // 192
    ref = R.rof_attention(F.round11(qkv), gate, B, T, Fb, axis)
    errs = {}
    for v in VARIANTS:
        c0 = [eng.counter(k) for k in ("attn6_launches", "attn6h_launches", "attn6s_launches")]
        out, ran = eng.op_attention(qkv, gate, B, T, Fb, axis=axis, exact=exact, variant=v)
        assert ran == v
        assert [eng.counter(k) - b for k, b in zip(("attn6_launches", "attn6h_launches", "attn6s_launches"), c0)] == [1, 1, 1]
        assert np.isnan(out[n:]).all(), f"{v} wrote padding rows"
        assert np.isfinite(out[:n]).all(), f"{v} left rows unwritten"
        errs[v] = R.worst_row_error(out[:n], ref, heads)
    print(f"{label}: " + " ".join(f"{v} {e:.2e}" for v, e in errs.items()))
    return errs


@pytest.mark.parametrize("axis", ["time", "freq"])
@pytest.mark.parametrize("L", LENGTHS)
def test_lengths(eng, L, axis):
    B, H, other = 1, 2, 3
    T, Fb = (L, other) if axis == "time" else (other, L)
    Q, K, V, G = make_case("normal", B * other, L, L, H, 64, seed=L)
    qkv, gate = pack_rof(Q, K, V, G, B, T, Fb, axis, pad_rows=3)
    for v, e in run(eng, qkv, gate, B, T, Fb, axis, label=f"fp16 x 1 attention {axis} L={L}").items():
        assert e < BAR32["plain"] + P_TERM, (v, e)


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("edge", EDGES)
def test_edges(eng, edge, exact):
    B, T, Fb, H = 1, 257, 2, 2
    Q, K, V, G = make_case(edge, B * Fb, T, T, H, 64, seed=EDGES.index(edge))
    qkv, gate = pack_rof(Q, K, V, G, B, T, Fb, "time", pad_rows=2)
    bar = BAR32.get(edge, BAR32["plain"]) + P_TERM
    for v, e in run(eng, qkv, gate, B, T, Fb, "time", exact=exact, label=f"fp16 x 1 attention {edge} exact={exact}").items():
        assert e < bar, (v, edge, e)


@pytest.mark.parametrize("edge", ["max_last", "max_first"])
def test_sharp_when_nothing_rounds(eng, edge):
    """Inputs that are ALREADY round11 and so peaked that P is one-hot (the winning logit more than 60 above the rest: every other probability is below 1e-26
    of it): no operand and no probability is changed by its rounding, so the kernel must meet float64 within the plain BAR32 bar -- the P term of
    the bar above has nothing to cover here."""
    B, T, Fb, H = 1, 257, 2, 2
    Q, K, V, G = make_case(edge, B * Fb, T, T, H, 64, seed=40)
    K[:, -1 if edge == "max_last" else 0] *= 4          # 24 u: the winner's logit is about 24 |u|^2 / 8 = 192
    Q, K, V = (F.round11(a).astype(np.float32) for a in (Q, K, V))
    qkv, gate = pack_rof(Q, K, V, G, B, T, Fb, "time")
    assert np.array_equal(F.round11(qkv), qkv.astype(np.float64))
    s = np.einsum("sihd,sjhd->shij", Q.astype(np.float64), K.astype(np.float64)) / 8
    top2 = np.sort(s, axis=-1)[..., -2:]
    assert (top2[..., 1] - top2[..., 0]).min() > 60, "not one-hot"
    for v, e in run(eng, qkv, gate, B, T, Fb, "time", label=f"fp16 x 1 attention, one-hot {edge}").items():
        assert e < BAR32["plain"], (v, e)


@pytest.mark.parametrize("variant", VARIANTS)
def test_deterministic_and_batch_invariant(eng, variant):
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


def test_auto_resolves_to_single_product_only_with_the_option(eng):
    """"auto" is attn6s_qw2 (more than 128 keys) / attn6s when and only when "gemm_f16x1" is on AND the fp16 x 3 form would run"""
    Q, K, V, G = make_case("normal", 2, 129, 129, 1, 64, seed=1)
    qkv, gate = pack_rof(Q, K, V, G, 1, 129, 2, "time")
    qkvs, gates = pack_rof(Q[:, :64], K[:, :64], V[:, :64], G[:, :64], 1, 64, 2, "time")
    expect = {(1, 1, 0): ("attn6h_qw2", "attn6h"), (1, 1, 1): ("attn6s_qw2", "attn6s"), (1, 0, 1): ("attn6_qw2", "attn6"), (0, 1, 1): ("attn2", "attn2")}
    assert eng.option("gemm_f16x1") == 0
    try:
        for (b6, h3, s1), (long_, short) in expect.items():
            eng.set_option("gemm_bf16x6", b6)
            eng.set_option("gemm_f16x3", h3)
            eng.set_option("gemm_f16x1", s1)
            c0 = eng.counter("attn6s_launches")
            assert eng.op_attention(qkv, gate, 1, 129, 2)[1] == long_
            assert eng.op_attention(qkvs, gates, 1, 64, 2)[1] == short
            assert eng.counter("attn6s_launches") - c0 == (2 if (b6, h3, s1) == (1, 1, 1) else 0)
    finally:
        eng.set_option("gemm_bf16x6", 1)
        eng.set_option("gemm_f16x3", 1)
        eng.set_option("gemm_f16x1", 0)
