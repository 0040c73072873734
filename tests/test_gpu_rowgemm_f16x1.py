"""The single-product row GEMM (tdf3_kernel<..., S>, engine option "gemm_f16x1": csrc/kernels_gemm3.h "fp16 x 1") against its arithmetic
contract, one launch at a time through Engine.op_tdf: float64 products of the operands rounded ONCE to 11 significant bits
(tests/f16x1_ref.py round11), held to the per-element bar of the fp32-accumulating kernels.  The single rounding is in the reference, so
nothing looser is needed -- a kernel that rounds twice, rounds the wrong operand or reads a stale l image misses the bar by 100x."""
import numpy as np
import pytest

from tests import f16x1_ref as F

BLOCK_MARGIN = F.BLOCK_MARGIN

pytestmark = pytest.mark.gpu

# the shapes of ROWGEMM_CASES in tests/test_gpu_parity.py: odd stage counts (K = 96, 160), N off the tile grid (72, 136, 200), 7-row tiles,
# residual on / off, x scales from 1e-3 to 1e4, all three tile forms and the 8-wave form (N = 384)
CASES = [
    # B, c, T, K, N, res, x scale
    (2, 48, 64, 3072, 384, False, 3.0), (2, 48, 64, 384, 3072, True, 1.0), (1, 96, 37, 1536, 192, False, 1e4),
    (1, 3, 41, 512, 2048, True, 1e-3), (1, 1, 1000, 64, 72, True, 1.0), (3, 5, 7, 128, 200, False, 30.0),
    (2, 144, 16, 96, 768, True, 1.0), (1, 2, 33, 160, 136, False, 5.0),
]


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


def engine(A):
    return A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=16, overlap=0.25))


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


def counters(eng):
    return tuple(eng.counter(k) for k in ("tdf3_launches", "tdf3h_launches", "tdf3s_launches"))


def rose(eng, before):
    return tuple(a - b for a, b in zip(counters(eng), before))


@pytest.mark.parametrize("B,c,T,K,N,res,xs", CASES)
def test_rowgemm_f16x1_vs_contract(A, B, c, T, K, N, res, xs):
    """ref = epilogue(float64(round11(x)) @ float64(round11(w)).T); |y - ref| <= 8e-7 mag + 1e-30 per element and rel-RMS < 2e-6.  `mag` is the size
    of the terms that enter an output, as at the bar's origin (tests/test_gpu_parity.py:203, whose `mag` carries its epilogue's bias): the products
    sc (|x| @ |w|.T) and the epilogue's addends |sh| and |res| -- an fp32 epilogue rounds the sum it forms, so a residual 50x a quiet row's products
    costs half a unit of ITS last place whatever the GEMM did (the bare product term cannot be met by an exact GEMM there).  The worst ratio against
    the bare products is printed for the cases without a residual."""
    eng = engine(A)
    fresh = engine(A)
    rng = np.random.default_rng(K * 11 + N)
    x = (xs * rng.standard_normal((B, c, T, K)) * np.exp2(rng.integers(-6, 7, (B, c, T, 1)))).astype(np.float32)
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    sc = (0.5 + rng.random(c)).astype(np.float32)
    sh = (0.2 * xs * rng.standard_normal(c)).astype(np.float32)
    r = (xs * rng.standard_normal((B, c, T, N))).astype(np.float32) if res else None
    xr, wr = F.round11(x), F.round11(w)
    sc4, sh4 = sc[None, :, None, None].astype(np.float64), sh[None, :, None, None].astype(np.float64)
    ref = np.maximum(sc4 * (xr @ wr.T) + sh4, 0)
    prod = sc4 * (np.abs(xr) @ np.abs(wr).T)
    mag = prod + np.abs(sh4)
    if res:
        ref = ref + r
        mag = mag + np.abs(r)
    assert eng.option("gemm_f16x1") == 0, "the option is off unless asked for"
    c0 = counters(eng)
    y_off = eng.op_tdf(x, w, None, sc, sh, r)
    assert rose(eng, c0) == (1, 1, 0), "option off: the fp16 x 3 kernel runs, the single-product counter does not move"
    assert np.array_equal(y_off, fresh.op_tdf(x, w, None, sc, sh, r)), "option off: not the bits of an untouched engine"
    eng.set_option("gemm_f16x1", 1)
    c0 = counters(eng)
    y = eng.op_tdf(x, w, None, sc, sh, r)
    assert rose(eng, c0) == (1, 1, 1), "the single-product kernel did not run (tdf3s_launches + 1, tdf3h_launches + 1)"
    assert np.array_equal(y, eng.op_tdf(x, w, None, sc, sh, r)), "not deterministic"
    eng.set_option("gemm_f16x1", 0)
    c0 = counters(eng)
    assert np.array_equal(eng.op_tdf(x, w, None, sc, sh, r), y_off), "option back to 0: not the fp16 x 3 bits"
    assert rose(eng, c0) == (1, 1, 0)
    assert np.isfinite(y).all(), "unwritten (NaN canary) output elements"
    d = np.abs(y - ref)
    e, e_un = rel_rms(y, ref), rel_rms(y, np.maximum(sc4 * (x.astype(np.float64) @ w.astype(np.float64).T) + sh4, 0) + (r if res else 0))
    print(f"fp16 x 1 row GEMM K={K} N={N}: worst |y - ref| / mag {float((d / mag).max()):.2e}" +
          ("" if res else f" (/ products alone {float((d / (prod + 1e-300)).max()):.2e})") +
          f", rel-RMS vs contract {e:.2e}, vs the unrounded GEMM {e_un:.2e}, fp16 x 3 vs contract {rel_rms(y_off, ref):.2e}")
    assert (d <= 8e-7 * mag + 1e-30).all(), float((d / mag).max())
    assert e < 2e-6, e
    assert e_un > 20 * e, "the contract reference is no closer than the unrounded GEMM: the launch was not single-product"


@pytest.mark.parametrize("shape", F.BLOCK_SHAPES)
def test_block_exponent(A, shape):
    """The five inputs of test_rowgemm_f16x3_block_exponent: elements leave fp16's normal range under the running exponent there, so the measure is
    per row x column group against the group's own scale, taken against the UNROUNDED float64 GEMM, and held to BLOCK_MARGIN x the same measure of
    the contract reference (tests/f16x1_ref.py derives the margin, tests/test_f16x1_math.py checks the policy model against it)."""
    eng = engine(A)
    x, w = F.block_exponent_case(shape)
    c = x.shape[1]
    sc, sh = np.ones(c, np.float32), np.zeros(c, np.float32)
    x2 = x.reshape(-1, x.shape[-1])
    lin = x2.astype(np.float64) @ w.astype(np.float64).T
    contract, _ = F.group_measure(np.maximum(F.round11(x2) @ F.round11(w).T, 0), lin, shape)
    eng.set_option("gemm_f16x1", 1)
    c0 = counters(eng)
    y = eng.op_tdf(x, w, None, sc, sh, None)
    assert rose(eng, c0) == (1, 1, 1)
    assert np.isfinite(y).all()
    dev, zeros_ok = F.group_measure(y.reshape(-1, w.shape[0]).astype(np.float64), lin, shape)
    print(f"fp16 x 1 row GEMM, {shape}: worst row x column-group error over its own scale {dev:.4e}, contract reference {contract:.4e} (x {dev / contract:.4f})")
    assert zeros_ok, "an all-zero row did not come out exactly zero"
    assert dev <= BLOCK_MARGIN * contract, (dev, contract)


def test_nonfinite_rows_stay_local(A):
    """as test_rowgemm_bf16x6_nonfinite_rows: the exponents are per row, so no other row changes by a bit; a poisoned row's accumulators are NaN
    (Inf 2^e is Inf in fp16, Inf x 0-weights and Inf - Inf sums are NaN) or +-Inf, and the ReLU's maxNum returns 0 for NaN"""
    eng = engine(A)
    B, c, T, K, N = 1, 2, 40, 128, 136
    rng = np.random.default_rng(78)
    clean = rng.standard_normal((B, c, T, K)).astype(np.float32)
    x = clean.copy()
    x[0, 0, 3, 17] = np.inf
    x[0, 0, 9, 0] = -np.inf
    x[0, 1, 5, 127] = np.nan
    x[0, 1, 30, 64] = np.inf
    x[0, 1, 30, 65] = -np.inf
    w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    sc, sh = np.ones(c, np.float32), np.zeros(c, np.float32)
    eng.set_option("gemm_f16x1", 1)
    c0 = counters(eng)
    y, yc = eng.op_tdf(x, w, None, sc, sh, None), eng.op_tdf(clean, w, None, sc, sh, None)
    assert rose(eng, c0) == (2, 2, 2)
    bad = np.zeros((B, c, T), bool)
    for idx in ((0, 0, 3), (0, 0, 9), (0, 1, 5), (0, 1, 30)):
        bad[idx] = True
    assert np.array_equal(y[~bad], yc[~bad]), "a non-finite input leaked into another row"
    assert np.isfinite(y[~bad]).all()
    assert not np.isnan(y[bad]).any() and ((y[bad] == 0) | np.isinf(y[bad])).all(), "a poisoned row is 0 (NaN through maxNum) or +Inf"
    assert (y[0, 1, 5] == 0).all(), "a NaN element: NaN accumulators, 0 behind the ReLU"


def test_weight_cache_follows_reloads(A):
    """The h-only image is cached beside the two-part one per weight tensor: a second layer uploaded to (possibly) the same address must see
    neither the first's image nor the other arithmetic's, with the option alternating between the reloads."""
    eng = engine(A)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, 2, 64, 128)).astype(np.float32)
    sc, sh = np.ones(2, np.float32), np.zeros(2, np.float32)
    xr = F.round11(x)
    for seed in range(6):
        on = seed % 2 == 0
        w = (np.random.default_rng(seed).standard_normal((128, 128)) / 11.0).astype(np.float32)
        eng.set_option("gemm_f16x1", 1 if on else 0)
        c0 = counters(eng)
        y = eng.op_tdf(x, w, None, sc, sh, None)
        assert rose(eng, c0) == (1, 1, 1 if on else 0)
        ref = np.maximum((xr @ F.round11(w).T) if on else (x.astype(np.float64) @ w.astype(np.float64).T), 0)
        assert rel_rms(y, ref) < 1e-6, (seed, on, rel_rms(y, ref))
