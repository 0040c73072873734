"""The single-product arithmetic ("fp16 x 1": csrc/kernels_gemm3.h, engine option "gemm_f16x1") restated in numpy: the rounding rule of
its contract, and a stage-by-stage model of tdf3_kernel<..., S> (running row exponents, one weight exponent per four output columns, one
fp16 rounding per scaled operand, fp32 accumulation).  A helper of tests/test_f16x1_math.py and tests/test_gpu_*_f16x1.py, not a test file."""
import numpy as np

RISE, RISE_CAP = 10, 40          # kernels_gemm3.h F16X3_RISE / F16X3_RISE_CAP

# The margin of tests/test_gpu_rowgemm_f16x1.py::test_block_exponent: device error against the UNROUNDED float64 GEMM <= MARGIN x the same measure of
# the contract reference (round11 operands, float64).  tests/test_f16x1_math.py::test_policy_on_block_exponent_inputs shows that the policy (which elements the running
# exponent leaves in the subnormal floor) moves the measure by less than 1e-9 of itself on these five inputs, and fp32 accumulation by 2e-4 of
# itself in the model; what remains is the accumulation error of the device's own summation order, which the fp16 x 3 test of the same inputs
# bounds by 4e-6 of a group's own scale (tests/test_gpu_parity.py::test_rowgemm_f16x3_block_exponent) against a contract measure of 4.7e-4
# at the least: 1 + 4e-6 / 4.7e-4 = 1.0085, rounded up.
BLOCK_MARGIN = 1.02


def round11(v):
    """v rounded to 11 significant bits, round-to-nearest-even, whatever its exponent (float64 in, float64 out): what an element that stays in
    fp16's normal range under its block exponent enters the products as."""
    m, ex = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(np.rint(m * 2048) / 2048, ex)


def scale_exp(m):
    """f16_scale_exp: e with m 2^e in [2^14, 2^15) (m > 0 finite); 15 for m == 0"""
    m = np.asarray(m, np.float32)
    _, ex = np.frexp(m)
    return np.where(m > 0, 15 - ex, 15).astype(np.int64)


def split1(x, e):
    """RNE_f16(v 2^e) as float64 (the ldexp is exact in fp32 inside fp16's range; fp16 values are exact in float64)"""
    xs = np.ldexp(np.asarray(x, np.float32), e).astype(np.float32)
    with np.errstate(over="ignore"):
        return xs.astype(np.float16).astype(np.float64)


def weight_exponents(w):
    """one exponent per group of four output columns: the group's largest |w| lands in [2^14, 2^15) (w3h_split_kernel)"""
    w = np.asarray(w, np.float32)
    ew = np.zeros(w.shape[0], np.int64)
    for t in range(0, w.shape[0], 4):
        m = np.abs(w[t:t + 4]).max()
        ew[t:t + 4] = scale_exp(m)[()] if m > 0 else 0
    return ew


def emulate_rows(x, w, stage=32, acc32=True):
    """y = x @ w.T the way tdf3_kernel<..., S> does it: the running per-row exponent of the fp16 x 3 form (drops to need - 2 when a stage would pass
    2^15, rises to need - 2 when a stage's largest element is more than RISE bits below the range, at most RISE_CAP bits above the row's lowest
    exponent so far; the accumulators follow by the exact power of two), every scaled operand rounded ONCE to fp16, one product per pair,
    fp32 accumulation (one rounding per 32-deep stage, as the MFMA commits at least; acc32 = False: float64 accumulation -- the policy alone)."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    M, K = x.shape
    N = w.shape[0]
    ew = weight_exponents(w)
    wh = split1(w, ew[:, None])
    acc = np.zeros((M, N), np.float32 if acc32 else np.float64)
    e_row = np.full(M, 200, np.int64)
    e_lo = np.full(M, 200, np.int64)
    for k0 in range(0, K, stage):
        xs = x[:, k0:k0 + stage]
        top = np.abs(xs).max(axis=1)
        need = scale_exp(top)
        e_new = np.where(need < e_row, need - 2, e_row)
        up = (need > e_row + RISE) & (top > 0)
        e_new = np.where(up, np.minimum(need - 2, e_lo + RISE_CAP), e_new)
        e_lo = np.minimum(e_lo, e_new)
        de = e_new - e_row
        with np.errstate(under="ignore"):
            acc = (acc * np.ldexp(np.float32(1.0), de)[:, None].astype(acc.dtype)).astype(acc.dtype)
        e_row = e_new
        xh = split1(xs, e_row[:, None])
        assert np.isfinite(xh).all(), "a scaled element overflowed fp16"
        acc = (acc.astype(np.float64) + xh @ wh[:, k0:k0 + stage].T).astype(acc.dtype)
    return np.ldexp(acc.astype(np.float64), -(e_row[:, None] + ew[None, :]))


def block_exponent_case(shape):
    """The five inputs of tests/test_gpu_parity.py::test_rowgemm_f16x3_block_exponent, same seed and construction: x [1, 2, 192, 1024], w [272, 1024]."""
    B, c, T, K, N = 1, 2, 192, 1024, 272
    rng = np.random.default_rng(91)
    x = rng.standard_normal((B, c, T, K))
    k = np.arange(K)
    if shape.startswith("decay"):
        x *= np.exp2((-60.0 if shape == "decay60" else -20.0) * k / K)[None, None, None, :] * np.exp2(3.0 * (np.arange(T) % 7) - 9)[None, None, :, None]
    elif shape == "growing":
        x *= np.exp2(24.0 * k / K)[None, None, None, :]
    else:
        x[..., : K // 2] = 0.0
        x[:, :, 100:, :] = 0.0
    x = x.astype(np.float32)
    w = rng.standard_normal((N, K)) / np.sqrt(K)
    w[:16, : K // 2] = 0.0
    w[16:32] *= 1e-6
    if shape == "chan4":
        w *= np.repeat(np.exp2(rng.integers(-20, 21, N // 4)), 4)[:, None]
    return x, w.astype(np.float32)


BLOCK_SHAPES = ("decay", "decay60", "growing", "zeros", "chan4")


def group_measure(y, lin, shape):
    """worst error of a row x column group over the group's own scale, as test_rowgemm_f16x3_block_exponent measures it (column groups 0-15, 16-31,
    32-N; "chan4": every column at its own scale too).  y and lin [rows, N]; the error is taken against relu(lin).  Returns (worst, all-zero rows
    came out exactly zero)."""
    ref = np.maximum(lin, 0)
    N = lin.shape[1]
    worst, zeros_ok = 0.0, True
    for cols in (slice(0, 16), slice(16, 32), slice(32, N)):
        scale = np.sqrt((lin[:, cols] ** 2).mean(axis=1))
        err = np.sqrt(((y[:, cols] - ref[:, cols]) ** 2).mean(axis=1))
        ok = scale > 0
        if ok.any():
            worst = max(worst, float((err[ok] / scale[ok]).max()))
        zeros_ok = zeros_ok and bool((err[~ok] == 0).all())
    if shape == "chan4":
        cs = np.sqrt((lin ** 2).mean(axis=0))
        ce = np.sqrt(((y - ref) ** 2).mean(axis=0))
        worst = max(worst, float((ce / cs).max()))
    return worst, zeros_ok
