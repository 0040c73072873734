"""The arithmetic contract of the single-product form ("fp16 x 1": csrc/kernels_gemm3.h, include/asx.h option "gemm_f16x1") on the CPU: the
rounding rule the GPU tests build their float64 references from, its subnormal floor, the per-element bound of a k-stage sum with fp32
accumulation, and the running-exponent policy on the block-exponent inputs of the GPU test (tests/f16x1_ref.py is the numpy model)."""
import numpy as np

from tests import f16x1_ref as F

BLOCK_MARGIN = F.BLOCK_MARGIN


def test_round11_is_fp16_rounding_of_the_scaled_value():
    rng = np.random.default_rng(0)
    n = 400000
    # the scaled value anywhere in fp16's NORMAL range [2^-14, 65504], the block exponent anywhere a float32 operand can need
    v16 = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-14, 15, n)) * rng.choice([-1.0, 1.0], n))
    e = rng.integers(-100, 101, n)
    v = np.ldexp(v16, -e).astype(np.float32)                   # the fp32 operand
    scaled = np.ldexp(v, e).astype(np.float32)                 # exact: a power of two
    assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), v.astype(np.float64))
    ok = (np.abs(scaled) >= 2.0 ** -14) & (np.abs(scaled) < 65504)
    assert ok.mean() > 0.99
    h = scaled.astype(np.float16).astype(np.float64)
    assert np.array_equal(np.ldexp(h, -e)[ok], F.round11(v.astype(np.float64))[ok])
    # ties go to even, as RNE_f16 does
    assert F.round11(1 + 2.0 ** -11) == 1.0 and F.round11(1 + 3 * 2.0 ** -11) == 1 + 2.0 ** -9
    assert F.round11(0.0) == 0.0
    # relative error of the rule: half a unit of the 11th bit, 2^-11 of the value at the most
    assert (np.abs(F.round11(v.astype(np.float64)) - v) <= np.abs(v) * 2.0 ** -11).all()


def test_subnormal_floor():
    """a row whose largest element sits anywhere in [2^12, 2^15) after scaling (two bits of headroom): elements down to 2^-26 of it stay
    normal and follow round11; below, the error is absolute, at most 2^-25 in scaled units -- under 2^-37 of the row maximum"""
    rng = np.random.default_rng(1)
    for top in (2.0 ** 12, 2.0 ** 13.5, 2.0 ** 14.99):
        rel = np.exp2(-rng.uniform(0, 40, 200000))
        xs = (rng.choice([-1.0, 1.0], rel.size) * top * rel).astype(np.float32)
        h = F.split1(xs, 0)
        assert np.isfinite(h).all()
        normal = np.abs(xs) >= top * 2.0 ** -26
        assert (np.abs(xs[normal]) >= 2.0 ** -14).all()
        assert np.array_equal(h[normal], F.round11(xs[normal].astype(np.float64)))
        err = np.abs(h - xs.astype(np.float64))
        floor = np.abs(xs) < 2.0 ** -14                          # fp16 subnormals (spacing 2^-24): all of them are below 2^-26 of the maximum
        assert floor.any() and not (floor & normal).any()
        assert (err[floor] <= 2.0 ** -25).all() and err[floor].max() <= top * 2.0 ** -37
        assert np.array_equal(h[~floor], F.round11(xs[~floor].astype(np.float64)))
    # W: the group maximum is in [2^14, 2^15): normal down to 2^-28 of it
    assert 2.0 ** 14 * 2.0 ** -28 == 2.0 ** -14
    # nothing overflows below 2^15 (fp16's largest finite value is 65504)
    assert np.isfinite(F.split1(np.float32(2.0 ** 15 * (1 - 2.0 ** -13)), 0))


def test_stage_sums_stay_inside_the_per_element_bound():
    """|y - round11(x) @ round11(w).T| <= 8e-7 (|x| @ |w|.T): the bar of tests/test_gpu_rowgemm_f16x1.py, on the model with one fp32 rounding per
    32-deep stage -- at K = 3072 (96 roundings of a running sum) and with rows 2^12 apart."""
    rng = np.random.default_rng(2)
    for M, K, N, xs in ((24, 3072, 40, 3.0), (16, 96, 24, 1e4), (16, 160, 24, 1e-3), (1, 32, 8, 1.0)):
        x = (xs * rng.standard_normal((M, K)) * np.exp2(rng.integers(-6, 7, (M, 1)))).astype(np.float32)
        w = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
        y = F.emulate_rows(x, w)
        xr, wr = F.round11(x), F.round11(w)
        ref = xr @ wr.T
        mag = np.abs(xr) @ np.abs(wr).T
        assert (np.abs(y - ref) <= 8e-7 * mag + 1e-30).all(), float((np.abs(y - ref) / mag).max())
        # ... and the single rounding is what separates it from the unrounded GEMM: a few 1e-4 of a row (2^-11 / sqrt(3) per operand)
        un = x.astype(np.float64) @ w.astype(np.float64).T
        rel = np.sqrt(((ref - un) ** 2).mean() / (un ** 2).mean())
        assert 5e-5 < rel < 5e-4, rel


def test_policy_on_block_exponent_inputs():
    """The five block-exponent inputs of the GPU test: the running exponent leaves some elements in the subnormal floor, so the model is
    measured against the UNROUNDED float64 GEMM per row x column group, beside the contract reference (round11 operands, float64)."""
    for shape in F.BLOCK_SHAPES:
        x, w = F.block_exponent_case(shape)
        x2 = x.reshape(-1, x.shape[-1])
        lin = x2.astype(np.float64) @ w.astype(np.float64).T
        contract, _ = F.group_measure(np.maximum(F.round11(x2) @ F.round11(w).T, 0), lin, shape)
        policy, zeros_ok = F.group_measure(np.maximum(F.emulate_rows(x2, w, acc32=False), 0), lin, shape)
        model, zeros_ok32 = F.group_measure(np.maximum(F.emulate_rows(x2, w), 0), lin, shape)
        print(f"{shape}: contract {contract:.4e}, policy alone {policy:.4e} (x {policy / contract:.6f}), with fp32 accumulation {model:.4e} (x {model / contract:.6f})")
        assert zeros_ok and zeros_ok32, "an all-zero row did not come out zero"
        assert 1e-4 < contract < 4e-3, contract                 # an 11-bit rounding of either operand: 2^-12 .. 2^-9 of a group
        assert abs(policy / contract - 1) < 1e-6, (shape, policy, contract)
        assert model <= (1 + (BLOCK_MARGIN - 1) / 4) * contract, (shape, model, contract)
