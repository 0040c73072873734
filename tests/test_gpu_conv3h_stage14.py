"""conv3h_kernel's 14-stage consumer (csrc/kernels_conv3h.h, Conv3hCfg::PLAN) on the device, through `op_conv("conv3x3", ...)`: the half stages
of two kernel rows of one exponent block share one MFMA stage (lanes g < 2 one row, lanes g >= 2 the other), the third row keeps its padded half
stage, wave 1 runs a stage program of its own.  One-hot weights on exactly the k groups those stages carry (a half that takes the wrong row's
weights or pixels moves a whole plane), exponent steps on block boundaries (waves 0 and 1 rescale between different stages), the accumulate
form at 96 / 144 channels, and batch invariance.  Every case proves which kernel ran."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    assert e.option("winograd") == 3 and e.option("conv_direct_f16x3") == 144 and e.option("gemm_f16x3") == 1
    yield e
    e.close()


def conv3h(eng, x, w, b, relu=False):
    c = x.shape[1]
    n0 = eng.counter("conv3h_launches")
    y = eng.op_conv("conv3x3", x, w, b, relu=relu)
    assert eng.counter("conv3h_launches") - n0 == (c // 48) ** 2, "conv3h_kernel did not run"
    return y


def ref64(x, w, b, relu=False):
    """float64 convolution and sum |w| |x| (+ |b|): what an fp32 chain's roundings are relative to"""
    X, W, Bv = torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double()
    r = torch.nn.functional.conv2d(X, W, Bv, padding=1)
    mag = torch.nn.functional.conv2d(X.abs(), W.abs(), Bv.abs(), padding=1).numpy()
    return (torch.relu(r) if relu else r).numpy(), mag


def test_one_hot_weights_on_the_half_stage_k_groups(eng):
    """k groups 16 and 17 of a kernel row are (kx = 2, channels 32..39 / 40..47): the merged and the padded stages.  One output channel per
    (ky, kx, ci) with a single weight 1.0, all in one launch; every other output channel has no weight at all.  The values are +-[0.5, 2): within two
    bits of the block's largest, so the two fp16 parts hold 22 bits of each and the unit weight (2^14 after scaling, exact) adds no rounding:
    2^-21 of each value is the format's bound, not a fitted one."""
    T, F = 12, 64
    rng = np.random.default_rng(14)
    x = (rng.uniform(0.5, 2.0, size=(1, 48, T, F)) * rng.choice([-1.0, 1.0], size=(1, 48, T, F))).astype(np.float32)
    taps = [(ky, kx, ci) for ky in range(3) for kx, ci in ((2, 32), (2, 40), (2, 47), (0, 0), (1, 20))]
    cos = [(7 * i + 3) % 48 for i in range(len(taps))]          # spread over the three channel tiles and both store halves
    assert len(set(cos)) == len(taps) == 15
    w = np.zeros((48, 48, 3, 3), np.float32)
    for co, (ky, kx, ci) in zip(cos, taps):
        w[co, ci, ky, kx] = 1.0
    y = conv3h(eng, x, w, np.zeros(48, np.float32))
    xp = np.pad(x[0], ((0, 0), (1, 1), (1, 1)))
    for co, (ky, kx, ci) in zip(cos, taps):
        want = xp[ci, ky:ky + T, kx:kx + F]
        err = np.abs(y[0, co].astype(np.float64) - want)
        for r in range(4):                              # every wave's rows
            worst = float((err[r::4] / np.maximum(np.abs(want[r::4]), 1e-30)).max())
            print(f"one-hot ky {ky} kx {kx} ci {ci} -> co {co}, rows t % 4 == {r}: max relative error {worst:.3e}")
            assert (err[r::4] <= 2.0 ** -21 * np.abs(want[r::4])).all(), (ky, kx, ci, r, worst)
    rest = [co for co in range(48) if co not in cos]
    assert (y[0, rest] == 0).all(), "an output channel without weights is not zero"


def stepped_input(rng, B, c, T, F, sign):
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    x[:, :, 5:] *= np.float32(2.0 ** (12 * sign))       # rows 5.. and 13.. open four-row blocks (block j = rows 4 j + 1 .. 4 j + 4): tiles 1 and 3 have
    x[:, :, 13:] *= np.float32(2.0 ** (12 * sign))      # their two rows of the previous block on one exponent and their own block on another
    return x


@pytest.mark.parametrize("sign", [1, -1])
def test_exponent_steps_at_block_boundaries(eng, sign):
    B, T, F = 2, 21, 64
    rng = np.random.default_rng(100 + sign)
    x = stepped_input(rng, B, 48, T, F, sign)
    w = (rng.standard_normal((48, 48, 3, 3)) / np.sqrt(9 * 48) * 10.0 ** rng.uniform(-1, 1, size=(48, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(48).astype(np.float32)
    y = conv3h(eng, x, w, b)
    assert np.array_equal(y, conv3h(eng, x, w, b)), "two runs differ"
    r, mag = ref64(x, w, b)
    q = np.abs(y - r) / (mag + 1e-30)
    print(f"exponent steps 2^{12 * sign:+d} at rows 5 and 13: max |y - ref| / sum |w||x| = {float(q.max()):.3e}, by row t % 4: "
          + ", ".join(f"{float(q[:, :, k::4].max()):.3e}" for k in range(4)))
    assert np.isfinite(y).all() and (np.abs(y - r) <= 2e-6 * mag + 1e-30).all(), float(q.max())


@pytest.mark.parametrize("c,T,F,spread", [(96, 18, 96, 2.0), (144, 16, 64, 0.0)])
def test_accumulate_form(eng, c, T, F, spread):
    rng = np.random.default_rng(c + T)
    x = rng.standard_normal((1, c, T, F)).astype(np.float32)
    if spread:
        tt, ff = np.meshgrid(np.arange(T), np.arange(F), indexing="ij")
        x *= (10.0 ** (spread * np.sin(0.013 * ff) * np.cos(0.21 * tt))).astype(np.float32)[None, None]
    w = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c) * 10.0 ** rng.uniform(-1, 1, size=(c, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    y = conv3h(eng, x, w, b, relu=True)
    assert np.array_equal(y, conv3h(eng, x, w, b, relu=True)), "two runs differ"
    r, mag = ref64(x, w, b, relu=True)
    q = np.abs(y - r) / (mag + 1e-30)
    print(f"{c} channels, T {T} F {F} spread {spread}: max |y - ref| / sum |w||x| = {float(q.max()):.3e}")
    assert np.isfinite(y).all() and (np.abs(y - r) <= 2e-6 * mag + 1e-30).all(), float(q.max())


def test_batch_invariance(eng):
    T, F = 21, 64
    rng = np.random.default_rng(7)
    x = stepped_input(rng, 3, 48, T, F, -1)
    w = (rng.standard_normal((48, 48, 3, 3)) / np.sqrt(9 * 48)).astype(np.float32)
    b = rng.standard_normal(48).astype(np.float32)
    alone = conv3h(eng, np.ascontiguousarray(x[1:2]), w, b, relu=True)
    batch = conv3h(eng, x, w, b, relu=True)
    assert np.isfinite(batch).all() and np.array_equal(alone[0], batch[1])
