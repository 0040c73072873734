"""conv3h_kernel's partial sums through the fragment-order scratch (csrc/kernels_conv3h.h, template parameter PS; engine option
"conv3h_partial_scratch") on the device, through `op_conv("conv3x3", ...)`: a 96- / 144-channel layer is 4 / 9 launches over 48-channel slices,
and the launches of one output slice hand their partial sum on through a private scratch in the consumer waves' own order (option 1, the
default) or through the output tensor in the planar layout (option 0).  The values and the order of the additions are the same, so the two
settings must agree BIT FOR BIT; the option-1 result is also held to the float64 convolution under the bound tests/test_gpu_conv3h_stage14.py
asserts for its 96- and 144-channel cases.  T = 4 is one tile row, 6 a ragged one (rows past T are never stored or loaded), 12 three tile rows
(deferred epilogues, the flush at the end of the walk).  Every case proves which kernel ran: the launch counter rises by (C / 48)^2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2e-6            # |y - ref| <= BOUND sum |w| |x|: the bar of tests/test_gpu_conv3h_stage14.py::test_accumulate_form


def make_engine():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    assert e.option("winograd") == 3 and e.option("conv_direct_f16x3") == 144 and e.option("gemm_f16x3") == 1
    assert e.option("conv3h_partial_scratch") == 1, "the scratch is the default"
    return e


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


def conv3h(eng, x, w, b, relu, scratch=1):
    c = x.shape[1]
    eng.set_option("conv3h_partial_scratch", scratch)
    try:
        n0 = eng.counter("conv3h_launches")
        y = eng.op_conv("conv3x3", x, w, b, relu=relu)
        assert eng.counter("conv3h_launches") - n0 == (c // 48) ** 2, "conv3h_kernel did not run n x n times"
    finally:
        eng.set_option("conv3h_partial_scratch", 1)
    return y


def ref64(x, w, b, relu):
    X, W, Bv = torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double()
    r = torch.nn.functional.conv2d(X, W, Bv, padding=1)
    mag = torch.nn.functional.conv2d(X.abs(), W.abs(), Bv.abs(), padding=1).numpy()
    return (torch.relu(r) if relu else r).numpy(), mag


def layer(seed, B, c, T, F):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    x *= (10.0 ** rng.uniform(-1, 1, size=(B, 1, T, 1))).astype(np.float32)       # rows of different loudness: the running exponent moves
    w = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c) * 10.0 ** rng.uniform(-1, 1, size=(c, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    return x, w, b


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("F", [32, 64])
@pytest.mark.parametrize("T", [4, 6, 12])
@pytest.mark.parametrize("c", [96, 144])
def test_scratch_equals_planar_bit_for_bit(eng, c, T, F, B, relu):
    x, w, b = layer(1000 * c + 100 * T + F + B, B, c, T, F)
    y1 = conv3h(eng, x, w, b, relu, scratch=1)
    y0 = conv3h(eng, x, w, b, relu, scratch=0)
    assert np.isfinite(y1).all()
    assert np.array_equal(bits(y1), bits(y0)), f"{int((bits(y1) != bits(y0)).sum())} of {y1.size} elements differ between the scratch and the planar form"
    r, mag = ref64(x, w, b, relu)
    q = np.abs(y1 - r) / (mag + 1e-30)
    print(f"{c} channels, B {B} T {T} F {F} relu {relu}: max |y - ref| / sum |w||x| = {float(q.max()):.3e}")
    assert (np.abs(y1 - r) <= BOUND * mag + 1e-30).all(), float(q.max())


def test_stale_scratch_of_a_larger_call_is_never_read(eng):
    """A 144-channel call at the largest shape leaves the scratch full of its partial sums; a 96-channel call at the smallest shape behind it
    must give what it gives on an engine whose scratch never held anything else."""
    big = layer(1, 3, 144, 12, 64)
    small = layer(2, 1, 96, 4, 32)
    conv3h(eng, *big, True)
    y = conv3h(eng, *small, True)
    fresh = make_engine()
    try:
        want = conv3h(fresh, *small, True)
    finally:
        fresh.close()
    assert np.isfinite(y).all() and np.array_equal(bits(y), bits(want))


@pytest.mark.parametrize("c", [96, 144])
def test_batch_invariance(eng, c):
    x, w, b = layer(3 + c, 3, c, 6, 64)
    alone = conv3h(eng, np.ascontiguousarray(x[1:2]), w, b, True)
    batch = conv3h(eng, x, w, b, True)
    assert np.isfinite(batch).all() and np.array_equal(bits(alone[0]), bits(batch[1]))
