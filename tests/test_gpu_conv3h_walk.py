"""conv3h_kernel's table walk (csrc/conv3h_walk_plan.h, csrc/kernels_conv3h.h; engine option "conv3h_walk") on the device, through
`op_conv("conv3x3", ...)`.  A block's exponent is a function of the block alone, so nothing about the schedule may show in the results: the
balanced walk (option 1, the default) equals the arithmetic walk (option 0) BIT FOR BIT, item i of a batch equals the item alone whatever the
batch size (the planner cuts the leftover items of a batch into other pieces for every size), two runs agree, and a small call behind a large
one finds its own table.  The results are held to the float64 convolution under the bound of the other conv3h tests, also where the input steps
by 2^+-12 exactly at the edges of the four-row blocks (rows 4 k + 1) and at the edges of the tile rows, where units begin (rows 4 k).
F = 288 is nine strips (a band edge inside the plane); B = 3, 9, 11 leave item counts that are no multiple of the 8, 16 or 32 groups.  Every
case proves which kernel ran: the launch counter rises by (C / 48)^2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BOUND = 2e-6            # |y - ref| <= BOUND sum |w| |x|: the bar of tests/test_gpu_conv3h_stage14.py and tests/test_gpu_conv3h_partial_scratch.py

# C, T, F, B, relu: every C in {48, 96, 144}, T in {4, 16, 48}, F in {32, 64, 288}, B in {1, 3, 9, 11} and both activations occur, each C with
# each T and each F; the float64 reference of the largest case is 5 GFLOP
CASES = [(48, 4, 32, 1, True), (48, 16, 288, 3, False), (48, 48, 64, 11, True),
         (96, 16, 64, 9, True), (96, 48, 32, 3, False), (96, 4, 288, 11, False),
         (144, 4, 64, 9, False), (144, 16, 32, 11, True), (144, 48, 288, 1, True)]


def make_engine():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    assert e.option("winograd") == 3 and e.option("conv_direct_f16x3") == 144 and e.option("gemm_f16x3") == 1
    assert e.option("conv3h_walk") == 1, "the balanced walk is the default"
    return e


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


def conv3h(eng, x, w, b, relu, walk=1):
    c = x.shape[1]
    eng.set_option("conv3h_walk", walk)
    try:
        n0 = eng.counter("conv3h_launches")
        y = eng.op_conv("conv3x3", x, w, b, relu=relu)
        assert eng.counter("conv3h_launches") - n0 == (c // 48) ** 2, "conv3h_kernel did not run n x n times"
    finally:
        eng.set_option("conv3h_walk", 1)
    return y


def ref64(x, w, b, relu):
    X, W, Bv = torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double()
    r = torch.nn.functional.conv2d(X, W, Bv, padding=1)
    mag = torch.nn.functional.conv2d(X.abs(), W.abs(), Bv.abs(), padding=1).numpy()
    return (torch.relu(r) if relu else r).numpy(), mag


def layer(seed, B, c, T, F):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    x *= (10.0 ** rng.uniform(-1, 1, size=(B, 1, T, 1))).astype(np.float32)       # rows of different loudness: the block exponents differ
    w = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c) * 10.0 ** rng.uniform(-1, 1, size=(c, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    return x, w, b


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def hold_to_float64(tag, y, x, w, b, relu):
    r, mag = ref64(x, w, b, relu)
    q = np.abs(y - r) / (mag + 1e-30)
    print(f"{tag}: max |y - ref| / sum |w||x| = {float(q.max()):.3e}")
    assert np.isfinite(y).all() and (np.abs(y - r) <= BOUND * mag + 1e-30).all(), float(q.max())


@pytest.mark.parametrize("c,T,F,B,relu", CASES)
def test_walks_agree_and_items_do_not_see_the_batch(eng, c, T, F, B, relu):
    x, w, b = layer(1000 * c + 100 * T + F + B, B, c, T, F)
    y1 = conv3h(eng, x, w, b, relu, walk=1)
    y0 = conv3h(eng, x, w, b, relu, walk=0)
    assert np.isfinite(y1).all()
    assert np.array_equal(bits(y1), bits(y0)), f"{int((bits(y1) != bits(y0)).sum())} of {y1.size} elements differ between the balanced and the arithmetic walk"
    assert np.array_equal(bits(y1), bits(conv3h(eng, x, w, b, relu, walk=1))), "two runs differ"
    for i in range(B):                                           # every item: the planner cuts the leftover ones, wherever they sit in the batch
        alone = conv3h(eng, np.ascontiguousarray(x[i:i + 1]), w, b, relu, walk=1)
        assert np.array_equal(bits(alone[0]), bits(y1[i])), f"item {i} of {B} differs from the item alone"
    hold_to_float64(f"{c} channels, B {B} T {T} F {F} relu {relu}", y1, x, w, b, relu)


@pytest.mark.parametrize("c,B", [(48, 3), (96, 9)])
@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("edge", ["block", "unit"])
def test_steps_of_2_to_the_12_at_block_and_unit_edges(eng, c, B, sign, edge):
    """Rows 4 k + 1 open the four-row blocks (each block then holds one level and differs from its neighbours by 2^12); rows 4 k open the tile
    rows, where the planner may begin a unit (a block then holds both levels)."""
    T, F = 16, 64
    rng = np.random.default_rng(7 * c + B + (sign > 0) + 2 * (edge == "unit"))
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    first = 5 if edge == "block" else 4
    x[:, :, first:] *= np.float32(2.0 ** (12 * sign))
    x[:, :, first + 4:] *= np.float32(2.0 ** (-12 * sign))
    x[:, :, first + 8:] *= np.float32(2.0 ** (12 * sign))
    w = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c) * 10.0 ** rng.uniform(-1, 1, size=(c, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    y1 = conv3h(eng, x, w, b, False, walk=1)
    y0 = conv3h(eng, x, w, b, False, walk=0)
    assert np.array_equal(bits(y1), bits(y0))
    hold_to_float64(f"{c} channels, steps of 2^{12 * sign} at {edge} edges", y1, x, w, b, False)


def test_a_small_call_behind_a_large_one_walks_its_own_table(eng):
    big = layer(1, 11, 144, 16, 64)
    small = layer(2, 1, 96, 4, 32)
    conv3h(eng, *big, True)
    y = conv3h(eng, *small, True)
    fresh = make_engine()
    try:
        want = conv3h(fresh, *small, True)
    finally:
        fresh.close()
    assert np.isfinite(y).all() and np.array_equal(bits(y), bits(want))
