"""conv3h_kernel's merged output slices (csrc/kernels_conv3h.h, Conv3hArgs::nob; engine option "conv3h_merge_out") on the device, through
`op_conv("conv3x3", ...)`: with the option at 144 a 96- / 144-channel layer is 2 / 3 dispatches, one per 48-channel INPUT slice, each running
the 2 / 3 output slices side by side on groups of workgroups that walk together; with 0 it is the 4 / 9 launches of before.  A lane adds the
same values in the same order either way, so the two settings must agree BIT FOR BIT, and both are held to the float64 convolution under the
bar of the other conv3h tests.  T = 4 is one tile row, 6 a ragged one, 12 three tile rows (deferred epilogues, the flush at the end of the
walk); F = 288 is nine strips: bands with padding strips at every band width; B = 11: the leftover items are cut into pieces and the walkers'
lists have unequal lengths.  Counter "conv3h_launches" counts (output slice, input slice) pairs in both settings, "conv3h_merged_dispatches"
the merged dispatches."""
import numpy as np
import pytest
import torch

from tests.test_gpu_conv3h_fused_input import make_net, spec_input

pytestmark = pytest.mark.gpu

BOUND = 2e-6            # |y - ref| <= BOUND sum |w| |x|: the bar of tests/test_gpu_conv3h_partial_scratch.py


def make_engine():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    assert e.option("winograd") == 3 and e.option("conv_direct_f16x3") == 144 and e.option("gemm_f16x3") == 1
    assert e.option("conv3h_partial_scratch") == 1 and e.option("conv3h_walk") == 1
    return e


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    default = e.option("conv3h_merge_out")
    yield e
    assert e.option("conv3h_merge_out") == default, "a test left the option changed"
    e.close()


def conv3h(eng, x, w, b, relu, merge, scratch=1, op="conv3x3"):
    """one layer under "conv3h_merge_out" = merge; the counters say how it ran: n x n (output slice, input slice) pairs, in n merged dispatches or none"""
    n = x.shape[1] // 48
    default = eng.option("conv3h_merge_out")
    eng.set_option("conv3h_merge_out", merge)
    eng.set_option("conv3h_partial_scratch", scratch)
    try:
        n0, m0 = eng.counter("conv3h_launches"), eng.counter("conv3h_merged_dispatches")
        y = eng.op_conv(op, x, w, b, relu=relu)
        assert eng.counter("conv3h_launches") - n0 == n * n, "conv3h_kernel did not run n x n slice pairs"
        want = n if merge >= x.shape[1] and scratch else 0
        assert eng.counter("conv3h_merged_dispatches") - m0 == want, (eng.counter("conv3h_merged_dispatches") - m0, want)
    finally:
        eng.set_option("conv3h_partial_scratch", 1)
        eng.set_option("conv3h_merge_out", default)
    return y


def ref64(x, w, b):
    """the float64 convolution (before the activation) and sum |w| |x| + |b|, tap by tap on the device"""
    X = torch.nn.functional.pad(torch.from_numpy(x).cuda().double(), (1, 1, 1, 1))
    W, Bv = torch.from_numpy(w).cuda().double(), torch.from_numpy(b).cuda().double()
    T, F = x.shape[2], x.shape[3]
    r = Bv.view(1, -1, 1, 1).expand(x.shape[0], -1, T, F).clone()
    mag = r.abs()
    for ky in range(3):
        for kx in range(3):
            xs = X[:, :, ky:ky + T, kx:kx + F]
            r += torch.einsum("oc,bctf->botf", W[:, :, ky, kx], xs)
            mag += torch.einsum("oc,bctf->botf", W[:, :, ky, kx].abs(), xs.abs())
    return r.cpu().numpy(), mag.cpu().numpy()


def layer(seed, B, c, T, F):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    x *= (10.0 ** rng.uniform(-1, 1, size=(B, 1, T, 1))).astype(np.float32)       # rows of different loudness: the block exponents differ
    w = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c) * 10.0 ** rng.uniform(-1, 1, size=(c, 1, 1, 1))).astype(np.float32)
    b = rng.standard_normal(c).astype(np.float32)
    return x, w, b


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


@pytest.mark.parametrize("B", [1, 3, 11])
@pytest.mark.parametrize("F", [32, 64, 288])
@pytest.mark.parametrize("T", [4, 6, 12])
@pytest.mark.parametrize("c", [96, 144])
def test_merged_equals_n_by_n_bit_for_bit_and_float64(eng, c, T, F, B):
    x, w, b = layer(1000 * c + 100 * T + F + B, B, c, T, F)
    r, mag = ref64(x, w, b)                                      # once for both activations
    for relu in (False, True):
        y1 = conv3h(eng, x, w, b, relu, merge=144)
        y0 = conv3h(eng, x, w, b, relu, merge=0)
        assert np.isfinite(y1).all()
        assert np.array_equal(bits(y1), bits(y0)), f"{int((bits(y1) != bits(y0)).sum())} of {y1.size} elements differ between the merged and the n x n form"
        want = np.maximum(r, 0.0) if relu else r
        for tag, y in (("merged", y1), ("n x n", y0)):
            q = np.abs(y - want) / (mag + 1e-30)
            print(f"{c} channels, B {B} T {T} F {F} relu {relu}, {tag}: max |y - ref| / sum |w||x| = {float(q.max()):.3e}")
            assert (np.abs(y - want) <= BOUND * mag + 1e-30).all(), float(q.max())


@pytest.mark.parametrize("c,merge", [(96, 96), (144, 96), (96, 144)])
def test_the_option_is_a_channel_count(eng, c, merge):
    """96: the 96-channel layers are merged, a 144-channel layer runs its nine launches (conv3h asserts the counters)"""
    x, w, b = layer(5 + c + merge, 3, c, 6, 64)
    assert np.array_equal(bits(conv3h(eng, x, w, b, True, merge=merge)), bits(conv3h(eng, x, w, b, True, merge=0)))


@pytest.mark.parametrize("c", [96, 144])
def test_two_runs_agree(eng, c):
    x, w, b = layer(7 + c, 11, c, 12, 288)
    assert np.array_equal(bits(conv3h(eng, x, w, b, True, merge=144)), bits(conv3h(eng, x, w, b, True, merge=144)))


@pytest.mark.parametrize("c", [96, 144])
def test_every_item_of_a_batch_equals_the_item_alone(eng, c):
    x, w, b = layer(3 + c, 11, c, 6, 64)
    batch = conv3h(eng, x, w, b, True, merge=144)
    assert np.isfinite(batch).all()
    for i in range(x.shape[0]):
        alone = conv3h(eng, np.ascontiguousarray(x[i:i + 1]), w, b, True, merge=144)
        assert np.array_equal(bits(alone[0]), bits(batch[i])), i


def test_stale_scratch_of_another_output_slice_is_never_read(eng):
    """A 144-channel call at a large shape leaves all three scratches full of its partial sums; a small 96-channel call behind it must give
    what it gives on an engine whose scratches never held anything else."""
    big = layer(1, 3, 144, 12, 288)
    small = layer(2, 1, 96, 4, 32)
    conv3h(eng, *big, True, merge=144)
    y = conv3h(eng, *small, True, merge=144)
    fresh = make_engine()
    try:
        want = conv3h(fresh, *small, True, merge=144)
    finally:
        fresh.close()
    assert np.isfinite(y).all() and np.array_equal(bits(y), bits(want))


@pytest.mark.parametrize("c", [96, 144])
def test_planar_partial_sums_run_n_by_n_with_merging_on(eng, c):
    """the merged form needs the scratch: "conv3h_partial_scratch" = 0 runs n x n launches whatever "conv3h_merge_out" says, and equals the default"""
    x, w, b = layer(11 + c, 3, c, 12, 64)
    y = conv3h(eng, x, w, b, True, merge=144, scratch=0)         # (asserts n x n pairs and no merged dispatch)
    assert np.array_equal(bits(y), bits(conv3h(eng, x, w, b, True, merge=eng.option("conv3h_merge_out"))))


@pytest.mark.parametrize("c,T,F,B", [(96, 4, 32, 1), (96, 12, 96, 3), (144, 8, 64, 3), (144, 12, 288, 11)])
def test_tile_order_sides(eng, c, T, F, B):
    """the three layers of a TFC block through the single-layer hooks: planar -> tile order, tile order on both sides, tile order -> planar;
    the raw buffers of every layer equal bit for bit with merging on and off"""
    rng = np.random.default_rng(c + T + F + B)
    ws = [layer(int(rng.integers(1 << 30)), 1, c, 4, 32)[1:] for _ in range(3)]
    x = layer(c * T + F + B, B, c, T, F)[0]
    outs = {}
    for merge in (144, 0):
        t1 = conv3h(eng, x, *ws[0], True, merge=merge, op="conv3x3_to_tiled")
        t2 = conv3h(eng, t1, *ws[1], True, merge=merge, op="conv3x3_tiled")
        outs[merge] = (t1, t2, conv3h(eng, t2, *ws[2], True, merge=merge, op="conv3x3_from_tiled"))
    for k, name in enumerate(("planar -> tile order", "tile order -> tile order", "tile order -> planar")):
        assert np.isfinite(outs[144][k]).all() and np.array_equal(bits(outs[144][k]), bits(outs[0][k])), name


def test_net_forward_merged_equals_n_by_n():
    """a ConvTDFNet at g = 48, F 64 x T 8, three blocks: the middle one has three 96-channel convs at 32 x 4, tile order between them -- two
    merged dispatches each with the option on, none with it off, the same bits"""
    import audio_separator_amd as A
    e, sd, d = make_net(A, 64, 8, 3, seed=23)
    try:
        default = e.option("conv3h_merge_out")
        x = spec_input(np.random.default_rng(9), 2, 64, 8, spread=2.0)
        out = {}
        for merge in (144, 0):
            e.set_option("conv3h_merge_out", merge)
            m0 = e.counter("conv3h_merged_dispatches")
            out[merge] = e.net_forward(x)
            assert e.counter("conv3h_merged_dispatches") - m0 == (3 * 2 if merge else 0)
        e.set_option("conv3h_merge_out", default)
        assert np.isfinite(out[144]).all() and np.array_equal(bits(out[144]), bits(out[0]))
    finally:
        e.close()
