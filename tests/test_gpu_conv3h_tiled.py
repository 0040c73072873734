"""conv3h_kernel's tile order (csrc/kernels_conv3h.h, template flags XT / YT; engine option "conv3h_tiled") on the device: the tensors between
the 3x3 convs of a TFC block travel in the kernel's own layout (Conv3hCfg::tl_off) instead of planar.  Same accumulators, same lanes, same
values, another address -- so everything here is equality on the uint32 view against the planar form, through the single-layer hooks
`op_conv("conv3x3_to_tiled" / "conv3x3_tiled" / "conv3x3_from_tiled", ...)`, whose raw buffers the numpy `pack` / `unpack` of
tests/test_conv3h_tiled_host.py (built from the compiled map) translate.  The planar chain itself is held to the float64 convolution per layer
under the bar of tests/test_gpu_conv3h_walk.py.  F = 32: both halo quads outside the image; F = 96: a middle strip with both halos read from
neighbours' blocks; T = 4: one tile row, every block borders the padding; 96 / 144 channels: every partial-sum form with a tile-order input or
final output.  Every case proves which kernels ran by the launch counters."""
import itertools

import numpy as np
import pytest
import torch

from oracle import mdx_oracle as O
from tests import test_conv3h_tiled_host as H
from tests.test_gpu_conv3h_fused_input import make_net, spec_input

pytestmark = pytest.mark.gpu

BOUND = 2e-6            # |y - ref| <= BOUND sum |w| |x| per layer: the bar of tests/test_gpu_conv3h_walk.py

SHAPES = list(itertools.product((48, 96, 144), (4, 8, 12), (32, 64, 96), (1, 3)))   # C, T, F, B


def make_engine():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    assert e.option("winograd") == 3 and e.option("conv_direct_f16x3") == 144 and e.option("gemm_f16x3") == 1 and e.option("conv3h_partial_scratch") == 1
    assert e.option("conv3h_tiled") == 1, "tile order between the 3x3 convs of a block is the default"
    return e


@pytest.fixture(scope="module")
def eng():
    e = make_engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def offs(tmp_path_factory):
    """(T, F) -> the compiled map of one 48-channel slice, [48, T, F] byte offsets"""
    exe = H.build_map_program(str(tmp_path_factory.mktemp("tl3h_gpu")))
    assert exe is not None, "g++ is needed to compile the layout map out of the header"
    cache = {}

    def get(T, F):
        if (T, F) not in cache:
            cache[(T, F)] = H.read_map(exe, T, F)["off"]
        return cache[(T, F)]
    return get


def bits(y):
    return np.ascontiguousarray(y).view(np.uint32)


def conv(eng, op, x, w, b, relu):
    """one layer; the counters say conv3h_kernel ran n x n times, and how many of the launches had a tile-order side"""
    n = x.shape[1] // 48
    n0, t0 = eng.counter("conv3h_launches"), eng.counter("conv3h_tiled_launches")
    y = eng.op_conv(op, x, w, b, relu=relu)
    assert eng.counter("conv3h_launches") - n0 == n * n, "conv3h_kernel did not run n x n times"
    # tile-order input: every launch reads it; tile-order output alone: the last input slice's launch of every output slice writes it
    want = {"conv3x3": 0, "conv3x3_to_tiled": n, "conv3x3_tiled": n * n, "conv3x3_from_tiled": n * n}[op]
    assert eng.counter("conv3h_tiled_launches") - t0 == want, (op, eng.counter("conv3h_tiled_launches") - t0, want)
    return y


def layers(seed, c, n=3):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        w = (rng.standard_normal((c, c, 3, 3)) / np.sqrt(9 * c) * 10.0 ** rng.uniform(-1, 1, size=(c, 1, 1, 1))).astype(np.float32)
        out.append((w, rng.standard_normal(c).astype(np.float32)))
    return out


def hold_to_float64(tag, y, x, w, b, relu):
    X, W, Bv = torch.from_numpy(x).double(), torch.from_numpy(w).double(), torch.from_numpy(b).double()
    r = torch.nn.functional.conv2d(X, W, Bv, padding=1)
    mag = torch.nn.functional.conv2d(X.abs(), W.abs(), Bv.abs(), padding=1).numpy()
    r = (torch.relu(r) if relu else r).numpy()
    q = np.abs(y - r) / (mag + 1e-30)
    print(f"{tag}: max |y - ref| / sum |w||x| = {float(q.max()):.3e}")
    assert np.isfinite(y).all() and (np.abs(y - r) <= BOUND * mag + 1e-30).all(), float(q.max())


def chains(eng, off, x, ws, relu, tag=None):
    """the planar chain of three layers and the same chain through tile order; checks (a), (b), (c) of the module text; returns the final output"""
    p = [x]
    for w, b in ws:
        p.append(conv(eng, "conv3x3", p[-1], w, b, relu))
        if tag:
            hold_to_float64(f"{tag} layer {len(p) - 1}", p[-1], p[-2], w, b, relu)
    t1 = conv(eng, "conv3x3_to_tiled", x, *ws[0], relu)
    assert np.array_equal(bits(H.unpack(t1, off)), bits(p[1])), "(a) a tile-order output, unpacked, is not the planar output"
    y2 = conv(eng, "conv3x3_from_tiled", H.pack(p[1], off), *ws[1], relu)
    assert np.array_equal(bits(y2), bits(p[2])), "(b) a layer reading a packed input differs from the planar layer"
    t2 = conv(eng, "conv3x3_tiled", t1, *ws[1], relu)
    assert np.array_equal(bits(H.unpack(t2, off)), bits(p[2])), "(c) the middle layer, tile order on both sides"
    y3 = conv(eng, "conv3x3_from_tiled", t2, *ws[2], relu)
    assert np.array_equal(bits(y3), bits(p[3])), "(c) the chain to_tiled -> tiled -> from_tiled differs from the planar chain"
    return y3


def rows_of_different_loudness(rng, B, c, T, F):
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    return x * (10.0 ** rng.uniform(-1, 1, size=(B, 1, T, 1))).astype(np.float32)   # the block exponents differ


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("c,T,F,B", SHAPES)
def test_tile_order_equals_planar_layer_by_layer_and_as_a_chain(eng, offs, c, T, F, B, relu):
    seed = 1000 * c + 100 * T + F + B
    x = rows_of_different_loudness(np.random.default_rng(seed), B, c, T, F)
    chains(eng, offs(T, F), x, layers(seed + 1, c), relu, tag=f"{c} channels, B {B} T {T} F {F} relu {relu}")


@pytest.mark.parametrize("c", [48, 96, 144])
@pytest.mark.parametrize("sign", [1, -1])
def test_steps_of_2_to_the_12_at_block_and_strip_edges(eng, offs, c, sign):
    """(d) the input steps by 2^+-12 at rows 4 k + 1 (the four-row blocks), at rows 4 k (the tile rows) and at columns 32 k and 32 k - 1 (the
    strips: the halo column of a strip then lies on the other level, in a neighbour's block of the tile-order tensor)"""
    T, F, B = 12, 96, 3
    rng = np.random.default_rng(7 * c + (sign > 0))
    x = rng.standard_normal((B, c, T, F)).astype(np.float32)
    s = np.float32(2.0 ** (12 * sign))
    x[0, :, 5:9] *= s                                            # item 0: block edges
    x[1, :, 4:8] *= s                                            # item 1: tile-row edges
    x[2, :, :, 32:64] *= s                                       # item 2: strip edges ...
    x[2, :, :, 31] *= s                                          # ... and one column early on the left
    chains(eng, offs(T, F), x, layers(c, c), False, tag=f"{c} channels, steps of 2^{12 * sign}")


@pytest.mark.parametrize("c", [48, 96, 144])
def test_item_1_of_3_equals_the_item_alone(eng, offs, c):
    T, F = 8, 96
    x = rows_of_different_loudness(np.random.default_rng(c), 3, c, T, F)
    ws = layers(c + 1, c)
    y = chains(eng, offs(T, F), x, ws, True)
    alone = chains(eng, offs(T, F), np.ascontiguousarray(x[1:2]), ws, True)
    assert np.array_equal(bits(alone[0]), bits(y[1]))


def test_a_small_call_behind_a_large_one_equals_a_fresh_engine(eng, offs):
    big = rows_of_different_loudness(np.random.default_rng(1), 3, 144, 12, 96)
    small = rows_of_different_loudness(np.random.default_rng(2), 1, 96, 4, 32)
    ws = layers(3, 96)
    chains(eng, offs(12, 96), big, layers(4, 144), True)
    y = chains(eng, offs(4, 32), small, ws, True)
    fresh = make_engine()
    try:
        want = chains(fresh, offs(4, 32), small, ws, True)
    finally:
        fresh.close()
    assert np.isfinite(y).all() and np.array_equal(bits(y), bits(want))


def net_forward_counted(e, x, tiled):
    e.set_option("conv3h_tiled", tiled)
    try:
        n0 = e.counter("conv3h_tiled_launches")
        y = e.net_forward(x)
        return y, e.counter("conv3h_tiled_launches") - n0
    finally:
        e.set_option("conv3h_tiled", 1)


def test_net_forward_tiled_equals_planar_and_counts_the_planned_launches():
    """(g) a ConvTDFNet at g = 48, F 64 x T 8, three blocks of three 3x3 convs: two blocks of 48 channels at 64 x 8 and the middle one of 96
    channels at 32 x 4.  In a block of n slices the first conv writes tile order in n launches (the last input slice's, per output slice), the
    second reads and writes it and the third reads it in n x n launches each: 3 + 10 + 3."""
    import audio_separator_amd as A
    e, sd, d = make_net(A, 64, 8, 3, seed=21)
    try:
        assert e.option("conv3h_tiled") == 1
        x = spec_input(np.random.default_rng(5), 2, 64, 8, spread=2.0)
        y1, n1 = net_forward_counted(e, x, 1)
        y0, n0 = net_forward_counted(e, x, 0)
        assert n0 == 0 and n1 == (1 + 2 * 1) + (2 + 2 * 4) + (1 + 2 * 1), (n0, n1)
        assert np.isfinite(y1).all() and np.array_equal(bits(y1), bits(y0)), "the net's output depends on the layout of its private intermediates"
        assert np.array_equal(bits(net_forward_counted(e, x, 1)[0]), bits(y1)), "two runs differ"
        ref = O.convtdf_forward(x, sd, d)
        err = float(np.sqrt(np.mean((y1.astype(np.float64) - ref) ** 2)) / np.sqrt(np.mean(np.asarray(ref, np.float64) ** 2)))
        assert err < 2e-5, err
    finally:
        e.close()


@pytest.mark.parametrize("dim_t,norm", [(8, "group"), (10, "batch")])
def test_net_forward_stays_planar_where_the_layout_does_not_apply(dim_t, norm):
    """GroupNorm reads the planar tensor between the convs; T % 4 != 0 (10 rows, 5 a level down) leaves ragged tile rows: no tile-order launch"""
    import audio_separator_amd as A
    e, sd, d = make_net(A, 64, dim_t, 3, norm=norm, seed=22)
    try:
        x = spec_input(np.random.default_rng(6), 2, 64, dim_t)
        y1, n1 = net_forward_counted(e, x, 1)
        y0, n0 = net_forward_counted(e, x, 0)
        assert n1 == 0 and n0 == 0
        assert np.array_equal(bits(y1), bits(y0))
    finally:
        e.close()
