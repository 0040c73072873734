"""The fused-output form of tdf3_kernel (csrc/kernels_gemm3.h, template flag CG, TdfCgMap; engine option "tdf_fuse_output"): the net's 1x1 output
conv (48 -> 4 channels) is computed in the epilogue of the last TDF block's second linear, on channel-grouped row tiles, instead of in a launch of
its own.  Small ConvTDFNets at g = 48 through the engine's net forward, fused (option 1, the default) against the two launches (option 0) and
against the float64 evaluation of the same net by the oracle's modules: which form ran, determinism, accuracy no worse than the unfused run,
alternating +1 / -1 output weights (a dropped channel or a bias added twice is O(1) wrong), a bit-equal fall-back wherever the form does not
apply, a NaN that stays inside its batch item, and a small call behind a large one.
Shapes: dim_f / 8 must be a multiple of 32 and at least 64 for the row GEMM to take the linears -- dim_f 512 and 768."""
import numpy as np
import pytest
import torch

from oracle import mdx_oracle as O
from tests.test_gpu_conv3h_fused_input import forward64, rel_rms, spec_input

pytestmark = pytest.mark.gpu

N_FFT = {512: 1024, 576: 1152, 768: 1536}


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


def make_net(A, dim_f, dim_t, num_blocks, g=48, norm="batch", seed=0, cancel=False):
    d = O.NetDims(dim_c=4, dim_f=dim_f, dim_t=dim_t, g=g, l=3, num_blocks=num_blocks, k=3, bn=8, norm=norm)
    sd = O.make_convtdf_state(d, seed=seed)
    if cancel:                                          # +1 / -1 on alternating channels, bias 3.0
        w = torch.ones_like(sd["final_conv.0.weight"])
        w[:, 1::2] = -1.0
        sd["final_conv.0.weight"] = w
        sd["final_conv.0.bias"] = torch.full_like(sd["final_conv.0.bias"], 3.0)
    n_fft = N_FFT[dim_f]
    eng = A.Engine(A.MDXConfig(n_fft=n_fft, hop_length=n_fft // 2, dim_f=dim_f, segment_size=dim_t, enable_denoise=False))
    eng.load_net(A.NetConfig(dim_c=4, dim_f=dim_f, dim_t=dim_t, g=g, l=3, num_blocks=num_blocks, k=3, bn=8, norm=norm),
                 A.fold_convtdf_state(sd, d.num_blocks, d.l))
    return eng, sd, d


def counted(eng, x):
    n0 = eng.counter("tdf_fused_output_launches")
    y = eng.net_forward(x)
    return y, eng.counter("tdf_fused_output_launches") - n0


def fused_and_not(eng, x):
    """(fused result, unfused result); asserts the counter with the option on and off and that two fused runs agree bit for bit"""
    assert eng.option("tdf_fuse_output") == 1, "the fused output is the default"
    y1, n1 = counted(eng, x)
    assert n1 == 1, f"{n1} fused-output launches in one net pass"
    y1b, _ = counted(eng, x)
    assert np.array_equal(y1, y1b), "two fused runs differ"
    eng.set_option("tdf_fuse_output", 0)
    y0, n0 = counted(eng, x)
    eng.set_option("tdf_fuse_output", 1)
    assert n0 == 0, f"{n0} fused-output launches with the option off"
    return y1, y0


# dim_f, dim_t, B, blocks, spread: one row tile, four column tiles, `mid` is the last block; two frame quads, the batch boundary, a decoder block
# last; six column tiles, three frame quads, three items, magnitudes over three decades (the rows' running exponents move)
@pytest.mark.parametrize("dim_f,dim_t,B,blocks,spread", [(512, 4, 1, 1, 0.0), (512, 8, 2, 3, 0.0), (768, 12, 3, 1, 3.0)])
def test_fused_output_vs_float64(A, dim_f, dim_t, B, blocks, spread):
    eng, sd, d = make_net(A, dim_f, dim_t, blocks, seed=dim_f + dim_t)
    x = spec_input(np.random.default_rng(dim_f * 100 + dim_t), B, dim_f, dim_t, spread)
    y1, y0 = fused_and_not(eng, x)
    ref = forward64(x, sd, d)
    e1, e0 = rel_rms(y1, ref), rel_rms(y0, ref)
    print(f"fused output, F {dim_f} T {dim_t} B {B} blocks {blocks} spread {spread}: rel-RMS vs float64 fused {e1:.3e}, two launches {e0:.3e}, "
          f"fused vs two launches {rel_rms(y1, y0):.3e}")
    assert np.isfinite(y1).all() and e1 <= 1.25 * e0 + 1e-8, (e1, e0)
    eng.close()


def test_fused_output_channel_cancellation(A):
    """Output weights +1 / -1 on alternating channels, bias 3.0: the 48 terms cancel, so the order of the sum shows, and a channel left out or
    counted twice, or the bias added once per lane instead of once, is wrong by O(1).  The whole output and every output channel on its own."""
    dim_f, dim_t, B = 512, 8, 2
    eng, sd, d = make_net(A, dim_f, dim_t, 1, seed=21, cancel=True)
    x = spec_input(np.random.default_rng(8), B, dim_f, dim_t)
    y1, y0 = fused_and_not(eng, x)
    ref = forward64(x, sd, d)
    for name, sl in [("all", slice(None))] + [(f"output channel {oc}", slice(oc, oc + 1)) for oc in range(4)]:
        e1, e0 = rel_rms(y1[:, sl], ref[:, sl]), rel_rms(y0[:, sl], ref[:, sl])
        print(f"fused output, channel cancellation, {name}: rel-RMS vs float64 fused {e1:.3e}, two launches {e0:.3e}")
        assert e1 <= 1.25 * e0 + 1e-8, (name, e1, e0)
    assert np.isfinite(y1).all()
    eng.close()


# GroupNorm (norm passes between the launches), 16 channels, a frame count off the quad grid, a width off the 128-column grid, the fp32 row GEMM
@pytest.mark.parametrize("dim_f,dim_t,blocks,g,norm,f16x3", [(512, 8, 3, 48, "group", 1), (512, 8, 3, 16, "batch", 1), (512, 10, 1, 48, "batch", 1),
                                                              (576, 8, 3, 48, "batch", 1), (512, 8, 3, 48, "batch", 0)])
def test_fused_output_falls_back(A, dim_f, dim_t, blocks, g, norm, f16x3):
    """where the form does not apply the two launches run whatever the option says: no fused launch, results equal bit for bit"""
    eng, sd, d = make_net(A, dim_f, dim_t, blocks, g=g, norm=norm, seed=9)
    if not f16x3:
        eng.set_option("gemm_f16x3", 0)
    x = spec_input(np.random.default_rng(4), 2, dim_f, dim_t)
    assert eng.option("tdf_fuse_output") == 1
    y1, n1 = counted(eng, x)
    eng.set_option("tdf_fuse_output", 0)
    y0, n0 = counted(eng, x)
    assert n1 == 0 and n0 == 0, (n1, n0)
    assert np.isfinite(y1).all() and np.array_equal(y1, y0)
    eng.close()


def test_fused_output_nan_stays_in_its_batch_item(A):
    dim_f, dim_t = 512, 8
    eng, sd, d = make_net(A, dim_f, dim_t, 1, seed=2)
    x = spec_input(np.random.default_rng(6), 2, dim_f, dim_t)
    clean = eng.net_forward(x)[1]
    x[0, 2, 17, 3] = np.nan
    y, n = counted(eng, x)
    assert n == 1
    assert np.isfinite(y[1]).all() and np.array_equal(y[1], clean), "the clean batch item was touched"
    eng.close()


def test_fused_output_small_call_behind_a_large_one(A):
    """a call of one item behind a call of three equals the same call on a fresh engine: no weight or destination argument outlives its launch"""
    dim_f, dim_t = 512, 8
    rng = np.random.default_rng(12)
    big, small = spec_input(rng, 3, dim_f, dim_t), spec_input(rng, 1, dim_f, dim_t)
    eng, sd, d = make_net(A, dim_f, dim_t, 3, seed=14)
    eng.net_forward(big)
    y, n = counted(eng, small)
    eng.close()
    fresh, _, _ = make_net(A, dim_f, dim_t, 3, seed=14)
    yf, nf = counted(fresh, small)
    fresh.close()
    assert n == 1 and nf == 1
    assert np.array_equal(y, yf)
