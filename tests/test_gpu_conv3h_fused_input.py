"""The fused-input form of conv3h_kernel (csrc/kernels_conv3h.h, template flag FIN; engine option "conv_fuse_input"): the net's 1x1 input
conv (4 -> 48 channels, folded BatchNorm, ReLU) is computed by the producer waves of the first TFC conv's launch instead of in a launch of its
own.  Small ConvTDFNets at g = 48 through the engine's net forward / run_model, fused (option 1, the default) against the two launches
(option 0) and against the float64 evaluation of the same net by the oracle's modules: which kernel ran, determinism, accuracy no worse than
the unfused run, the zero padding of the 48-channel activation (not relu(bias)) on the rim, running-exponent rescales fed by computed values,
a clean fall-back where the form does not apply, and a NaN input that stays inside its batch item."""
import numpy as np
import pytest
import torch

from oracle import mdx_oracle as O

pytestmark = pytest.mark.gpu


def rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


@torch.no_grad()
def forward64(x, sd, d):
    """ConvTDFNet.forward as oracle.mdx_oracle.convtdf_forward states it, on float64 tensors."""
    sd = {k: v.double() for k, v in sd.items()}
    x = torch.from_numpy(np.ascontiguousarray(x)).double()
    x = torch.relu(O._bn(torch.nn.functional.conv2d(x, sd["first_conv.0.weight"], sd["first_conv.0.bias"]), sd, "first_conv.1"))
    x = x.transpose(-1, -2)
    skips = []
    for i in range(d.n):
        x = O._tfc_tdf(x, sd, f"encoding_blocks.{i}", d)
        skips.append(x)
        x = torch.relu(O._bn(torch.nn.functional.conv2d(x, sd[f"ds.{i}.0.weight"], sd[f"ds.{i}.0.bias"], stride=2), sd, f"ds.{i}.1"))
    x = O._tfc_tdf(x, sd, "bottleneck_block", d)
    for i in range(d.n):
        x = torch.relu(O._bn(torch.nn.functional.conv_transpose2d(x, sd[f"us.{i}.0.weight"], sd[f"us.{i}.0.bias"], stride=2), sd, f"us.{i}.1"))
        x = x * skips[-i - 1]
        x = O._tfc_tdf(x, sd, f"decoding_blocks.{i}", d)
    x = x.transpose(-1, -2)
    return torch.nn.functional.conv2d(x, sd["final_conv.0.weight"], sd["final_conv.0.bias"]).numpy()


def mdx_cfg(A, dim_f, dim_t, denoise=False):
    # the net forward needs no transform: any valid STFT geometry with this dim_f / segment (n_fft / 2 a product of 2, 3, 5; chunk longer than n_fft)
    n_fft = {32: 64, 64: 128, 96: 192, 1088: 2304}[dim_f]
    return A.MDXConfig(n_fft=n_fft, hop_length=n_fft // 2, dim_f=dim_f, segment_size=dim_t, enable_denoise=denoise)


def make_net(A, dim_f, dim_t, num_blocks, g=48, norm="batch", seed=0, first_bias=None, denoise=False):
    d = O.NetDims(dim_c=4, dim_f=dim_f, dim_t=dim_t, g=g, l=3, num_blocks=num_blocks, k=3, bn=8, norm=norm)
    sd = O.make_convtdf_state(d, seed=seed)
    if first_bias is not None:                          # the FOLDED bias of the input conv, on every channel (through the BatchNorm shift)
        folded = A.fold_convtdf_state(sd, d.num_blocks, d.l)
        sd["first_conv.1.bias"] = sd["first_conv.1.bias"] + (first_bias - torch.as_tensor(np.asarray(folded["first.b"], np.float32)))
    eng = A.Engine(mdx_cfg(A, dim_f, dim_t, denoise))
    eng.load_net(A.NetConfig(dim_c=4, dim_f=dim_f, dim_t=dim_t, g=g, l=3, num_blocks=num_blocks, k=3, bn=8, norm=norm),
                 A.fold_convtdf_state(sd, d.num_blocks, d.l))
    if first_bias is not None:
        assert np.allclose(np.asarray(A.fold_convtdf_state(sd, d.num_blocks, d.l)["first.b"]), first_bias, atol=1e-5)
    return eng, sd, d


def counted(eng, run):
    n3, nf = eng.counter("conv3h_launches"), eng.counter("conv3h_fin_launches")
    y = run()
    return y, eng.counter("conv3h_launches") - n3, eng.counter("conv3h_fin_launches") - nf


def fused_and_not(eng, run):
    """(fused result, unfused result); asserts the counters of item 1 of the issue and the determinism of item 2"""
    assert eng.option("conv_fuse_input") == 1, "the fused input is the default"
    y1, n3_1, nf_1 = counted(eng, run)
    assert nf_1 == 1, f"{nf_1} fused-input launches in one net pass"
    y1b, _, _ = counted(eng, run)
    assert np.array_equal(y1, y1b), "two fused runs differ"
    eng.set_option("conv_fuse_input", 0)
    y0, n3_0, nf_0 = counted(eng, run)
    eng.set_option("conv_fuse_input", 1)
    assert nf_0 == 0 and n3_0 == n3_1 and n3_1 >= 1, (n3_0, n3_1, nf_0)
    return y1, y0


def spec_input(rng, B, dim_f, dim_t, spread=0.0):
    x = rng.standard_normal((B, 4, dim_f, dim_t)).astype(np.float32)
    if spread:                                          # magnitudes varying by `spread` decades over the plane (the construction of test_conv3x3_direct_f16x3)
        ff, tt = np.meshgrid(np.arange(dim_f), np.arange(dim_t), indexing="ij")
        x *= (10.0 ** (spread * np.sin(0.013 * ff) * np.cos(0.21 * tt))).astype(np.float32)[None, None]
    return x


# dim_f, dim_t, B, blocks, spread: one tile where every pixel touches padding; ragged T (bottom-row predicate); several tiles per walk and
# batch items, magnitudes over 3 decades (rescales); more than 32 strips (band walk, right edge).  Odd T: one block (no 2 x 2 down conv).
@pytest.mark.parametrize("dim_f,dim_t,B,blocks,spread", [(32, 4, 1, 3, 0.0), (64, 10, 2, 3, 0.0), (96, 37, 3, 1, 3.0), (1088, 5, 1, 1, 0.0)])
def test_fused_input_vs_float64(A, dim_f, dim_t, B, blocks, spread):
    eng, sd, d = make_net(A, dim_f, dim_t, blocks, seed=dim_f + dim_t)
    x = spec_input(np.random.default_rng(dim_f * 100 + dim_t), B, dim_f, dim_t, spread)
    y1, y0 = fused_and_not(eng, lambda: eng.net_forward(x))
    ref = forward64(x, sd, d)
    e1, e0 = rel_rms(y1, ref), rel_rms(y0, ref)
    print(f"fused input, F {dim_f} T {dim_t} B {B} blocks {blocks} spread {spread}: rel-RMS vs float64 fused {e1:.3e}, two launches {e0:.3e}")
    assert np.isfinite(y1).all() and e1 <= 1.25 * e0 + 1e-8, (e1, e0)


def test_fused_input_denoise_run_model(A):
    """enable_denoise: the batch doubled with the negated spectrogram, through run_model"""
    dim_f, dim_t, B = 64, 16, 2
    eng, sd, d = make_net(A, dim_f, dim_t, 3, seed=7, denoise=True)
    p = O.MDXParams(n_fft=128, hop_length=64, dim_f=dim_f, segment_size=dim_t, enable_denoise=True)
    w = (0.3 * np.random.default_rng(11).standard_normal((B, 2, p.chunk_size))).astype(np.float32)
    y1, y0 = fused_and_not(eng, lambda: eng.run_model(w))
    ref = O.run_model(w, p, lambda spek: forward64(np.asarray(spek, np.float32), sd, d))
    e1, e0 = rel_rms(y1, ref), rel_rms(y0, ref)
    print(f"fused input, denoise run_model: rel-RMS vs float64 net fused {e1:.3e}, two launches {e0:.3e}")
    assert np.isfinite(y1).all() and e1 <= 1.25 * e0 + 1e-8, (e1, e0)


def test_fused_input_padding_canary(A):
    """Folded input-conv bias + 3.0 on every channel: relu(b1) > 0 everywhere, so padding the 3x3 conv with relu(b1) instead of 0 is wrong by
    O(1) on the whole rim.  One block: the net's output pixels depend on the rim of the first conv directly.  Rim and interior to one bar."""
    dim_f, dim_t, B = 64, 10, 2
    eng, sd, d = make_net(A, dim_f, dim_t, 1, seed=5, first_bias=3.0)
    x = spec_input(np.random.default_rng(3), B, dim_f, dim_t)
    y1, y0 = fused_and_not(eng, lambda: eng.net_forward(x))
    ref = forward64(x, sd, d)
    rim = np.zeros((dim_f, dim_t), bool)
    rim[[0, -1], :] = True
    rim[:, [0, -1]] = True
    for name, m in (("rim rows t", np.isin(np.arange(dim_t), [0, dim_t - 1])[None, :] & np.ones((dim_f, 1), bool)),
                    ("rim columns f", np.isin(np.arange(dim_f), [0, dim_f - 1])[:, None] & np.ones((1, dim_t), bool)), ("interior", ~rim)):
        e1, e0 = rel_rms(y1[:, :, m], ref[:, :, m]), rel_rms(y0[:, :, m], ref[:, :, m])
        print(f"fused input, padding canary, {name}: rel-RMS vs float64 fused {e1:.3e}, two launches {e0:.3e}")
        assert e1 <= 1.25 * e0 + 1e-8, (name, e1, e0)


@pytest.mark.parametrize("g,norm", [(48, "group"), (16, "batch")])
def test_fused_input_falls_back(A, g, norm):
    """GroupNorm between the two convs, or a width the kernel does not take: the two launches run whatever the option says"""
    dim_f, dim_t = 64, 8
    eng, sd, d = make_net(A, dim_f, dim_t, 3, g=g, norm=norm, seed=9)
    x = spec_input(np.random.default_rng(4), 2, dim_f, dim_t)
    y1, _, nf1 = counted(eng, lambda: eng.net_forward(x))
    eng.set_option("conv_fuse_input", 0)
    y0, _, nf0 = counted(eng, lambda: eng.net_forward(x))
    assert nf1 == 0 and nf0 == 0
    assert np.array_equal(y1, y0)
    assert rel_rms(y1, O.convtdf_forward(x, sd, d)) < 2e-5


def test_fused_input_nan_stays_in_its_batch_item(A):
    dim_f, dim_t = 64, 10
    eng, sd, d = make_net(A, dim_f, dim_t, 1, seed=2)
    x = spec_input(np.random.default_rng(6), 2, dim_f, dim_t)
    clean = eng.net_forward(x)[1]
    x[0, 2, 17, 3] = np.nan
    y, _, nf = counted(eng, lambda: eng.net_forward(x))
    assert nf == 1
    assert np.isfinite(y[1]).all() and np.array_equal(y[1], clean), "the clean batch item was touched"
