"""GPU parity of the MDXC (TFC-TDF v3) norm / act variants: BatchNorm (eval), GroupNorm<g>, elu<alpha> and an unrecognised
norm string (Identity), against goldens written by the reference's own TFC_TDF_net / MDXCSeparator
(tests/golden/make_golden_mdxc_variants.py), plus the GroupNorm statistics pass at a size where it splits every group over
many workgroups, checked against a float64 restatement of the net.  Bar: 1e-4 relative RMS (TOL of test_gpu_mdxc.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from oracle import mdxc_oracle as M
from oracle.mdx_oracle import stft_forward, stft_inverse
from tests import separate_cases as SC
from tests.mdxc_variant_states import BASE, VARIANTS, cfg_of, state_of

pytestmark = pytest.mark.gpu
TOL = 1e-4


def rel_rms(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "mdxc_variants.npz"))


def demixer(A, cfg, sd, overlap, max_batch=0):
    arch = {"overlap": overlap, "batch_size": 2, "pitch_shift": 0}
    return A.MDXCDemixer({"model_data": cfg.as_model_data(), "torch_device": 0, "secondary_stem_name": "Instrumental"}, arch,
                         state_dict=sd, max_batch=max_batch)


# ---- float64 restatement of TFC_TDF_net.forward (tfc_tdf_v3.py:55-80, 110-267) for every norm / act kind --------------
def _norm_act64(x, sd, prefix, cfg):
    t = lambda k: torch.as_tensor(np.asarray(sd[prefix + k]), dtype=torch.float64)  # noqa: E731
    n = cfg.norm
    if n == "InstanceNorm":
        x = F.instance_norm(x, weight=t(".weight"), bias=t(".bias"), eps=1e-5)
    elif n == "BatchNorm":
        x = F.batch_norm(x, t(".running_mean"), t(".running_var"), t(".weight"), t(".bias"), training=False, eps=1e-5)
    elif n and "GroupNorm" in n:
        x = F.group_norm(x, int(n.replace("GroupNorm", "")), t(".weight"), t(".bias"), 1e-5)
    return _act64(x, cfg)


def _act64(x, cfg):
    if cfg.act == "gelu":
        return F.gelu(x)
    if cfg.act == "relu":
        return F.relu(x)
    return F.elu(x, float(cfg.act.replace("elu", "")))


def forward64(wave, sd, cfg):
    w = lambda k: torch.as_tensor(np.asarray(sd[k]), dtype=torch.float64)  # noqa: E731

    def tfc_tdf(x, prefix):
        for j in range(cfg.num_blocks_per_scale):
            p = f"{prefix}.blocks.{j}"
            s = F.conv2d(x, w(p + ".shortcut.weight"))
            x = F.conv2d(_norm_act64(x, sd, p + ".tfc1.0", cfg), w(p + ".tfc1.2.weight"), padding=1)
            h = F.linear(_norm_act64(x, sd, p + ".tdf.0", cfg), w(p + ".tdf.2.weight"))
            x = x + F.linear(_norm_act64(h, sd, p + ".tdf.3", cfg), w(p + ".tdf.5.weight"))
            x = F.conv2d(_norm_act64(x, sd, p + ".tfc2.0", cfg), w(p + ".tfc2.2.weight"), padding=1) + s
        return x

    spec = torch.as_tensor(stft_forward(np.asarray(wave, np.float32), cfg.n_fft, cfg.hop_length, cfg.dim_f), dtype=torch.float64)
    k = cfg.num_subbands
    b, c, f, t = spec.shape
    mix = spec.reshape(b, c, k, f // k, t).reshape(b, c * k, f // k, t)
    first = x = F.conv2d(mix, w("first_conv.weight"))
    x = x.transpose(-1, -2)
    enc = []
    for i in range(cfg.num_scales):
        x = tfc_tdf(x, f"encoder_blocks.{i}.tfc_tdf")
        enc.append(x)
        x = F.conv2d(_norm_act64(x, sd, f"encoder_blocks.{i}.downscale.conv.0", cfg), w(f"encoder_blocks.{i}.downscale.conv.2.weight"),
                     stride=2)
    x = tfc_tdf(x, "bottleneck_block")
    for i in range(cfg.num_scales):
        x = F.conv_transpose2d(_norm_act64(x, sd, f"decoder_blocks.{i}.upscale.conv.0", cfg),
                               w(f"decoder_blocks.{i}.upscale.conv.2.weight"), stride=2)
        x = tfc_tdf(torch.cat([x, enc.pop()], 1), f"decoder_blocks.{i}.tfc_tdf")
    x = x.transpose(-1, -2) * first
    x = F.conv2d(torch.cat([mix, x], 1), w("final_conv.0.weight"))
    x = F.conv2d(_act64(x, cfg), w("final_conv.2.weight"))
    b, c, f, t = x.shape
    y = x.reshape(b, c // k, k, f, t).reshape(b * cfg.num_targets, c // k // cfg.num_targets, f * k, t).numpy()
    return stft_inverse(y.astype(np.float32), cfg.n_fft, cfg.hop_length).reshape(b, cfg.num_targets, 2, -1)


# ---- tests --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(VARIANTS))
def test_forward_golden(A, g, tag):
    w = (0.4 * np.random.default_rng(61).standard_normal((2, 2, 240))).astype(np.float32)
    y = demixer(A, cfg_of(tag), state_of(tag), 4).engine.v3_forward(w)
    assert y.shape == g[f"{tag}__fwd"].shape
    assert rel_rms(y, g[f"{tag}__fwd"]) < TOL, rel_rms(y, g[f"{tag}__fwd"])


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_demix_golden(A, g, tag):
    cfg = cfg_of(tag)
    mix = (0.4 * np.random.default_rng(3070).standard_normal((2, 1000))).astype(np.float32)
    out = demixer(A, cfg, state_of(tag), 4, max_batch=3).demix(mix)
    got = np.stack([out[k] for k in cfg.instruments])
    assert rel_rms(got, g[f"{tag}__demix"]) < TOL, rel_rms(got, g[f"{tag}__demix"])


# dim_t 256 x dim_f 1024 over 2 subbands: level 0 is 8 channels x 131072 pixels, so GroupNorm2 sums 524288 floats per group
# and the split rule (csrc/v3_norm.h: v3_gn_splits, pinned by tests/test_host_mdxc_variants.py) gives 32 slices per group
BIG = M.V3Config(n_fft=2048, hop_length=512, dim_f=1024, dim_t=256, num_subbands=2, num_scales=2, num_blocks_per_scale=1,
                 num_channels_model=8, growth=8, bottleneck_factor=4, norm="GroupNorm2", act="relu")


def test_groupnorm_split_reduction_float64(A):
    sd = {k: v.numpy() for k, v in M.make_v3_state(BIG, 21).items()}
    d = demixer(A, BIG, sd, 2)
    chunk = BIG.hop_length * (BIG.dim_t - 1)
    w = (0.4 * np.random.default_rng(22).standard_normal((1, 2, chunk))).astype(np.float32)
    y = d.engine.v3_forward(w)
    ref = forward64(w, sd, BIG)
    assert rel_rms(y, ref) < TOL, rel_rms(y, ref)
    y2 = d.engine.v3_forward(w)
    assert np.array_equal(y.view(np.uint32), y2.view(np.uint32)), "two runs of the GroupNorm net differ"


def test_groups_must_divide_channels(A):
    cfg = M.V3Config(**dict(BASE, num_channels_model=6, growth=6), norm="GroupNorm4", act="gelu")   # 6 channels, 4 groups
    sd = {k: v.numpy() for k, v in M.make_v3_state(cfg, 3).items()}
    with pytest.raises(A.engine.AsxError, match="GroupNorm4 needs the channel count to be divisible"):
        demixer(A, cfg, sd, 2)


def test_mdxc_separator_groupnorm_elu_yaml(A, g, tmp_path, monkeypatch):
    cfg = cfg_of("gn4_elu")
    path = str(tmp_path / "mdxc_gn4_elu.ckpt")
    torch.save(state_of("gn4_elu"), path)
    with open(tmp_path / "mdxc_gn4_elu.yaml", "w") as f:
        yaml.safe_dump(cfg.as_model_data(), f)
    md = SC.load_yaml(str(tmp_path / "mdxc_gn4_elu.yaml"))
    arch = dict(SC.MDXC_ARCH, overlap=2)
    case = ("sep_gn4_elu", "MDXCSeparator", SC.common_config("mdxc_gn4_elu", path, md, str(tmp_path / "out")), arch,
            os.path.join(SC.AUDIO, "mdxc_in.wav"), None)
    inst, worst = SC.run_case(case, g, monkeypatch)
    assert type(inst.engine).__name__ == "Engine" and worst < TOL
