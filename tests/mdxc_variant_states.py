"""Seeded weights of the MDXC norm / act variant nets (tests/golden/make_golden_mdxc_variants.py, tests/test_gpu_mdxc_variants.py):
oracle.mdxc_oracle.make_v3_state for the convs / linears and the norm affines, and for BatchNorm non-trivial running statistics
(mean in [-0.3, 0.3], var in [0.5, 2]).  Regenerated where needed instead of being stored with the goldens."""
import torch

from oracle import mdxc_oracle as M

BASE = dict(n_fft=128, hop_length=16, dim_f=64, dim_t=16, num_subbands=2, num_scales=2, num_blocks_per_scale=2,
            num_channels_model=8, growth=8, bottleneck_factor=4)
# tag -> (norm, act, seed); channel counts 8 / 16 / 24 and decoder inputs 32 / 16: divisible by 2 and 4
VARIANTS = {"bn_gelu": ("BatchNorm", "gelu", 11), "gn2_relu": ("GroupNorm2", "relu", 12), "gn4_elu": ("GroupNorm4", "elu1.0", 13),
            "in_elu": ("InstanceNorm", "elu0.5", 14), "id_gelu": ("LayerNorm", "gelu", 15)}


def cfg_of(tag):
    norm, act, _ = VARIANTS[tag]
    return M.V3Config(norm=norm, act=act, **BASE)


def state_of(tag):
    """The state_dict the reference's TFC_TDF_net for this variant loads with strict=True (float32 tensors)."""
    norm, _, seed = VARIANTS[tag]
    sd = M.make_v3_state(cfg_of(tag), seed)
    norm_w = sorted(k[:-len(".weight")] for k, v in sd.items() if v.dim() == 1 and k.endswith(".weight"))   # norm affines: the only 1-D tensors
    if norm not in ("BatchNorm", "InstanceNorm") and "GroupNorm" not in norm:        # get_norm: Identity, no parameters
        return {k: v for k, v in sd.items() if v.dim() != 1}
    if norm == "BatchNorm":
        gen = torch.Generator().manual_seed(1000 + seed)
        for p in norm_w:
            c = sd[p + ".weight"].numel()
            sd[p + ".running_mean"] = 0.3 * (2 * torch.rand(c, generator=gen) - 1)
            sd[p + ".running_var"] = 0.5 + 1.5 * torch.rand(c, generator=gen)
            sd[p + ".num_batches_tracked"] = torch.tensor(100, dtype=torch.long)
    return sd
