"""ctypes binding of libasx.so (C ABI: include/asx.h).

This is the only bridge between host Python and the HIP engine.  There is no CPU
fallback: if the shared library is missing or no GPU is visible, construction
raises.  PyTorch is not needed here; device pointers are plain integers (e.g.
``tensor.data_ptr()``).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

ASX_FLAG_MATCH_MIX = 1
PROF_CLASSES = ["stft", "conv3x3", "tdf", "down", "up", "conv1x1", "istft", "ola", "finalize", "misc"]


class AsxError(RuntimeError):
    pass


def lib_path() -> str:
    return os.path.join(_HERE, "libasx.so")


class _MdxCfg(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop_length", C.c_int32), ("dim_f", C.c_int32), ("segment_size", C.c_int32),
                ("overlap", C.c_double), ("enable_denoise", C.c_int32), ("max_batch", C.c_int32), ("win_length", C.c_int32),
                ("reserved", C.c_int32)]


class _NetCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim_c", "dim_f", "dim_t", "g", "l", "num_blocks", "k", "bn", "tdf_bias", "norm")]


class _V3Cfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_channels", "num_subbands", "num_scales", "num_blocks_per_scale",
                                         "num_channels_model", "growth", "bottleneck_factor", "norm", "act",
                                         "num_targets")]


class _RofCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "depth", "heads", "dim_head", "num_stems", "time_depth", "freq_depth",
                                         "mlp_expansion_factor", "mask_estimator_depth", "n_bands", "n_out")] + \
               [("freqs_per_bands", C.c_int32 * 128), ("mel", C.c_int32), ("band_start", C.c_int32 * 128), ("stft_normalized", C.c_int32)]


class _HtCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_sources", "channels", "growth", "nfft", "depth", "kernel_size", "stride",
                                         "dconv_depth", "dconv_comp", "bottom_channels", "t_layers", "t_heads",
                                         "t_hidden", "samplerate", "segment_samples")] + \
               [("freq_emb_scale", C.c_float), ("max_batch", C.c_int32)]


class _HdCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_sources", "channels", "growth", "nfft", "depth", "kernel_size", "stride", "time_stride",
                                         "norm_starts", "norm_groups", "dconv_depth", "dconv_comp", "dconv_attn", "dconv_lstm",
                                         "samplerate", "segment_samples")] + \
               [("freq_emb_scale", C.c_float), ("max_batch", C.c_int32)]


VR_RES_TYPES = {"polyphase": 0, "sinc_fastest": 1}      # ASX_VR_RES_*


class _VrBand(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("sr", "hl", "n_fft", "crop_start", "crop_stop", "hpf_start", "hpf_stop", "lpf_start",
                                         "lpf_stop", "convert", "res_type")]


class _VrCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bins", "n_bands", "pre_filter_start", "pre_filter_stop", "channel_mode", "arch")] + \
               [("cap", C.c_int32 * 6), ("window_size", C.c_int32), ("offset", C.c_int32), ("max_batch", C.c_int32),
                ("v51", C.c_int32), ("synth_res_type", C.c_int32), ("band", _VrBand * 8)]


class _VrParams(C.Structure):
    _fields_ = [("aggr_value", C.c_float), ("split_bin", C.c_int32), ("is_non_accom", C.c_int32), ("has_corr", C.c_int32),
                ("corr_left", C.c_float), ("corr_right", C.c_float), ("enable_tta", C.c_int32),
                ("enable_post_process", C.c_int32), ("post_thres", C.c_float), ("high_end_process", C.c_int32)]


class _Plan(C.Structure):
    _fields_ = [("n_samples", C.c_int64), ("padded_len", C.c_int64), ("chunk_size", C.c_int64),
                ("gen_size", C.c_int64), ("pad", C.c_int64), ("step", C.c_int64), ("trim", C.c_int32),
                ("n_chunks", C.c_int32), ("n_frames", C.c_int32), ("reserved", C.c_int32)]


class _Profile(C.Structure):
    _fields_ = [("launches", C.c_int64 * 10), ("ms", C.c_double * 10), ("flops", C.c_double * 10),
                ("bytes", C.c_double * 10)]


@dataclass
class MDXConfig:
    """Scalars of MDXSeparator that shape the path (mdx_separator.py:31-72)."""
    n_fft: int = 6144
    hop_length: int = 1024
    dim_f: int = 3072
    segment_size: int = 256
    overlap: float = 0.25
    enable_denoise: bool = False
    max_batch: int = 0
    win_length: int = 0       # torch.stft win_length (Roformer stft_win_length); 0 = n_fft


@dataclass
class NetConfig:
    """ConvTDFNet hyper-parameters (uvr_lib_v5/mdxnet.py:31-44)."""
    dim_c: int = 4
    dim_f: int = 3072
    dim_t: int = 256
    g: int = 48
    l: int = 3
    num_blocks: int = 11
    k: int = 3
    bn: int = 8              # 0 = one Linear(f, f) TDF (modules.py:55-60); -1 = `bn is None`, no TDF branch
    tdf_bias: bool = False
    norm: str = "batch"      # "batch" (optimizer 'rmsprop', BatchNorm folded by weights.fold_convtdf_state) | "group" (GroupNorm(2, c), 'adamw')


@dataclass
class V3Config:
    """TFC_TDF_net hyper-parameters (uvr_lib_v5/tfc_tdf_v3.py:151-214; the model YAML's
    audio/model/training sections).  n_fft / hop_length / dim_f / dim_t live in MDXConfig."""
    num_channels: int = 2
    num_subbands: int = 4
    num_scales: int = 5
    num_blocks_per_scale: int = 2
    num_channels_model: int = 128
    growth: int = 128
    bottleneck_factor: int = 4
    norm: str | None = "InstanceNorm"
    act: str = "gelu"
    num_targets: int = 2


# asx_v3_config.norm / act codes (include/asx.h)
V3_NORM_NONE, V3_NORM_INSTANCE, V3_NORM_BATCH, V3_NORM_GROUP = 0, 1, 2, 256
V3_ACT_RELU, V3_ACT_GELU, V3_ACT_ELU = 0, 1, 2
V3_ACT_ALPHA_TENSOR = "__act_alpha__"


def v3_norm_act_codes(norm, act) -> tuple:
    """model.norm / model.act of an MDX23C YAML -> (norm code, act code, elu alpha), with the rules of the reference's
    get_norm / get_act (uvr_lib_v5/tfc_tdf_v3.py:55-80): norm None / BatchNorm / InstanceNorm / any string containing
    "GroupNorm" (the rest must be an int, ValueError otherwise); any other norm is Identity.  act gelu / relu / elu<float>;
    anything else raises ValueError."""
    if norm is None:
        n = V3_NORM_NONE
    elif norm == "BatchNorm":
        n = V3_NORM_BATCH
    elif norm == "InstanceNorm":
        n = V3_NORM_INSTANCE
    elif "GroupNorm" in norm:
        g = int(norm.replace("GroupNorm", ""))
        if g < 1:
            raise ValueError(f"GroupNorm needs at least one group, got {norm!r}")
        n = V3_NORM_GROUP + g
    else:
        n = V3_NORM_NONE                                  # nn.Identity
    alpha = 1.0
    if act == "gelu":
        a = V3_ACT_GELU
    elif act == "relu":
        a = V3_ACT_RELU
    elif isinstance(act, str) and act[:3] == "elu":
        alpha = float(act.replace("elu", ""))
        a = V3_ACT_ELU
    else:
        raise ValueError(f"unsupported act {act!r} (gelu, relu or elu<alpha>)")
    return n, a, alpha


@dataclass
class RofConfig:
    """BSRoformer constructor arguments (roformer_loader.py:123-150); n_fft / hop / dim_t live in MDXConfig."""
    dim: int = 512
    depth: int = 12
    heads: int = 8
    dim_head: int = 64
    num_stems: int = 1
    time_transformer_depth: int = 1
    freq_transformer_depth: int = 1
    mlp_expansion_factor: int = 4
    mask_estimator_depth: int = 2
    freqs_per_bands: tuple = ()
    n_out: int = 2
    mel: bool = False           # MelBandRoformer: band j covers bins [band_starts[j], + freqs_per_bands[j])
    band_starts: tuple = ()
    stft_normalized: bool = False   # torch.stft / istft normalized=True (bs_roformer.py:332, 384)


@dataclass
class HTConfig:
    """HTDemucs constructor arguments (uvr_lib_v5/demucs/htdemucs.py:32-110) the engine builds."""
    sources: tuple = ("drums", "bass", "other", "vocals")
    channels: int = 48
    growth: int = 2
    nfft: int = 4096
    depth: int = 4
    kernel_size: int = 8
    stride: int = 4
    dconv_depth: int = 2
    dconv_comp: int = 8
    freq_emb: float = 0.2
    bottom_channels: int = 0
    t_layers: int = 5
    t_heads: int = 8
    t_hidden_scale: float = 4.0
    samplerate: int = 44100
    segment: object = 7.8          # seconds (Fraction in the checkpoints)
    max_batch: int = 0

    @property
    def segment_samples(self) -> int:
        return int(self.segment * self.samplerate)

    @property
    def transformer_dim(self) -> int:
        return self.bottom_channels or self.channels * self.growth ** (self.depth - 1)


@dataclass
class HDConfig:
    """HDemucs constructor arguments (uvr_lib_v5/demucs/hdemucs.py:362-420) the engine builds (Demucs v3: `hdemucs_mmi`)."""
    sources: tuple = ("drums", "bass", "other", "vocals")
    channels: int = 48
    growth: int = 2
    nfft: int = 4096
    depth: int = 6
    kernel_size: int = 8
    stride: int = 4
    time_stride: int = 2
    norm_starts: int = 4
    norm_groups: int = 4
    dconv_depth: int = 2
    dconv_comp: int = 4
    dconv_attn: int = 4
    dconv_lstm: int = 4
    freq_emb: float = 0.2
    samplerate: int = 44100
    segment: object = 40           # seconds
    max_batch: int = 0

    @property
    def segment_samples(self) -> int:
        return int(self.samplerate * self.segment)


_FP = C.POINTER(C.c_float)
_lib = None

ABI_VERSION = 8   # ASX_ABI_VERSION of include/asx.h the structures below mirror

# every symbol include/asx.h declares
SYMBOLS = ["asx_abi_version", "asx_last_error", "asx_device_count", "asx_engine_create", "asx_engine_destroy",
           "asx_net_begin", "asx_net_set_tensor", "asx_net_commit", "asx_net_flops", "asx_plan_query", "asx_demix",
           "asx_demix_dev", "asx_demix_chunks_dev", "asx_finalize_dev", "asx_separate", "asx_separate_dev",
           "asx_stft", "asx_istft", "asx_net_forward", "asx_run_model", "asx_op_conv", "asx_op_tdf",
           "asx_profile_enable", "asx_profile_read", "asx_v3_begin", "asx_v3_commit", "asx_v3_flops",
           "asx_v3_forward", "asx_mdxc_plan", "asx_mdxc_demix", "asx_mdxc_demix_dev", "asx_set_option",
           "asx_rof_begin", "asx_rof_commit", "asx_rof_flops", "asx_rof_forward", "asx_rof_demix",
           "asx_rof_demix_dev", "asx_ht_begin", "asx_ht_commit", "asx_ht_flops", "asx_ht_forward", "asx_ht_demix",
           "asx_ht_demix_dev", "asx_vr_begin", "asx_vr_commit", "asx_vr_flops", "asx_vr_plan", "asx_vr_forward",
           "asx_vr_analysis", "asx_vr_separate", "asx_vr_separate_dev", "asx_debug_fetch", "asx_mdxc_chunks_dev",
           "asx_mdxc_finalize_dev", "asx_rof_plan", "asx_rof_chunks_dev", "asx_rof_finalize_dev", "asx_ht_plan",
           "asx_ht_segments_dev", "asx_ht_fold_dev", "asx_hd_begin", "asx_hd_commit", "asx_hd_flops",
           "asx_hd_forward", "asx_hd_demix", "asx_hd_demix_dev", "asx_ht_demix_batch_dev", "asx_hd_demix_batch_dev", "asx_hd_plan", "asx_hd_segments_dev",
           "asx_hd_fold_dev", "asx_pcm16", "asx_pcm16_dev", "asx_pcm16_rows_dev", "asx_pcm_decode_dev",
           "asx_ht_standardize_dev", "asx_ht_bag_accumulate_dev", "asx_ht_bag_finish_dev", "asx_ensemble",
           "asx_ensemble_dev", "asx_invert_stem", "asx_normalize", "asx_normalize_dev", "asx_residual_dev",
           "asx_profile_launches", "asx_debug_trace", "asx_resample_sinc", "asx_resample_sinc_dev", "asx_counter",
           "asx_set_stft_window", "asx_op_tdf_block", "asx_op_attention", "asx_op_mha", "asx_get_option",
           "asx_demix_batch_dev", "asx_separate_batch_dev", "asx_ensemble_slot_dev", "asx_vr_separate_batch_dev",
           "asx_mdxc_demix_batch_dev", "asx_rof_demix_batch_dev", "asx_ensemble_batch_dev", "asx_resample_rational_plan",
           "asx_resample_rational", "asx_resample_rational_dev", "asx_op_hd_lstm_layer", "asx_op_hd_lstm_frames", "asx_op_vr_lstm",
           "asx_op_vr_lstm_layout", "asx_flac_plan", "asx_flac_encode", "asx_flac_encode_dev",
           "asx_flac_decode_plan", "asx_flac_decode_scan_dev", "asx_flac_decode_finish_dev", "asx_flac_decode",
           "asx_flac_plan_pcm", "asx_flac_encode_pcm", "asx_flac_encode_pcm_dev", "asx_pcm_encode", "asx_pcm_encode_dev",
           "asx_invert_stem_dev", "asx_invert_stem_batch_dev", "asx_op_gconv", "asx_op_dconv", "asx_resample_sinc_batch_dev",
           "asx_resample_rational_stem", "asx_resample_rational_stem_dev", "asx_op_stft", "asx_op_istft", "asx_op_ht_spec",
           "asx_op_ht_ispec", "asx_ensemble_batch_modes_dev", "asx_resample_rational_complement",
           "asx_resample_rational_complement_dev", "asx_normalize_scale_dev", "asx_mixdown_batch_dev", "asx_mixdown",
           "asx_phase_fix_batch_dev", "asx_phase_fix_dev", "asx_phase_fix", "asx_op_rownorm", "asx_op_group_stats",
           "asx_op_group_norm"]

# the attention variants of asx_op_attention / asx_op_mha, in the order of their `resolved` index (include/asx.h)
ATTN_VARIANTS = ("auto", "attn2", "attn2_qw2", "attn2_db", "attn6", "attn6_qw2", "attn6h", "attn6h_qw2", "mha", "mha_db", "mha6",
                 "mha6_wide", "mha6h", "mha6h_wide", "hd_local", "attn6s", "attn6s_qw2")


GCONV_VARIANTS = ("auto", "gg", "halo", "gather")   # asx_op_gconv: `variant`, and resolved[0] as an index (0: nothing ran)
GCONV_MODES = {"dense": 0, "glu": 1, "convt": 2}


class _GconvDesc(C.Structure):     # struct asx_gconv_desc
    _fields_ = [(n, C.c_int32) for n in ("B", "O", "I", "Cin", "ldc", "Cout", "ldy", "KO", "KI", "DO", "DI", "PO", "PI", "SO", "SI", "OR",
                                         "IR", "x_col0", "y_col0", "mode", "act", "res", "ldr", "res_mod", "Iout", "crop", "So",
                                         "no_halo")] + [("x_bs", C.c_int64), ("y_bs", C.c_int64)]


# asx_op_stft / asx_op_istft: resolved[0] as an index (0: nothing ran)
STFT_KERNELS = (None, "stft", "stft_pool", "stft3", "stft3_pool", "stft3p", "stft3p_pool", "istft+ola", "istft3", "istft3p")
STFT_MODES = {"chunks": 0, "song": 1, "pool": 2}


class _StftDesc(C.Structure):      # struct asx_stft_desc
    _fields_ = [(n, C.c_int32) for n in ("b", "t", "layout", "subbands", "zero_low", "n_inst", "combine", "stft_normalized", "mode", "front",
                                         "n_songs")] + [("sign", C.c_float), ("c", C.c_int64), ("bstride", C.c_int64),
                                                        ("spec_floats", C.c_int64), ("starts", C.POINTER(C.c_int64)),
                                                        ("song_of", C.POINTER(C.c_int32)), ("song_len", C.POINTER(C.c_int64)),
                                                        ("n_act", C.POINTER(C.c_int64))]


# asx_op_rownorm: `kind`; asx_op_group_norm: `family`, the hd modes, and the norm / act codes of asx_v3_config for "v3"
ROWNORM_KINDS = ("rms", "rms_factor", "layer")
GROUP_NORM_FAMILIES = ("ht", "hd", "std", "time", "hd_time", "v3", "mdx")
HD_GN_MODES = {"gelu": 0, "glu": 1, "none": 2}
V3_ACTS = {"relu": 0, "gelu": 1, "elu": 2}


def v3_norm_code(norm):
    """asx_v3_config.norm of the model's norm name: None, InstanceNorm, BatchNorm or GroupNorm<g>"""
    if norm is None or norm == "None":
        return 0
    if norm in ("InstanceNorm", "BatchNorm"):
        return 1 if norm == "InstanceNorm" else 2
    if isinstance(norm, str) and norm.startswith("GroupNorm") and norm[9:].isdigit() and int(norm[9:]) > 0:
        return 256 + int(norm[9:])
    raise AsxError(f"unknown norm {norm!r}")


class _GroupNormDesc(C.Structure):  # struct asx_group_norm_desc
    _fields_ = [(n, C.c_int32) for n in ("b", "c", "g", "mode", "norm", "act", "ctot", "c0", "in_place")] + [("alpha", C.c_float)] + \
               [(n, C.c_int64) for n in ("r", "rin", "r0", "p")]


class _LaunchRec(C.Structure):     # struct asx_launch_rec
    _fields_ = [("cls", C.c_int32), ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double)]


class _Song(C.Structure):          # struct asx_song
    _fields_ = [("mix_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_samples", C.c_int64)]


class _ApplySong(C.Structure):     # struct asx_apply_song
    _fields_ = [("mix_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_samples", C.c_int64), ("offsets", C.POINTER(C.c_int64))]


class _VrSong(C.Structure):        # struct asx_vr_song
    _fields_ = [("wave_dev", C.c_void_p), ("n_samples", C.c_int64), ("primary_dev", C.c_void_p), ("secondary_dev", C.c_void_p)]


class _MdxcSong(C.Structure):      # struct asx_mdxc_song
    _fields_ = [("mix_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_samples", C.c_int64)]


ENS_MAX_K = 8                      # ASX_ENS_MAX_K: contributors of one ensemble job


class _EnsJob(C.Structure):        # struct asx_ens_job
    _fields_ = [("k", C.c_int32), ("live", C.c_int32), ("stem_dev", C.c_void_p * ENS_MAX_K), ("n_samples", C.c_int64 * ENS_MAX_K),
                ("layout", C.c_int32 * ENS_MAX_K), ("out_dev", C.c_void_p), ("out_capacity", C.c_int64), ("n_out", C.c_int64),
                ("peak_after", C.c_float * ENS_MAX_K)]


MIX_MAX_K = 8                      # ASX_MIX_MAX_K: sources of one mix-down job


class _MixSrc(C.Structure):        # struct asx_mix_src
    _fields_ = [("x", C.c_void_p), ("layout", C.c_int32), ("n", C.c_int64), ("w", C.c_float)]


class _MixJob(C.Structure):        # struct asx_mix_job
    _fields_ = [("src", _MixSrc * MIX_MAX_K), ("k", C.c_int32), ("out", C.c_void_p), ("out_layout", C.c_int32), ("n_out", C.c_int64)]


PHASE_BINS = 1025                  # ASX_PHASE_BINS: bins of the phase fix's STFT (n_fft 2048), one weight each
PHASE_HOPS = (256, 512, 1024)


class _PhaseJob(C.Structure):      # struct asx_phase_job
    _fields_ = [("target_dev", C.c_void_p), ("source_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_samples", C.c_int64),
                ("source_n_samples", C.c_int64), ("target_layout", C.c_int32), ("source_layout", C.c_int32), ("out_layout", C.c_int32),
                ("reserved", C.c_int32)]


class _InvertSong(C.Structure):    # struct asx_invert_song
    _fields_ = [("mix_dev", C.c_void_p), ("stem_dev", C.c_void_p), ("out_dev", C.c_void_p), ("n_samples", C.c_int64),
                ("out_capacity", C.c_int64), ("n_out", C.c_int64), ("stem_layout", C.c_int32)]


class _SincJob(C.Structure):       # struct asx_sinc_job
    _fields_ = [("x_dev", C.c_void_p), ("y_dev", C.c_void_p), ("n_in", C.c_int64), ("n_out", C.c_int64), ("channels", C.c_int32),
                ("reserved", C.c_int32)]


VR_POOL_SEGMENTS = 16             # ASX_VR_POOL_SEGMENTS: songs one gather / scatter launch of a pooled VR pass serves


class _SongStems(C.Structure):     # struct asx_song_stems
    _fields_ = [("mix_dev", C.c_void_p), ("primary_dev", C.c_void_p), ("secondary_dev", C.c_void_p), ("n_samples", C.c_int64)]


def load_library():
    """dlopen libasx.so and declare the signatures.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    try:
        # torch-ROCm bundles its own libamdhip64 (same soname).  Importing it first makes the
        # dynamic loader resolve libasx.so against that one runtime, so device pointers taken
        # from torch tensors and the engine's own allocations live in the same HIP context.
        import torch  # noqa: F401
    except Exception:  # torch is plumbing, not a requirement of the engine
        pass
    if not os.path.exists(path):
        raise AsxError(f"{path} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                       "There is no CPU fallback for the demix path.")
    lib = C.CDLL(path)
    vp, i32, i64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32
    lib.asx_abi_version.restype = C.c_int
    if lib.asx_abi_version() != ABI_VERSION:
        raise AsxError(f"{path} speaks ABI {lib.asx_abi_version()}, this binding ABI {ABI_VERSION}: rebuild (python __graft_entry__.py)")
    lib.asx_last_error.restype = C.c_char_p
    lib.asx_device_count.restype = C.c_int
    lib.asx_engine_create.argtypes = [C.c_int, C.POINTER(_MdxCfg), C.POINTER(vp)]
    lib.asx_engine_destroy.argtypes = [vp]
    lib.asx_engine_destroy.restype = None
    lib.asx_net_begin.argtypes = [vp, C.POINTER(_NetCfg)]
    lib.asx_net_set_tensor.argtypes = [vp, C.c_char_p, _FP, i64]
    lib.asx_net_commit.argtypes = [vp]
    lib.asx_net_flops.argtypes = [vp, i32]
    lib.asx_net_flops.restype = C.c_double
    lib.asx_plan_query.argtypes = [vp, i64, u32, C.POINTER(_Plan)]
    lib.asx_demix.argtypes = [vp, _FP, i64, _FP, u32]
    lib.asx_demix_dev.argtypes = [vp, vp, i64, vp, u32, vp]
    lib.asx_demix_chunks_dev.argtypes = [vp, vp, i64, i32, i32, vp, u32, vp]
    lib.asx_finalize_dev.argtypes = [vp, vp, i64, vp, u32, vp]
    f32 = C.c_float
    lib.asx_separate.argtypes = [vp, _FP, i64, f32, f32, i32, f32, _FP, _FP]
    lib.asx_separate_dev.argtypes = [vp, vp, i64, f32, f32, i32, f32, vp, vp, vp]
    lib.asx_demix_batch_dev.argtypes = [vp, C.POINTER(_Song), i32, u32, vp]
    lib.asx_separate_batch_dev.argtypes = [vp, C.POINTER(_SongStems), i32, f32, f32, i32, f32, vp]
    lib.asx_stft.argtypes = [vp, _FP, i32, i64, _FP]
    lib.asx_istft.argtypes = [vp, _FP, i32, i32, _FP]
    lib.asx_net_forward.argtypes = [vp, _FP, i32, _FP]
    lib.asx_run_model.argtypes = [vp, _FP, i32, _FP, u32]
    lib.asx_op_conv.argtypes = [vp, C.c_char_p, _FP, i32, i32, i32, i32, _FP, _FP, i32, _FP, i32, _FP]
    lib.asx_op_tdf.argtypes = [vp, _FP, i32, i32, i32, i32, _FP, _FP, i32, _FP, _FP, _FP, _FP]
    lib.asx_op_tdf_block.argtypes = [vp, _FP, i32, i32, i32, i32, _FP, _FP, _FP, i32, _FP, _FP, _FP, _FP, _FP]
    lib.asx_op_attention.argtypes = [vp, _FP, _FP, i64, i32, i32, i32, i32, i32, i32, i32, C.c_char_p, _FP, C.POINTER(i32)]
    lib.asx_op_mha.argtypes = [vp, _FP, i64, _FP, i64, _FP, i64, _FP, i64, i32, i32, i32, i32, i32, i32, C.c_char_p, _FP, i64,
                               C.POINTER(i32)]
    lib.asx_op_hd_lstm_layer.argtypes = [vp, _FP, _FP, i32, i32, i32, _FP, _FP]
    lib.asx_op_hd_lstm_frames.argtypes = [vp, i32, _FP, i32, i32, i32, i32, i32, _FP, C.POINTER(i32), C.POINTER(i32)]
    lib.asx_op_vr_lstm.argtypes = [vp, _FP, _FP, i32, i32, i32, _FP]
    lib.asx_op_vr_lstm_layout.argtypes = [vp, i32, _FP, i32, i32, i32, i32, i32, _FP]
    lib.asx_op_gconv.argtypes = [vp, C.POINTER(_GconvDesc), _FP, _FP, _FP, _FP, C.c_char_p, _FP, C.POINTER(i32)]
    lib.asx_op_stft.argtypes = [vp, C.POINTER(_StftDesc), _FP, _FP, C.POINTER(i32)]
    lib.asx_op_istft.argtypes = [vp, C.POINTER(_StftDesc), _FP, _FP, _FP, C.POINTER(i32)]
    _DP = C.POINTER(C.c_double)
    lib.asx_op_ht_spec.argtypes = [vp, i32, _FP, i32, i64, i64, i64, _FP]
    lib.asx_op_ht_ispec.argtypes = [vp, i32, _FP, i32, i32, i32, _DP, C.c_double, _FP, _DP, i64, _FP]
    lib.asx_op_dconv.argtypes = [vp, _FP, i32, i32, i32, i32, i32, i32, i32, i32, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP,
                                 C.POINTER(i32)]
    lib.asx_op_rownorm.argtypes = [vp, C.c_char_p, _FP, i64, i32, i64, _FP, _FP, _FP, i64, i32, _FP, i64]
    lib.asx_op_group_stats.argtypes = [vp, _FP, i32, i64, i64, i64, i32, i32, i32, _DP]
    lib.asx_op_group_norm.argtypes = [vp, C.c_char_p, C.POINTER(_GroupNormDesc), _FP, _FP, _FP, _FP, _FP, _FP, _FP]
    lib.asx_v3_begin.argtypes = [vp, C.POINTER(_V3Cfg)]
    lib.asx_v3_commit.argtypes = [vp]
    lib.asx_v3_flops.argtypes = [vp, i32]
    lib.asx_v3_flops.restype = C.c_double
    lib.asx_v3_forward.argtypes = [vp, _FP, i32, _FP]
    lib.asx_mdxc_plan.argtypes = [vp, i64, i32, C.POINTER(_Plan)]
    lib.asx_mdxc_demix.argtypes = [vp, _FP, i64, i32, _FP]
    lib.asx_mdxc_demix_dev.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.asx_rof_begin.argtypes = [vp, C.POINTER(_RofCfg)]
    lib.asx_rof_commit.argtypes = [vp]
    lib.asx_rof_flops.argtypes = [vp, i32]
    lib.asx_rof_flops.restype = C.c_double
    lib.asx_rof_forward.argtypes = [vp, _FP, i32, _FP]
    lib.asx_rof_demix.argtypes = [vp, _FP, i64, i64, _FP]
    lib.asx_rof_demix_dev.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.asx_mdxc_demix_batch_dev.argtypes = [vp, C.POINTER(_MdxcSong), i32, i32, vp]
    lib.asx_rof_demix_batch_dev.argtypes = [vp, C.POINTER(_MdxcSong), i32, i64, vp]
    lib.asx_set_option.argtypes = [vp, C.c_char_p, i32]
    lib.asx_get_option.argtypes = [vp, C.c_char_p, C.POINTER(i32)]
    lib.asx_counter.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.asx_set_stft_window.argtypes = [vp, _FP, i32]
    lib.asx_ht_begin.argtypes = [vp, C.POINTER(_HtCfg)]
    lib.asx_ht_commit.argtypes = [vp]
    lib.asx_ht_flops.argtypes = [vp]
    lib.asx_ht_flops.restype = C.c_double
    lib.asx_ht_forward.argtypes = [vp, _FP, i32, i64, _FP]
    lib.asx_ht_demix.argtypes = [vp, _FP, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, _FP]
    lib.asx_ht_demix_dev.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, vp, vp]
    lib.asx_vr_begin.argtypes = [vp, C.POINTER(_VrCfg)]
    lib.asx_vr_commit.argtypes = [vp]
    lib.asx_vr_flops.argtypes = [vp]
    lib.asx_vr_flops.restype = C.c_double
    lib.asx_vr_plan.argtypes = [vp, i64, C.POINTER(i32), C.POINTER(i64)]
    lib.asx_vr_forward.argtypes = [vp, _FP, i32, _FP]
    lib.asx_vr_analysis.argtypes = [vp, _FP, i64, _FP]
    lib.asx_vr_separate.argtypes = [vp, _FP, i64, C.POINTER(_VrParams), _FP, _FP]
    lib.asx_vr_separate_dev.argtypes = [vp, vp, i64, C.POINTER(_VrParams), vp, vp, vp]
    lib.asx_vr_separate_batch_dev.argtypes = [vp, C.POINTER(_VrSong), i32, C.POINTER(_VrParams), vp]
    lib.asx_debug_fetch.argtypes = [vp, C.c_char_p, _FP, i64]
    lib.asx_resample_sinc.argtypes = [vp, _FP, i32, i64, C.c_double, i32, _FP, i64]
    lib.asx_resample_sinc_dev.argtypes = [vp, vp, i32, i64, C.c_double, i32, vp, i64, vp]
    lib.asx_resample_sinc_batch_dev.argtypes = [vp, C.POINTER(_SincJob), i32, C.c_double, i32, vp]
    lib.asx_resample_rational_plan.argtypes = [i32, i32, i64, C.POINTER(i64), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.asx_resample_rational.argtypes = [vp, _FP, i32, i64, i32, i32, _FP, i64]
    lib.asx_resample_rational_dev.argtypes = [vp, vp, i32, i64, i32, i32, vp, i64, vp]
    lib.asx_resample_rational_stem.argtypes = [vp, _FP, i32, i32, i64, i32, i32, _FP, i64]
    lib.asx_resample_rational_stem_dev.argtypes = [vp, vp, i32, i32, i64, i32, i32, vp, i64, vp]
    lib.asx_resample_rational_complement.argtypes = [vp, _FP, i32, i32, i64, i32, i32, _FP, i64, C.c_float, C.c_float, _FP, _FP, i64]
    lib.asx_resample_rational_complement_dev.argtypes = [vp, vp, i32, i32, i64, i32, i32, vp, i64, C.c_float, C.c_float, vp, vp, i64, vp]
    lib.asx_normalize_scale_dev.argtypes = [vp, vp, i64, C.c_float, C.c_float, i32, C.POINTER(C.c_float), vp]
    lib.asx_mixdown_batch_dev.argtypes = [vp, C.POINTER(_MixJob), i32, vp]
    lib.asx_mixdown.argtypes = [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(i64), C.POINTER(C.c_float), i32, _FP, i32, i64]
    lib.asx_phase_fix_batch_dev.argtypes = [vp, C.POINTER(_PhaseJob), i32, _FP, i32, vp]
    lib.asx_phase_fix_dev.argtypes = [vp, C.POINTER(_PhaseJob), _FP, i32, vp]
    lib.asx_phase_fix.argtypes = [vp, _FP, i32, i64, _FP, i32, i64, _FP, i32, _FP, i32]
    lib.asx_flac_plan.argtypes = [i64, i32, i32, i32, C.POINTER(i64), C.POINTER(i32), C.POINTER(i64), C.POINTER(i64)]
    lib.asx_flac_encode.argtypes = [vp, C.POINTER(C.c_int16), i64, i32, i32, i32, C.POINTER(C.c_uint8), i64, C.POINTER(i32), C.POINTER(i64)]
    lib.asx_flac_encode_dev.argtypes = [vp, vp, i64, i32, i32, i32, vp, i64, vp, C.POINTER(i64), vp]
    lib.asx_flac_plan_pcm.argtypes = lib.asx_flac_plan.argtypes
    lib.asx_flac_encode_pcm.argtypes = [vp, C.POINTER(i32), i64, i32, i32, i32, C.POINTER(C.c_uint8), i64, C.POINTER(i32), C.POINTER(i64)]
    lib.asx_flac_encode_pcm_dev.argtypes = lib.asx_flac_encode_dev.argtypes
    lib.asx_pcm_encode.argtypes = [vp, _FP, i64, i32, C.c_float, C.c_float, i32, i32, vp, _FP]
    lib.asx_pcm_encode_dev.argtypes = [vp, vp, i64, i32, C.c_float, C.c_float, i32, i32, vp, _FP, vp]
    lib.asx_flac_decode_plan.argtypes = [i64, i32, i32, i32, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    lib.asx_flac_decode_scan_dev.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64), vp]
    lib.asx_flac_decode_finish_dev.argtypes = [vp, vp, i64, _FP, vp]
    lib.asx_flac_decode.argtypes = [vp, C.POINTER(C.c_uint8), i64, i32, i32, i32, i32, i32, _FP, i64, C.POINTER(i64), C.POINTER(i64),
                                    C.POINTER(i64), _FP]
    lib.asx_ensemble.argtypes = [vp, _FP, i32, i64, i32, C.POINTER(C.c_double), _FP, C.POINTER(i64)]
    lib.asx_ensemble_dev.argtypes = [vp, vp, i32, i64, i32, C.POINTER(C.c_double), vp, C.POINTER(i64), vp]
    lib.asx_invert_stem.argtypes = [vp, _FP, _FP, i64, _FP, C.POINTER(i64)]
    lib.asx_invert_stem_dev.argtypes = [vp, vp, vp, i64, i32, C.c_float, vp, i64, C.POINTER(i64), vp]
    lib.asx_invert_stem_batch_dev.argtypes = [vp, C.POINTER(_InvertSong), i32, C.c_float, vp]
    lib.asx_ensemble_batch_dev.argtypes = [vp, C.POINTER(_EnsJob), i32, i32, C.POINTER(C.c_double), i32, i32, C.c_float, C.c_float, i32,
                                           C.c_double, vp]
    lib.asx_ensemble_batch_modes_dev.argtypes = [vp, C.POINTER(_EnsJob), i32, C.POINTER(i32), i32, C.POINTER(C.c_double), i32, C.c_float, C.c_float,
                                                 i32, C.c_double, vp]
    lib.asx_ensemble_slot_dev.argtypes = [vp, vp, i64, i32, C.c_float, C.c_float, i32, i32, vp, i32, i64, _FP, vp]
    lib.asx_pcm16.argtypes = [vp, _FP, i64, C.c_float, C.c_float, i32, C.POINTER(C.c_int16), _FP]
    lib.asx_normalize.argtypes = [vp, _FP, i64, C.c_float, C.c_float, i32, _FP]
    lib.asx_pcm16_dev.argtypes = [vp, vp, i64, C.c_float, C.c_float, i32, vp, _FP, vp]
    lib.asx_pcm16_rows_dev.argtypes = [vp, vp, i64, C.c_float, C.c_float, i32, vp, _FP, vp]
    lib.asx_pcm_decode_dev.argtypes = [vp, vp, i64, i32, i32, vp, _FP, vp]
    lib.asx_profile_launches.argtypes = [vp, C.POINTER(_LaunchRec), i32, C.POINTER(i32)]
    lib.asx_normalize_dev.argtypes = [vp, vp, i64, C.c_float, C.c_float, i32, vp]
    lib.asx_residual_dev.argtypes = [vp, vp, vp, vp, i64, vp]
    lib.asx_ht_standardize_dev.argtypes = [vp, vp, i64, vp, vp]
    lib.asx_ht_bag_accumulate_dev.argtypes = [vp, vp, vp, _FP, i32, i64, i32, vp]
    lib.asx_ht_bag_finish_dev.argtypes = [vp, vp, _FP, i32, vp, i64, C.c_uint32, vp, vp]
    lib.asx_mdxc_chunks_dev.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp]
    lib.asx_mdxc_finalize_dev.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.asx_rof_plan.argtypes = [vp, i64, i64, C.POINTER(i32), C.POINTER(i64)]
    lib.asx_rof_chunks_dev.argtypes = [vp, vp, i64, i64, i32, i32, vp, vp]
    lib.asx_rof_finalize_dev.argtypes = [vp, vp, i64, i64, vp, vp]
    lib.asx_ht_plan.argtypes = [vp, i64, i32, C.POINTER(C.c_int64), C.c_double, C.POINTER(i32), C.POINTER(i64)]
    lib.asx_ht_segments_dev.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, i32, i32, vp, vp]
    lib.asx_ht_fold_dev.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, vp, vp, vp]
    lib.asx_hd_begin.argtypes = [vp, C.POINTER(_HdCfg)]
    lib.asx_hd_commit.argtypes = [vp]
    lib.asx_hd_flops.argtypes = [vp, i64]
    lib.asx_hd_flops.restype = C.c_double
    lib.asx_hd_forward.argtypes = [vp, _FP, i32, i64, _FP]
    lib.asx_hd_demix.argtypes = [vp, _FP, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, _FP]
    lib.asx_hd_demix_dev.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, vp, vp]
    lib.asx_hd_plan.argtypes = [vp, i64, i32, C.POINTER(C.c_int64), C.c_double, C.POINTER(i32), C.POINTER(i64)]
    lib.asx_hd_segments_dev.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, i32, i32, vp, vp]
    lib.asx_hd_fold_dev.argtypes = [vp, vp, i64, i32, C.POINTER(C.c_int64), C.c_double, u32, vp, vp, vp]
    lib.asx_ht_demix_batch_dev.argtypes = [vp, C.POINTER(_ApplySong), i32, i32, C.c_double, u32, vp]
    lib.asx_hd_demix_batch_dev.argtypes = [vp, C.POINTER(_ApplySong), i32, i32, C.c_double, u32, vp]
    lib.asx_profile_enable.argtypes = [vp, i32]
    lib.asx_profile_read.argtypes = [vp, C.POINTER(_Profile)]
    for name in SYMBOLS:
        getattr(lib, name)  # AttributeError if the library does not export what the header declares
    _lib = lib
    return lib


def ht_pos_tables(hc: "HTConfig") -> dict:
    """The two sinusoidal tables of CrossTransformerEncoder (transformer.py:18-46, 522-537) in torch float32 on the
    host, in the engine's token order: "pos_emb_freq" rows (t1, fr), "pos_emb_time" rows t2."""
    import math

    import torch
    Ct = hc.transformer_dim
    hop = hc.nfft // 4
    T1 = -(-hc.segment_samples // hop)
    Fr = hc.nfft // 2 // hc.stride ** hc.depth
    T2 = hc.segment_samples
    for _ in range(hc.depth):
        T2 = -(-T2 // hc.stride)
    pe = torch.zeros(Ct, Fr, T1)
    dm = Ct // 2
    div = torch.exp(torch.arange(0.0, dm, 2) * -(math.log(10000.0) / dm))
    pw = torch.arange(0.0, T1).unsqueeze(1)
    ph = torch.arange(0.0, Fr).unsqueeze(1)
    pe[0:dm:2] = torch.sin(pw * div).transpose(0, 1).unsqueeze(1).repeat(1, Fr, 1)
    pe[1:dm:2] = torch.cos(pw * div).transpose(0, 1).unsqueeze(1).repeat(1, Fr, 1)
    pe[dm::2] = torch.sin(ph * div).transpose(0, 1).unsqueeze(2).repeat(1, 1, T1)
    pe[dm + 1::2] = torch.cos(ph * div).transpose(0, 1).unsqueeze(2).repeat(1, 1, T1)
    half = Ct // 2
    pos = torch.arange(T2).view(-1, 1)
    adim = torch.arange(half).view(1, -1)
    phase = pos / (10000.0 ** (adim / (half - 1)))
    pt = torch.cat([torch.cos(phase), torch.sin(phase)], dim=-1)
    return {"pos_emb_freq": pe.permute(2, 1, 0).reshape(T1 * Fr, Ct).contiguous().numpy(),
            "pos_emb_time": pt.contiguous().numpy()}


def _f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_FP)


def _optptr(a):
    return _ptr(a) if a is not None else None


class Engine:
    """One HIP engine bound to one GPU (asx_engine)."""

    def __init__(self, cfg: MDXConfig, device: int = 0):
        self._lib = load_library()
        self._h = C.c_void_p()
        self.cfg = cfg
        self.device = device
        self.net_cfg = None
        if self._lib.asx_device_count() <= 0:
            raise AsxError("no HIP device visible: the demix path runs on MI355X only (no CPU fallback)")
        c = _MdxCfg(cfg.n_fft, cfg.hop_length, cfg.dim_f, cfg.segment_size, float(cfg.overlap),
                    int(bool(cfg.enable_denoise)), int(cfg.max_batch), int(getattr(cfg, "win_length", 0) or 0), 0)
        self._check(self._lib.asx_engine_create(device, C.byref(c), C.byref(self._h)))

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            msg = self._lib.asx_last_error()
            raise AsxError(f"asx error {rc}: {msg.decode() if msg else '?'}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.asx_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key: str, value: int):
        self._check(self._lib.asx_set_option(self._h, key.encode(), int(value)))

    def option(self, key: str) -> int:
        """Current value of an engine option, as the library holds it (asx_get_option)."""
        out = C.c_int32(0)
        self._check(self._lib.asx_get_option(self._h, key.encode(), C.byref(out)))
        return int(out.value)

    def counter(self, name: str) -> int:
        """A library launch counter (asx_counter): "tdf3_launches" = bf16x6 row-GEMM launches of this process, ..."""
        out = C.c_int64(0)
        self._check(self._lib.asx_counter(self._h, name.encode(), C.byref(out)))
        return int(out.value)

    # -- weights ------------------------------------------------------------
    def _set_tensors(self, tensors: dict):
        """name -> float32 array / torch tensor, handed to the net that the last asx_*_begin opened"""
        for name, t in tensors.items():
            if hasattr(t, "detach"):
                t = t.detach().cpu().numpy()
            a = _f32(t).reshape(-1)
            self._check(self._lib.asx_net_set_tensor(self._h, name.encode(), _ptr(a), a.size))

    def load_net(self, net_cfg: NetConfig, tensors: dict):
        """tensors: canonical name -> float32 array (see include/asx.h)."""
        if net_cfg.norm not in ("batch", "group"):
            raise ValueError(f"NetConfig.norm must be 'batch' or 'group', got {net_cfg.norm!r}")
        n = _NetCfg(net_cfg.dim_c, net_cfg.dim_f, net_cfg.dim_t, net_cfg.g, net_cfg.l, net_cfg.num_blocks, net_cfg.k,
                    -1 if net_cfg.bn is None else net_cfg.bn, int(bool(net_cfg.tdf_bias)), 1 if net_cfg.norm == "group" else 0)
        self._check(self._lib.asx_net_begin(self._h, C.byref(n)))
        self._set_tensors(tensors)
        self._check(self._lib.asx_net_commit(self._h))
        self.net_cfg = net_cfg

    def net_flops(self, batch: int = 1) -> float:
        return float(self._lib.asx_net_flops(self._h, batch))

    # -- MDXC / TFC-TDF v3 ------------------------------------------------------
    def load_v3(self, v3: V3Config, state_dict: dict):
        """state_dict: the reference TFC_TDF_net's own keys -> float32 arrays / torch tensors (BatchNorm running statistics
        included).  norm / act as the YAML names them (v3_norm_act_codes)."""
        norm, act, alpha = v3_norm_act_codes(v3.norm, v3.act)
        c = _V3Cfg(v3.num_channels, v3.num_subbands, v3.num_scales, v3.num_blocks_per_scale, v3.num_channels_model,
                   v3.growth, v3.bottleneck_factor, norm, act, v3.num_targets)
        self._check(self._lib.asx_v3_begin(self._h, C.byref(c)))
        self._set_tensors(state_dict)
        if act == V3_ACT_ELU:
            self._set_tensors({V3_ACT_ALPHA_TENSOR: np.array([alpha], np.float32)})
        self._check(self._lib.asx_v3_commit(self._h))
        self.v3_cfg = v3

    def v3_flops(self, batch: int = 1) -> float:
        return float(self._lib.asx_v3_flops(self._h, batch))

    def v3_forward(self, wave: np.ndarray) -> np.ndarray:
        wave = _f32(wave)
        B, ch, Cn = wave.shape
        out = np.empty((B, self.v3_cfg.num_targets, 2, Cn), np.float32)
        self._check(self._lib.asx_v3_forward(self._h, _ptr(wave), B, _ptr(out)))
        return out

    def mdxc_plan(self, n_samples: int, overlap: int) -> dict:
        p = _Plan()
        self._check(self._lib.asx_mdxc_plan(self._h, n_samples, overlap, C.byref(p)))
        return {k: getattr(p, k) for k, _ in _Plan._fields_ if k != "reserved"}

    def mdxc_demix(self, mix: np.ndarray, overlap: int) -> np.ndarray:
        mix = _f32(mix)
        if mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
        out = np.empty((self.v3_cfg.num_targets, 2, mix.shape[1]), np.float32)
        self._check(self._lib.asx_mdxc_demix(self._h, _ptr(mix), mix.shape[1], int(overlap), _ptr(out)))
        return out

    def mdxc_demix_dev(self, mix_ptr: int, n_samples: int, overlap: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.asx_mdxc_demix_dev(self._h, mix_ptr, n_samples, int(overlap), out_ptr, stream or None))

    # a batch of songs in one call: the chunks of all of them pooled per net pass (both MDXC loops)
    def _mdxc_batch_dev(self, fn, songs, arg, stream):
        songs = list(songs)
        arr = (_MdxcSong * max(1, len(songs)))()
        for i, (mix_ptr, out_ptr, n) in enumerate(songs):
            arr[i] = _MdxcSong(mix_ptr or None, out_ptr or None, int(n))
        self._check(fn(self._h, arr, len(songs), int(arg), stream or None))

    def _mdxc_batch(self, dev_call, rows, mixes, arg) -> list:
        """A list of float32 [2, N_i] arrays through one pooled call; returns the list of [rows, 2, N_i] results.  Device staging
        buffers come from torch (the plumbing layer), as in ``demix_batch``."""
        host = []
        for mix in mixes:
            mix = _f32(mix)
            if mix.ndim != 2 or mix.shape[0] != 2:
                raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
            host.append(mix)
        if not host:
            return []
        torch, dev, st = self._torch_stream()
        with torch.cuda.stream(st):
            d_mix = [torch.from_numpy(m).to(dev) for m in host]
            d_out = [torch.empty((rows, 2, m.shape[1]), dtype=torch.float32, device=dev) for m in host]
            dev_call([(m.data_ptr() if m.numel() else 0, o.data_ptr() if o.numel() else 0, m.shape[1]) for m, o in zip(d_mix, d_out)],
                     arg, st.cuda_stream)
            outs = [o.cpu().numpy() for o in d_out]
        return outs

    def mdxc_demix_batch_dev(self, songs, overlap: int, stream: int = 0):
        """``songs``: a list of ``(mix_ptr, out_ptr, n_samples)`` -- mix [2, n] and out [S, 2, n] in HBM.  The chunks of all songs
        share the net passes; every ``out`` equals what ``mdxc_demix_dev`` writes for that song alone, bit for bit
        (asx_mdxc_demix_batch_dev)."""
        self._mdxc_batch_dev(self._lib.asx_mdxc_demix_batch_dev, songs, overlap, stream)

    def mdxc_demix_batch(self, mixes, overlap: int) -> list:
        return self._mdxc_batch(self.mdxc_demix_batch_dev, self.v3_cfg.num_targets if mixes else 0, mixes, overlap)

    def rof_demix_batch_dev(self, songs, step: int, stream: int = 0):
        """As ``mdxc_demix_batch_dev`` on the Roformer loop: out [n_out, 2, n] each, equal to ``rof_demix_dev``'s
        (asx_rof_demix_batch_dev).  A song shorter than one chunk is refused, by index, before anything runs."""
        self._mdxc_batch_dev(self._lib.asx_rof_demix_batch_dev, songs, step, stream)

    def rof_demix_batch(self, mixes, step: int) -> list:
        return self._mdxc_batch(self.rof_demix_batch_dev, self.rof_cfg.n_out if mixes else 0, mixes, step)

    # -- BS-Roformer ------------------------------------------------------------
    def load_rof(self, rc: RofConfig, state_dict: dict):
        if len(rc.freqs_per_bands) > 128:
            raise ValueError("at most 128 bands")
        c = _RofCfg(rc.dim, rc.depth, rc.heads, rc.dim_head, rc.num_stems, rc.time_transformer_depth,
                    rc.freq_transformer_depth, rc.mlp_expansion_factor, rc.mask_estimator_depth,
                    len(rc.freqs_per_bands), rc.n_out)
        for i, f in enumerate(rc.freqs_per_bands):
            c.freqs_per_bands[i] = int(f)
        c.mel = int(bool(rc.mel))
        c.stft_normalized = int(bool(rc.stft_normalized))
        if rc.mel:
            if len(rc.band_starts) != len(rc.freqs_per_bands):
                raise ValueError("mel: one band start per band")
            for i, f in enumerate(rc.band_starts):
                c.band_start[i] = int(f)
        self._check(self._lib.asx_rof_begin(self._h, C.byref(c)))
        self._set_tensors(state_dict)
        self._check(self._lib.asx_rof_commit(self._h))
        self.rof_cfg = rc

    def set_stft_window(self, window: np.ndarray):
        """Replace the periodic Hann of torch.stft / istft by `window` [n_fft] (already zero padded from win_length like torch pads it)."""
        w = _f32(window).reshape(-1)
        self._check(self._lib.asx_set_stft_window(self._h, _ptr(w), int(w.size)))

    def rof_flops(self, batch: int = 1) -> float:
        return float(self._lib.asx_rof_flops(self._h, batch))

    def rof_forward(self, wave: np.ndarray) -> np.ndarray:
        wave = _f32(wave)
        B, ch, Cn = wave.shape
        out = np.empty((B, self.rof_cfg.num_stems, 2, Cn), np.float32)
        self._check(self._lib.asx_rof_forward(self._h, _ptr(wave), B, _ptr(out)))
        return out

    def rof_demix(self, mix: np.ndarray, step: int) -> np.ndarray:
        mix = _f32(mix)
        if mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
        out = np.empty((self.rof_cfg.n_out, 2, mix.shape[1]), np.float32)
        self._check(self._lib.asx_rof_demix(self._h, _ptr(mix), mix.shape[1], int(step), _ptr(out)))
        return out

    def rof_demix_dev(self, mix_ptr: int, n_samples: int, step: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.asx_rof_demix_dev(self._h, mix_ptr, n_samples, int(step), out_ptr, stream or None))

    # -- Demucs v4 ----------------------------------------------------------------
    def load_ht(self, hc: HTConfig, state_dict: dict, pos_tables: bool = True):
        """HTDemucs(**kwargs) + load_state_dict.  pos_tables: compute the sinusoidal tables with torch on the host
        (bit-identical to transformer.py:18-46 on CPU) and hand them over; otherwise the engine builds them itself."""
        C_t = hc.transformer_dim
        c = _HtCfg(len(hc.sources), hc.channels, hc.growth, hc.nfft, hc.depth, hc.kernel_size, hc.stride, hc.dconv_depth,
                   hc.dconv_comp, hc.bottom_channels, hc.t_layers, hc.t_heads, int(C_t * hc.t_hidden_scale),
                   hc.samplerate, hc.segment_samples, float(hc.freq_emb), hc.max_batch)
        self._check(self._lib.asx_ht_begin(self._h, C.byref(c)))
        tensors = dict(state_dict)
        if pos_tables and hc.t_layers > 0:
            tensors.update(ht_pos_tables(hc))
        self._set_tensors(tensors)
        self._check(self._lib.asx_ht_commit(self._h))
        self.ht_cfg = hc

    def ht_flops(self) -> float:
        return float(self._lib.asx_ht_flops(self._h))

    def ht_forward(self, mix: np.ndarray) -> np.ndarray:
        mix = _f32(mix)
        B, ch, L = mix.shape
        if ch != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got {ch} channels")
        out = np.empty((B, len(self.ht_cfg.sources), 2, L), np.float32)
        self._check(self._lib.asx_ht_forward(self._h, _ptr(mix), B, L, _ptr(out)))
        return out

    def ht_demix(self, mix: np.ndarray, shifts: int = 0, offsets=None, overlap: float = 0.25, standardize: bool = False,
                 swap01: bool = False) -> np.ndarray:
        return self._apply_demix("ht", len(self.ht_cfg.sources), mix, shifts, offsets, overlap, standardize, swap01)

    def ht_demix_dev(self, mix_ptr: int, n_samples: int, out_ptr: int, shifts: int = 0, offsets=None,
                     overlap: float = 0.25, flags: int = 0, stream: int = 0):
        self._apply_demix_dev("ht", mix_ptr, n_samples, out_ptr, shifts, offsets, overlap, flags, stream)

    # -- BagOfModels combine on the device -----------------------------------------
    def ht_standardize_dev(self, mix_ptr: int, n_samples: int, out_ptr: int, stream: int = 0):
        self._check(self._lib.asx_ht_standardize_dev(self._h, mix_ptr, n_samples, out_ptr, stream or None))

    def ht_bag_accumulate_dev(self, est_ptr: int, member_ptr: int, weights, n_samples: int, first: bool, stream: int = 0):
        w = (C.c_float * len(weights))(*[float(v) for v in weights])
        self._check(self._lib.asx_ht_bag_accumulate_dev(self._h, est_ptr, member_ptr, w, len(weights), n_samples, int(bool(first)),
                                                        stream or None))

    def ht_bag_finish_dev(self, est_ptr: int, totals, mix_ptr: int, n_samples: int, out_ptr: int, standardize: bool = True,
                          swap01: bool = True, stream: int = 0):
        t = (C.c_float * len(totals))(*[float(v) for v in totals])
        flags = (1 if standardize else 0) | (2 if swap01 else 0)
        self._check(self._lib.asx_ht_bag_finish_dev(self._h, est_ptr, t, len(totals), mix_ptr, n_samples, flags, out_ptr, stream or None))

    # -- Demucs v3 ----------------------------------------------------------------
    def load_hd(self, hc: HDConfig, state_dict: dict):
        """HDemucs(**kwargs) + load_state_dict (uvr_lib_v5/demucs/hdemucs.py:362-571)."""
        c = _HdCfg(len(hc.sources), hc.channels, hc.growth, hc.nfft, hc.depth, hc.kernel_size, hc.stride, hc.time_stride,
                   hc.norm_starts, hc.norm_groups, hc.dconv_depth, hc.dconv_comp, hc.dconv_attn, hc.dconv_lstm, hc.samplerate,
                   hc.segment_samples, float(hc.freq_emb), hc.max_batch)
        self._check(self._lib.asx_hd_begin(self._h, C.byref(c)))
        self._set_tensors(state_dict)
        self._check(self._lib.asx_hd_commit(self._h))
        self.hd_cfg = hc

    def hd_flops(self, length: int) -> float:
        return float(self._lib.asx_hd_flops(self._h, int(length)))

    def hd_forward(self, mix: np.ndarray) -> np.ndarray:
        """HDemucs.forward: [B, 2, L] -> [B, S, 2, L], any L >= nfft."""
        mix = _f32(mix)
        B, ch, L = mix.shape
        if ch != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got {ch} channels")
        out = np.empty((B, len(self.hd_cfg.sources), 2, L), np.float32)
        self._check(self._lib.asx_hd_forward(self._h, _ptr(mix), B, L, _ptr(out)))
        return out

    def hd_demix(self, mix: np.ndarray, shifts: int = 0, offsets=None, overlap: float = 0.25, standardize: bool = False,
                 swap01: bool = False) -> np.ndarray:
        return self._apply_demix("hd", len(self.hd_cfg.sources), mix, shifts, offsets, overlap, standardize, swap01)

    def hd_demix_dev(self, mix_ptr: int, n_samples: int, out_ptr: int, shifts: int = 0, offsets=None, overlap: float = 0.25,
                     flags: int = 0, stream: int = 0):
        self._apply_demix_dev("hd", mix_ptr, n_samples, out_ptr, shifts, offsets, overlap, flags, stream)

    # -- VR -----------------------------------------------------------------------
    def load_vr(self, model_params: dict, arch: int, capacity, state_dict: dict, window_size: int = 512, offset: int = 128,
                max_batch: int = 0, v51=None, wav_resolution: str = "polyphase"):
        """nets.determine_model_capacity(bins * 2, arch) + load_state_dict.  model_params: the modelparams JSON dict
        (int band keys); capacity: the model_capacity_data table of nets.py:74-86.  v51 = (nout, nout_lstm) selects
        nets_new.CascadedNet and the is_v51_model branches instead (capacity is then ignored).  ``wav_resolution``: the
        synthesis chain's converter (spec_utils.py:33-38), "sinc_fastest" or "polyphase"; the analysis converters follow each
        band's own "res_type" ("sinc_fastest" -> the sinc converter, anything else -> polyphase)."""
        mp = model_params
        mode = 3 if mp.get("reverse") else (1 if mp.get("mid_side") else (2 if mp.get("mid_side_b2") else 0))
        nb = len(mp["band"])
        c = _VrCfg(mp["bins"], nb, mp["pre_filter_start"], mp["pre_filter_stop"], 0 if v51 else mode, int(arch))
        caps = (v51[0], v51[1], 0, 0, 0, 0) if v51 else (capacity[0][1], capacity[2][1], capacity[3][1], capacity[4][1], capacity[5][1], 0)
        for i, v in enumerate(caps):
            c.cap[i] = int(v)
        c.window_size, c.offset, c.max_batch, c.v51 = int(window_size), int(offset), int(max_batch), int(bool(v51))
        if wav_resolution not in VR_RES_TYPES:
            raise ValueError(f"wav_resolution {wav_resolution!r}: expected one of {sorted(VR_RES_TYPES)}")
        c.synth_res_type = VR_RES_TYPES[wav_resolution]
        conv = {None: 0, "mid_side": 1, "mid_side_c": 4, "stereo_n": 5}
        for d in range(1, nb + 1):
            bp = mp["band"][d]
            cc = bp.get("convert_channels") if v51 else None
            if cc not in conv:
                raise NotImplementedError(f"convert_channels {cc!r}")
            c.band[d - 1] = _VrBand(bp["sr"], bp["hl"], bp["n_fft"], bp["crop_start"], bp["crop_stop"], bp.get("hpf_start", 0),
                                    bp.get("hpf_stop", 0), bp.get("lpf_start", 0), bp.get("lpf_stop", 0), conv[cc],
                                    VR_RES_TYPES.get(bp.get("res_type", "polyphase"), 0))
        self._check(self._lib.asx_vr_begin(self._h, C.byref(c)))
        self._set_tensors(state_dict)
        self._check(self._lib.asx_vr_commit(self._h))
        self.vr_bins = mp["bins"]
        self.vr_window = int(window_size)

    def resample_sinc(self, x: np.ndarray, ratio: float, mono_calls: bool = False) -> np.ndarray:
        """librosa.resample(x, orig_sr, target_sr, res_type="sinc_fastest") with ratio = float(target_sr) / orig_sr on x [C, n]
        (or [n]) -> [C, ceil(n * ratio)].  ``mono_calls``: channel by channel, as spec_utils.change_pitch_semitones calls it."""
        x = _f32(x)
        one = x.ndim == 1
        x2 = np.ascontiguousarray(x[None] if one else x)
        if x2.ndim != 2 or x2.shape[1] < 1:
            raise ValueError(f"resample_sinc expects [channels, n], got {x.shape}")
        n_out = int(np.ceil(x2.shape[1] * float(ratio)))
        y = np.empty((x2.shape[0], n_out), np.float32)
        self._check(self._lib.asx_resample_sinc(self._h, _ptr(x2), x2.shape[0], x2.shape[1], float(ratio), int(bool(mono_calls) or one),
                                                _ptr(y), n_out))
        return y[0] if one else y

    def resample_sinc_dev(self, x_ptr: int, channels: int, n_in: int, ratio: float, mono_calls: bool, y_ptr: int, n_out: int, stream: int = 0):
        self._check(self._lib.asx_resample_sinc_dev(self._h, x_ptr, int(channels), int(n_in), float(ratio), int(bool(mono_calls)), y_ptr,
                                                    int(n_out), stream or None))

    def resample_sinc_batch_dev(self, jobs, ratio: float, mono_calls: bool, stream: int = 0):
        """asx_resample_sinc_batch_dev: ``resample_sinc_dev`` for a list of ``(x_ptr, y_ptr, n_in, n_out, channels)`` at one ratio in
        ONE launch of the converter; every output equals the single call's bit for bit, ``n_out`` is free per job (frames beyond the
        generated count are zero).  Only enqueues work on ``stream`` (an engine's first sinc call also builds the coefficient table and allocates
        the job table, once); a bad job raises AsxError naming it before anything runs."""
        arr = (_SincJob * max(1, len(jobs)))()
        for i, (x_ptr, y_ptr, n_in, n_out, channels) in enumerate(jobs):
            arr[i] = _SincJob(x_ptr or None, y_ptr or None, int(n_in), int(n_out), int(channels), 0)
        self._check(self._lib.asx_resample_sinc_batch_dev(self._h, arr, len(jobs), float(ratio), int(bool(mono_calls)), stream or None))

    @staticmethod
    def resample_rational_plan(sr_in: int, sr_out: int, n_in: int = 1):
        """asx_resample_rational_plan (pure host: no engine, no GPU): (n_out, L, M, taps per output) of the rational polyphase
        converter for ``n_in`` samples at ``sr_in`` Hz -> ``sr_out`` Hz.  Raises AsxError for a pair the converter refuses (equal
        rates, a coefficient table beyond 2^20 floats)."""
        lib = load_library()
        n_out, up, down, taps = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32()
        rc = lib.asx_resample_rational_plan(int(sr_in), int(sr_out), int(n_in), C.byref(n_out), C.byref(up), C.byref(down), C.byref(taps))
        if rc != 0:
            msg = lib.asx_last_error()
            raise AsxError(f"asx error {rc}: {msg.decode() if msg else '?'}")
        return n_out.value, up.value, down.value, taps.value

    def resample_rational(self, x: np.ndarray, sr_in: int, sr_out: int) -> np.ndarray:
        """x [C, n] (or [n]) at ``sr_in`` Hz -> [C, ceil(n * sr_out / sr_in)] at ``sr_out`` Hz through the high-quality polyphase
        converter (asx_resample_rational: the step of loading a file at another rate than the model's)."""
        x = _f32(x)
        one = x.ndim == 1
        x2 = np.ascontiguousarray(x[None] if one else x)
        if x2.ndim != 2 or x2.shape[1] < 1:
            raise ValueError(f"resample_rational expects [channels, n], got {x.shape}")
        n_out = self.resample_rational_plan(sr_in, sr_out, x2.shape[1])[0]
        y = np.empty((x2.shape[0], n_out), np.float32)
        self._check(self._lib.asx_resample_rational(self._h, _ptr(x2), x2.shape[0], x2.shape[1], int(sr_in), int(sr_out), _ptr(y), n_out))
        return y[0] if one else y

    def resample_rational_dev(self, x_ptr: int, channels: int, n_in: int, sr_in: int, sr_out: int, y_ptr: int, n_out: int, stream: int = 0):
        self._check(self._lib.asx_resample_rational_dev(self._h, x_ptr, int(channels), int(n_in), int(sr_in), int(sr_out), y_ptr, int(n_out),
                                                        stream or None))

    RESAMPLE_LAYOUTS = {"planar": 0, "rows": 1}     # asx_resample_rational_stem: x [channels, n] | [n, channels]

    def resample_rational_stem(self, x: np.ndarray, sr_in: int, sr_out: int, n_out: int, layout: str = "planar") -> np.ndarray:
        """The writer-side form of the converter (asx_resample_rational_stem): x [C, n] ("planar"; [n] is one channel) or [n, C]
        ("rows", the MDX stem layout) at ``sr_in`` Hz -> planar [C, n_out] at ``sr_out`` Hz with the caller's ``n_out`` -- the definition
        of ``resample_rational`` carried on past, or cut before, its ceil(n * sr_out / sr_in) outputs (zeros once the filter has left
        the input)."""
        if layout not in self.RESAMPLE_LAYOUTS:
            raise ValueError(f"layout must be one of {tuple(self.RESAMPLE_LAYOUTS)}, not {layout!r}")
        x = _f32(x)
        one = x.ndim == 1 and layout == "planar"
        x2 = np.ascontiguousarray(x[None] if one else x)
        if x2.ndim != 2 or min(x2.shape) < 1:
            raise ValueError(f"resample_rational_stem expects {'[channels, n]' if layout == 'planar' else '[n, channels]'}, got {x.shape}")
        ch, n_in = x2.shape if layout == "planar" else x2.shape[::-1]
        y = np.empty((ch, max(int(n_out), 0)), np.float32)
        self._check(self._lib.asx_resample_rational_stem(self._h, _ptr(x2), self.RESAMPLE_LAYOUTS[layout], ch, n_in, int(sr_in), int(sr_out),
                                                         _ptr(y), int(n_out)))
        return y[0] if one else y

    def resample_rational_stem_dev(self, x_ptr: int, layout: str, channels: int, n_in: int, sr_in: int, sr_out: int, y_ptr: int, n_out: int,
                                   stream: int = 0):
        self._check(self._lib.asx_resample_rational_stem_dev(self._h, x_ptr, self.RESAMPLE_LAYOUTS[layout], int(channels), int(n_in), int(sr_in),
                                                             int(sr_out), y_ptr, int(n_out), stream or None))

    def resample_rational_complement(self, x: np.ndarray, sr_in: int, sr_out: int, n_out: int, mix: np.ndarray, mix_scale: float = 1.0,
                                     stem_scale: float = 1.0, layout: str = "planar", want_stem: bool = True):
        """The complement form of ``resample_rational_stem`` (asx_resample_rational_complement): with y what that call gives for ``x``,
        returns (y, c), both planar [C, n_out] -- (None, c) without ``want_stem`` -- where
        c[ch][m] = fl(fl(mix_scale * mix[ch][m]) - fl(stem_scale * y[ch][m])), one float32 rounding each.  ``mix``: planar [C, >= n_out]
        at ``sr_out`` Hz (a row stride beyond ``n_out`` is passed on as it is)."""
        if layout not in self.RESAMPLE_LAYOUTS:
            raise ValueError(f"layout must be one of {tuple(self.RESAMPLE_LAYOUTS)}, not {layout!r}")
        x = _f32(x)
        one = x.ndim == 1 and layout == "planar"
        x2 = np.ascontiguousarray(x[None] if one else x)
        if x2.ndim != 2 or min(x2.shape) < 1:
            raise ValueError(f"resample_rational_complement expects {'[channels, n]' if layout == 'planar' else '[n, channels]'}, got {x.shape}")
        ch, n_in = x2.shape if layout == "planar" else x2.shape[::-1]
        m = _f32(mix)
        m2 = np.ascontiguousarray(m[None] if m.ndim == 1 else m)
        if m2.ndim != 2 or m2.shape[0] != ch:
            raise ValueError(f"resample_rational_complement expects a mix of [{ch}, >= n_out], got {m.shape}")
        y = np.empty((ch, max(int(n_out), 0)), np.float32) if want_stem else None
        c = np.empty((ch, max(int(n_out), 0)), np.float32)
        self._check(self._lib.asx_resample_rational_complement(self._h, _ptr(x2), self.RESAMPLE_LAYOUTS[layout], ch, n_in, int(sr_in),
                                                               int(sr_out), _ptr(m2), m2.shape[1], float(mix_scale), float(stem_scale),
                                                               _ptr(y) if want_stem else None, _ptr(c), int(n_out)))
        return (y[0] if one and want_stem else y), (c[0] if one else c)

    def resample_rational_complement_dev(self, x_ptr: int, layout: str, channels: int, n_in: int, sr_in: int, sr_out: int, mix_ptr: int,
                                         mix_stride: int, mix_scale: float, stem_scale: float, y_ptr: int, c_ptr: int, n_out: int,
                                         stream: int = 0):
        """asx_resample_rational_complement_dev; ``y_ptr`` = 0: only the complement is stored."""
        self._check(self._lib.asx_resample_rational_complement_dev(self._h, x_ptr, self.RESAMPLE_LAYOUTS[layout], int(channels), int(n_in),
                                                                   int(sr_in), int(sr_out), mix_ptr, int(mix_stride), float(mix_scale),
                                                                   float(stem_scale), y_ptr or None, c_ptr, int(n_out), stream or None))

    def vr_flops(self) -> float:
        return float(self._lib.asx_vr_flops(self._h))

    def vr_plan(self, n_samples: int):
        t, n = C.c_int32(), C.c_int64()
        self._check(self._lib.asx_vr_plan(self._h, int(n_samples), C.byref(t), C.byref(n)))
        return t.value, n.value

    def vr_forward(self, x: np.ndarray) -> np.ndarray:
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 2 or x.shape[2] != self.vr_bins + 1 or x.shape[3] != self.vr_window:
            raise ValueError(f"expected [B, 2, {self.vr_bins + 1}, {self.vr_window}], got {x.shape}")
        out = np.empty_like(x)
        self._check(self._lib.asx_vr_forward(self._h, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def vr_analysis(self, wave: np.ndarray) -> np.ndarray:
        """loading_mix: [2, n] -> complex64 [2, bins+1, n_frames] (transposed back to the reference layout)."""
        wave = _f32(wave)
        T, _ = self.vr_plan(wave.shape[1])
        buf = np.empty((2, T, self.vr_bins + 1, 2), np.float32)
        self._check(self._lib.asx_vr_analysis(self._h, _ptr(wave), wave.shape[1], _ptr(buf)))
        return np.ascontiguousarray(buf.view(np.complex64)[..., 0].transpose(0, 2, 1))

    @staticmethod
    def _vr_params(aggr_value, split_bin, is_non_accom, aggr_correction, enable_tta, enable_post_process, post_thres, high_end_process):
        corr = aggr_correction or {}
        return _VrParams(float(aggr_value), int(split_bin), int(bool(is_non_accom)), int(aggr_correction is not None),
                         float(corr.get("left", 0.0)), float(corr.get("right", 0.0)), int(bool(enable_tta)),
                         int(bool(enable_post_process)), float(post_thres), int(bool(high_end_process)))

    def vr_separate(self, wave: np.ndarray, aggr_value: float, split_bin: int, is_non_accom: bool = False, aggr_correction=None,
                    enable_tta: bool = False, enable_post_process: bool = False, post_thres: float = 0.2,
                    high_end_process: bool = False):
        wave = _f32(wave)
        if wave.ndim != 2 or wave.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {wave.shape}")
        _, n_out = self.vr_plan(wave.shape[1])
        pr = self._vr_params(aggr_value, split_bin, is_non_accom, aggr_correction, enable_tta, enable_post_process, post_thres, high_end_process)
        p = np.empty((2, n_out), np.float32)
        q = np.empty((2, n_out), np.float32)
        self._check(self._lib.asx_vr_separate(self._h, _ptr(wave), wave.shape[1], C.byref(pr), _ptr(p), _ptr(q)))
        return p, q

    def vr_separate_dev(self, wave_ptr: int, n_samples: int, primary_ptr: int, secondary_ptr: int, aggr_value: float,
                        split_bin: int, is_non_accom: bool = False, enable_tta: bool = False, enable_post_process: bool = False,
                        post_thres: float = 0.2, stream: int = 0, aggr_correction=None, high_end_process: bool = False):
        pr = self._vr_params(aggr_value, split_bin, is_non_accom, aggr_correction, enable_tta, enable_post_process, post_thres, high_end_process)
        self._check(self._lib.asx_vr_separate_dev(self._h, wave_ptr, n_samples, C.byref(pr), primary_ptr or None,
                                                  secondary_ptr or None, stream or None))

    def vr_separate_batch_dev(self, songs, aggr_value: float, split_bin: int, is_non_accom: bool = False, enable_tta: bool = False,
                              enable_post_process: bool = False, post_thres: float = 0.2, stream: int = 0, aggr_correction=None,
                              high_end_process: bool = False):
        """``songs``: a list of ``(wave_ptr, n_samples, primary_ptr or 0, secondary_ptr or 0)`` -- wave [2, n] and the stems
        [2, n_out] (``vr_plan``) in HBM; a 0 output pointer leaves that stem out.  The patches of all songs share the net passes;
        every stem equals what ``vr_separate_dev`` writes for that song alone (asx_vr_separate_batch_dev)."""
        songs = list(songs)
        arr = (_VrSong * max(1, len(songs)))()
        for i, (wave_ptr, n, primary_ptr, secondary_ptr) in enumerate(songs):
            arr[i] = _VrSong(wave_ptr or None, int(n), primary_ptr or None, secondary_ptr or None)
        pr = self._vr_params(aggr_value, split_bin, is_non_accom, aggr_correction, enable_tta, enable_post_process, post_thres, high_end_process)
        self._check(self._lib.asx_vr_separate_batch_dev(self._h, arr, len(songs), C.byref(pr), stream or None))

    # -- chunk-range halves of the sibling loops (multi-GPU sharding, sharding.py) ----------------------------
    def mdxc_chunks_dev(self, mix_ptr, n, overlap, k0, k1, out_ptr, stream=0):
        self._check(self._lib.asx_mdxc_chunks_dev(self._h, mix_ptr, n, int(overlap), k0, k1, out_ptr, stream or None))

    def mdxc_finalize_dev(self, chunks_ptr, n, overlap, out_ptr, stream=0):
        self._check(self._lib.asx_mdxc_finalize_dev(self._h, chunks_ptr, n, int(overlap), out_ptr, stream or None))

    def rof_plan(self, n, step):
        k, c = C.c_int32(), C.c_int64()
        self._check(self._lib.asx_rof_plan(self._h, n, int(step), C.byref(k), C.byref(c)))
        return {"n_chunks": k.value, "chunk_size": c.value}

    def rof_chunks_dev(self, mix_ptr, n, step, k0, k1, out_ptr, stream=0):
        self._check(self._lib.asx_rof_chunks_dev(self._h, mix_ptr, n, int(step), k0, k1, out_ptr, stream or None))

    def rof_finalize_dev(self, chunks_ptr, n, step, out_ptr, stream=0):
        self._check(self._lib.asx_rof_finalize_dev(self._h, chunks_ptr, n, int(step), out_ptr, stream or None))

    # -- apply_model of Demucs v4 ("ht") and v3 ("hd"): one body per verb, the generation picks the asx_<gen>_* entry point ------
    @staticmethod
    def _offs(shifts, offsets):
        return (C.c_int64 * shifts)(*[int(o) for o in offsets]) if shifts else None

    def _apply_demix(self, gen, n_sources, mix, shifts, offsets, overlap, standardize, swap01):
        mix = _f32(mix)
        if mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
        if shifts and (offsets is None or len(offsets) != shifts):
            raise ValueError("shifts > 0 needs one offset per shift")
        out = np.empty((n_sources, 2, mix.shape[1]), np.float32)
        flags = (1 if standardize else 0) | (2 if swap01 else 0)
        self._check(getattr(self._lib, f"asx_{gen}_demix")(self._h, _ptr(mix), mix.shape[1], int(shifts), self._offs(shifts, offsets),
                                                          float(overlap), flags, _ptr(out)))
        return out

    def _apply_demix_dev(self, gen, mix_ptr, n, out_ptr, shifts, offsets, overlap, flags, stream):
        self._check(getattr(self._lib, f"asx_{gen}_demix_dev")(self._h, mix_ptr, n, int(shifts), self._offs(shifts, offsets),
                                                              float(overlap), flags, out_ptr, stream or None))

    def _apply_plan(self, gen, n, shifts, offsets, overlap):
        k, c = C.c_int32(), C.c_int64()
        self._check(getattr(self._lib, f"asx_{gen}_plan")(self._h, n, int(shifts), self._offs(shifts, offsets), float(overlap),
                                                         C.byref(k), C.byref(c)))
        return {"n_chunks": k.value, "chunk_size": c.value}

    def _apply_segments_dev(self, gen, mix_ptr, n, k0, k1, out_ptr, shifts, offsets, overlap, flags, stream):
        self._check(getattr(self._lib, f"asx_{gen}_segments_dev")(self._h, mix_ptr, n, int(shifts), self._offs(shifts, offsets),
                                                                 float(overlap), flags, k0, k1, out_ptr, stream or None))

    def _apply_fold_dev(self, gen, mix_ptr, n, chunks_ptr, out_ptr, shifts, offsets, overlap, flags, stream):
        self._check(getattr(self._lib, f"asx_{gen}_fold_dev")(self._h, mix_ptr, n, int(shifts), self._offs(shifts, offsets),
                                                             float(overlap), flags, chunks_ptr, out_ptr, stream or None))

    def _apply_demix_batch_dev(self, gen, songs, shifts, overlap, flags, stream):
        """``songs``: a list of ``(mix_ptr, out_ptr, n_samples, offsets)`` -- mix [2, n] and out [S, 2, n] in HBM, ``offsets`` the
        ``shifts`` draws of that song (None when shifts == 0).  The segments of all songs share the forwards; every ``out`` equals
        what ``<gen>_demix_dev`` writes for that song alone, bit for bit (asx_<gen>_demix_batch_dev)."""
        songs = list(songs)
        arr = (_ApplySong * max(1, len(songs)))()
        keep = []                                          # the offset arrays live until the call returns
        for i, (mix_ptr, out_ptr, n, offsets) in enumerate(songs):
            offs = None
            if shifts and offsets is not None:
                if len(offsets) != shifts:
                    raise ValueError(f"song {i}: shifts > 0 needs one offset per shift")
                offs = self._offs(shifts, offsets)
                keep.append(offs)
            arr[i] = _ApplySong(mix_ptr or None, out_ptr or None, int(n), offs)
        self._check(getattr(self._lib, f"asx_{gen}_demix_batch_dev")(self._h, arr, len(songs), int(shifts), float(overlap), flags,
                                                                    stream or None))

    def ht_demix_batch_dev(self, songs, shifts=0, overlap=0.25, flags=0, stream=0):
        self._apply_demix_batch_dev("ht", songs, shifts, overlap, flags, stream)

    def hd_demix_batch_dev(self, songs, shifts=0, overlap=0.25, flags=0, stream=0):
        self._apply_demix_batch_dev("hd", songs, shifts, overlap, flags, stream)

    def _apply_demix_batch(self, gen, n_sources, mixes, shifts, offsets, overlap, standardize, swap01):
        """``<gen>_demix`` for a list of float32 [2, N_i] arrays in one pooled call; ``offsets[i]`` are song i's draws.  Returns the
        list of [S, 2, N_i] results.  Device staging buffers come from torch (the plumbing layer), as in ``demix_batch``."""
        host = []
        for mix in mixes:
            mix = _f32(mix)
            if mix.ndim != 2 or mix.shape[0] != 2:
                raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
            host.append(mix)
        if shifts and (offsets is None or len(offsets) != len(host)):
            raise ValueError("shifts > 0 needs one list of offsets per song")
        if not host:
            return []
        torch, dev, st = self._torch_stream()
        flags = (1 if standardize else 0) | (2 if swap01 else 0)
        with torch.cuda.stream(st):
            d_mix = [torch.from_numpy(m).to(dev) for m in host]
            d_out = [torch.empty((n_sources, 2, m.shape[1]), dtype=torch.float32, device=dev) for m in host]
            self._apply_demix_batch_dev(gen, [(m.data_ptr() if m.numel() else 0, o.data_ptr() if o.numel() else 0, m.shape[1],
                                               offsets[i] if shifts else None) for i, (m, o) in enumerate(zip(d_mix, d_out))],
                                        shifts, overlap, flags, st.cuda_stream)
            outs = [o.cpu().numpy() for o in d_out]
        return outs

    def ht_demix_batch(self, mixes, shifts=0, offsets=None, overlap=0.25, standardize=False, swap01=False) -> list:
        return self._apply_demix_batch("ht", len(self.ht_cfg.sources), mixes, shifts, offsets, overlap, standardize, swap01)

    def hd_demix_batch(self, mixes, shifts=0, offsets=None, overlap=0.25, standardize=False, swap01=False) -> list:
        return self._apply_demix_batch("hd", len(self.hd_cfg.sources), mixes, shifts, offsets, overlap, standardize, swap01)

    def ht_plan(self, n, shifts=0, offsets=None, overlap=0.25):
        return self._apply_plan("ht", n, shifts, offsets, overlap)

    def ht_segments_dev(self, mix_ptr, n, k0, k1, out_ptr, shifts=0, offsets=None, overlap=0.25, flags=0, stream=0):
        self._apply_segments_dev("ht", mix_ptr, n, k0, k1, out_ptr, shifts, offsets, overlap, flags, stream)

    def ht_fold_dev(self, mix_ptr, n, chunks_ptr, out_ptr, shifts=0, offsets=None, overlap=0.25, flags=0, stream=0):
        self._apply_fold_dev("ht", mix_ptr, n, chunks_ptr, out_ptr, shifts, offsets, overlap, flags, stream)

    def hd_plan(self, n, shifts=0, offsets=None, overlap=0.25):
        return self._apply_plan("hd", n, shifts, offsets, overlap)

    def hd_segments_dev(self, mix_ptr, n, k0, k1, out_ptr, shifts=0, offsets=None, overlap=0.25, flags=0, stream=0):
        self._apply_segments_dev("hd", mix_ptr, n, k0, k1, out_ptr, shifts, offsets, overlap, flags, stream)

    def hd_fold_dev(self, mix_ptr, n, chunks_ptr, out_ptr, shifts=0, offsets=None, overlap=0.25, flags=0, stream=0):
        self._apply_fold_dev("hd", mix_ptr, n, chunks_ptr, out_ptr, shifts, offsets, overlap, flags, stream)

    def pcm16(self, stem: np.ndarray, max_peak: float = 1.0, min_peak=None):
        """write_audio_pydub's array work: stem [N, 2] (or [2, N] planar with planar=True semantics when shape[0] == 2)
        -> (int16 interleaved [N, 2], peak after normalisation)."""
        stem = np.asarray(stem, np.float32)
        planar = np.ascontiguousarray(stem.T if stem.shape[-1] == 2 and stem.shape[0] != 2 else stem)
        n = planar.shape[1]
        out = np.empty((n, 2), np.int16)
        pk = C.c_float()
        self._check(self._lib.asx_pcm16(self._h, _ptr(planar), n, float(max_peak), float(min_peak or 0.0), int(min_peak is not None),
                                        out.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(pk)))
        return out, pk.value

    FLAC_BLOCK_SIZE = 4096

    @staticmethod
    def flac_plan(n_samples: int, channels: int = 2, bits_per_sample: int = 16, block_size: int = FLAC_BLOCK_SIZE) -> dict:
        """asx_flac_plan (pure host: no engine, no GPU): {n_blocks, frame_stride, max_bytes, scratch_bytes} of the FLAC encoder for
        ``n_samples`` inter-channel samples.  Raises AsxError for what the encoder refuses (channels other than 2, bits per sample other
        than 16 / 24, a block size outside 16 .. 4608, no samples)."""
        return Engine._flac_plan("asx_flac_plan", n_samples, channels, bits_per_sample, block_size)

    @staticmethod
    def _flac_plan(symbol, n_samples, channels, bits_per_sample, block_size) -> dict:
        lib = load_library()
        nb, stride, mx, scratch = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64()
        rc = getattr(lib, symbol)(int(n_samples), int(channels), int(bits_per_sample), int(block_size), C.byref(nb), C.byref(stride), C.byref(mx),
                                  C.byref(scratch))
        if rc != 0:
            msg = lib.asx_last_error()
            raise AsxError(f"asx error {rc}: {msg.decode() if msg else '?'}")
        return {"n_blocks": nb.value, "frame_stride": stride.value, "max_bytes": mx.value, "scratch_bytes": scratch.value}

    def flac_encode(self, pcm: np.ndarray, samplerate: int, bits_per_sample: int = 16, block_size: int = FLAC_BLOCK_SIZE):
        """int16 [n, 2] -> (the stream's audio frames back to back as uint8, their sizes as int32 [n_blocks]); asx_flac_encode.
        ``bits_per_sample`` 24 writes every value shifted left by 8."""
        a = np.asarray(pcm)
        if a.dtype != np.int16 or a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"flac_encode expects int16 [n, 2], got {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a)
        plan = self.flac_plan(a.shape[0], 2, bits_per_sample, block_size)
        out = np.empty(plan["max_bytes"], np.uint8)
        sizes = np.empty(plan["n_blocks"], np.int32)
        total = C.c_int64()
        self._check(self._lib.asx_flac_encode(self._h, a.ctypes.data_as(C.POINTER(C.c_int16)), a.shape[0], int(samplerate), int(bits_per_sample),
                                              int(block_size), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size,
                                              sizes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(total)))
        return out[:total.value], sizes

    def flac_encode_dev(self, pcm_ptr: int, n_samples: int, samplerate: int, bits_per_sample: int, block_size: int, out_ptr: int,
                        out_capacity: int, frame_bytes_ptr: int, stream: int = 0) -> int:
        """asx_flac_encode_dev: device int16 [n, 2] -> frames in ``out_ptr`` (room for the plan's max_bytes), sizes in
        ``frame_bytes_ptr`` (int32 [n_blocks]); returns the frames' total bytes (synchronises the stream once)."""
        total = C.c_int64()
        self._check(self._lib.asx_flac_encode_dev(self._h, pcm_ptr, int(n_samples), int(samplerate), int(bits_per_sample), int(block_size), out_ptr,
                                                  int(out_capacity), frame_bytes_ptr, C.byref(total), stream or None))
        return total.value

    @staticmethod
    def flac_plan_pcm(n_samples: int, channels: int = 2, bits_per_sample: int = 24, block_size: int = FLAC_BLOCK_SIZE) -> dict:
        """asx_flac_plan_pcm (pure host): ``flac_plan`` for the encoder of int32 samples of 16 or 24 real bits, whose worst frame is
        header + 2 x (16 + (bits_per_sample + 1) x block_size) bits + padding + CRC-16."""
        return Engine._flac_plan("asx_flac_plan_pcm", n_samples, channels, bits_per_sample, block_size)

    def flac_encode_pcm(self, pcm: np.ndarray, samplerate: int, bits_per_sample: int = 24, block_size: int = FLAC_BLOCK_SIZE):
        """int32 [n, 2] samples of ``bits_per_sample`` (16 or 24) real bits -> (the stream's audio frames back to back as uint8, their
        sizes as int32 [n_blocks]); asx_flac_encode_pcm.  A sample outside the width is refused."""
        a = np.asarray(pcm)
        if a.dtype != np.int32 or a.ndim != 2 or a.shape[1] != 2:
            raise ValueError(f"flac_encode_pcm expects int32 [n, 2], got {a.dtype} {a.shape}")
        a = np.ascontiguousarray(a)
        plan = self.flac_plan_pcm(a.shape[0], 2, bits_per_sample, block_size)
        out = np.empty(plan["max_bytes"], np.uint8)
        sizes = np.empty(plan["n_blocks"], np.int32)
        total = C.c_int64()
        self._check(self._lib.asx_flac_encode_pcm(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0], int(samplerate), int(bits_per_sample),
                                                  int(block_size), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size,
                                                  sizes.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(total)))
        return out[:total.value], sizes

    def flac_encode_pcm_dev(self, pcm_ptr: int, n_samples: int, samplerate: int, bits_per_sample: int, block_size: int, out_ptr: int,
                            out_capacity: int, frame_bytes_ptr: int, stream: int = 0) -> int:
        """asx_flac_encode_pcm_dev: device int32 [n, 2] (``pcm_encode_dev`` with "S16_IN_32" / "S24_IN_32") -> frames in ``out_ptr`` (room
        for ``flac_plan_pcm``'s max_bytes), sizes in ``frame_bytes_ptr``; returns the frames' total bytes (synchronises the stream once)."""
        total = C.c_int64()
        self._check(self._lib.asx_flac_encode_pcm_dev(self._h, pcm_ptr, int(n_samples), int(samplerate), int(bits_per_sample), int(block_size),
                                                      out_ptr, int(out_capacity), frame_bytes_ptr, C.byref(total), stream or None))
        return total.value

    @staticmethod
    def flac_decode_plan(audio_bytes: int, channels: int = 2, bits_per_sample: int = 16, max_blocksize: int = FLAC_BLOCK_SIZE,
                         max_framesize: int = 0) -> dict:
        """asx_flac_decode_plan (pure host: no engine, no GPU): {max_candidates, slot_bytes, scratch_bytes} of the FLAC decoder for an audio
        part of ``audio_bytes``.  Raises AsxError for what the decoder refuses: widths outside 8 .. 24 bits, more than two channels, a
        maximum block size outside 16 .. 16384, empty input."""
        lib = load_library()
        cap, slot, scratch = C.c_int64(), C.c_int64(), C.c_int64()
        rc = lib.asx_flac_decode_plan(int(audio_bytes), int(channels), int(bits_per_sample), int(max_blocksize), int(max_framesize),
                                      C.byref(cap), C.byref(slot), C.byref(scratch))
        if rc != 0:
            msg = lib.asx_last_error()
            raise AsxError(f"asx error {rc}: {msg.decode() if msg else '?'}")
        return {"max_candidates": cap.value, "slot_bytes": slot.value, "scratch_bytes": scratch.value}

    def flac_decode_scan_dev(self, audio_ptr: int, audio_bytes: int, info: dict, stream: int = 0) -> dict:
        """asx_flac_decode_scan_dev: the audio part of a FLAC stream on the device (``info``: audio_io.flac_stream's STREAMINFO fields) ->
        {n_samples, n_frames, bytes_consumed}; the decoded frames stay in engine scratch for ``flac_decode_finish_dev``."""
        n, nf, used = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.asx_flac_decode_scan_dev(self._h, audio_ptr, int(audio_bytes), int(info["samplerate"]), int(info["channels"]),
                                                       int(info["bits_per_sample"]), int(info["max_blocksize"]), int(info["max_framesize"]),
                                                       C.byref(n), C.byref(nf), C.byref(used), stream or None))
        return {"n_samples": n.value, "n_frames": nf.value, "bytes_consumed": used.value}

    def flac_decode_finish_dev(self, mix_ptr: int, n_samples: int, stream: int = 0, want_peak: bool = True):
        """asx_flac_decode_finish_dev: the frames of the last scan -> float32 planar [2, n_samples] at ``mix_ptr``; returns max |mix|
        (synchronises the stream) or None."""
        pk = C.c_float()
        self._check(self._lib.asx_flac_decode_finish_dev(self._h, mix_ptr, int(n_samples), C.byref(pk) if want_peak else None, stream or None))
        return pk.value if want_peak else None

    def flac_decode(self, data, info: dict, details: bool = False):
        """The audio part of a FLAC stream (bytes or uint8 array) -> float32 [2, n]; asx_flac_decode.  ``details``: also
        {n_samples, n_frames, bytes_consumed, peak}."""
        a = np.frombuffer(data, np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, np.uint8).reshape(-1)
        args = (int(info["samplerate"]), int(info["channels"]), int(info["bits_per_sample"]), int(info["max_blocksize"]), int(info["max_framesize"]))
        self.flac_decode_plan(a.size, *args[1:])
        n, nf, used, pk = C.c_int64(), C.c_int64(), C.c_int64(), C.c_float()
        capacity = int(info.get("total_samples") or 0) or 16 * a.size
        for _ in range(2):                       # total_samples is a hint: a stream that holds more is decoded again at its own count
            out = np.empty((2, capacity), np.float32)
            rc = self._lib.asx_flac_decode(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.size, *args, _ptr(out), capacity, C.byref(n),
                                           C.byref(nf), C.byref(used), C.byref(pk))
            if rc == 0 or n.value <= capacity:
                break
            capacity = n.value
        self._check(rc)
        mix = np.ascontiguousarray(out.reshape(-1)[:2 * n.value].reshape(2, n.value))
        if details:
            return mix, {"n_samples": n.value, "n_frames": nf.value, "bytes_consumed": used.value, "peak": pk.value}
        return mix

    def pcm16_rows_dev(self, stem_ptr: int, n_samples: int, max_peak: float, min_peak, pcm_ptr: int, stream: int = 0,
                       want_peak: bool = True):
        """asx_pcm16_rows_dev: a device-resident [N, 2] stem -> int16 [N, 2] on the device; returns the peak after
        normalisation (synchronises the stream) or None."""
        pk = C.c_float()
        self._check(self._lib.asx_pcm16_rows_dev(self._h, stem_ptr, n_samples, float(max_peak), float(min_peak or 0.0),
                                                 int(min_peak is not None), pcm_ptr, C.byref(pk) if want_peak else None, stream or None))
        return pk.value if want_peak else None

    def pcm16_planar_dev(self, stem_ptr: int, n_samples: int, max_peak: float, min_peak, pcm_ptr: int, stream: int = 0,
                         want_peak: bool = True):
        """asx_pcm16_dev: a device-resident planar [2, N] stem -> int16 [N, 2] on the device; returns the peak after
        normalisation (synchronises the stream) or None."""
        pk = C.c_float()
        self._check(self._lib.asx_pcm16_dev(self._h, stem_ptr, n_samples, float(max_peak), float(min_peak or 0.0),
                                            int(min_peak is not None), pcm_ptr, C.byref(pk) if want_peak else None, stream or None))
        return pk.value if want_peak else None

    PCM_FORMATS = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32, "FLOAT": 0x120}

    # sample formats of pcm_encode*: the WAV subtypes, and the 16- / 24-bit integers in int32 containers that flac_encode_pcm_dev reads
    PCM_ENCODE_FORMATS = dict(PCM_FORMATS, S16_IN_32=0x410, S24_IN_32=0x418)
    PCM_ENCODE_DTYPES = {"PCM_16": ("<i2", 2), "PCM_24": ("u1", 6), "PCM_32": ("<i4", 2), "FLOAT": ("<f4", 2), "S16_IN_32": ("<i4", 2),
                         "S24_IN_32": ("<i4", 2)}          # numpy dtype and columns per frame of the encoded body
    STEM_LAYOUTS = {"planar": 0, "rows": 1}

    def pcm_encode(self, stem: np.ndarray, subtype: str, max_peak: float = 1.0, min_peak=None, layout: str = "rows"):
        """write_audio_soundfile's array work: ``stem`` float32 [n, 2] (``layout`` "rows") or [2, n] ("planar") -> (the samples in the
        file's format, interleaved: [n, 2] of the subtype's dtype, PCM_24 as uint8 [n, 6]; the peak after normalisation).  asx_pcm_encode."""
        if subtype not in self.PCM_ENCODE_FORMATS:
            raise ValueError(f"no device encoder for subtype {subtype}")
        a = np.ascontiguousarray(stem, np.float32)
        if a.ndim != 2 or a.shape[1 if layout == "rows" else 0] != 2:
            raise ValueError(f"pcm_encode expects a {'[n, 2]' if layout == 'rows' else '[2, n]'} stem, got {a.shape}")
        n = a.shape[0 if layout == "rows" else 1]
        dtype, cols = self.PCM_ENCODE_DTYPES[subtype]
        out = np.empty((n, cols), dtype)
        pk = C.c_float()
        self._check(self._lib.asx_pcm_encode(self._h, _ptr(a), n, self.STEM_LAYOUTS[layout], float(max_peak), float(min_peak or 0.0),
                                             int(min_peak is not None), self.PCM_ENCODE_FORMATS[subtype], out.ctypes.data, C.byref(pk)))
        return out, pk.value

    def pcm_encode_dev(self, stem_ptr: int, n_samples: int, layout: str, max_peak: float, min_peak, subtype: str, out_ptr: int,
                       stream: int = 0, want_peak: bool = True):
        """asx_pcm_encode_dev: a device-resident stem (only read) -> the body of a WAVE data chunk at ``out_ptr`` (16-byte aligned,
        n_samples x 4, 6 or 8 bytes); returns the peak after normalisation (synchronises the stream) or None."""
        if subtype not in self.PCM_ENCODE_FORMATS:
            raise ValueError(f"no device encoder for subtype {subtype}")
        pk = C.c_float()
        self._check(self._lib.asx_pcm_encode_dev(self._h, stem_ptr, int(n_samples), self.STEM_LAYOUTS[layout], float(max_peak),
                                                 float(min_peak or 0.0), int(min_peak is not None), self.PCM_ENCODE_FORMATS[subtype], out_ptr,
                                                 C.byref(pk) if want_peak else None, stream or None))
        return pk.value if want_peak else None

    def pcm_decode_dev(self, raw_ptr: int, frames: int, channels: int, subtype: str, mix_ptr: int, stream: int = 0,
                       want_peak: bool = True):
        """asx_pcm_decode_dev: a WAVE data chunk on the device -> float32 planar [2, frames]; returns max |mix| or None."""
        if subtype not in self.PCM_FORMATS:
            raise ValueError(f"no device decoder for subtype {subtype}")
        pk = C.c_float()
        self._check(self._lib.asx_pcm_decode_dev(self._h, raw_ptr, frames, channels, self.PCM_FORMATS[subtype], mix_ptr,
                                                 C.byref(pk) if want_peak else None, stream or None))
        return pk.value if want_peak else None

    def normalize(self, wave: np.ndarray, max_peak: float = 1.0, min_peak=None) -> np.ndarray:
        """spec_utils.normalize (uvr_lib_v5/spec_utils.py:99-115): scales ``wave`` IN PLACE when it is a C-contiguous float32
        array (like the reference, whose ``wave *= ...`` mutates the caller's array) and returns it."""
        a = wave if (isinstance(wave, np.ndarray) and wave.dtype == np.float32 and wave.flags.c_contiguous) else None
        buf = a if a is not None else np.ascontiguousarray(wave, np.float32)
        if buf.size:
            pk = C.c_float()
            self._check(self._lib.asx_normalize(self._h, _ptr(buf), buf.size, float(max_peak), float(min_peak or 0.0),
                                                int(min_peak is not None), C.byref(pk)))
        if a is None and isinstance(wave, np.ndarray) and wave.dtype == np.float32:
            wave[...] = buf                      # non-contiguous view (e.g. a transposed stem): write the result back
            return wave
        return buf

    def normalize_dev(self, wave_ptr: int, numel: int, max_peak: float = 1.0, min_peak=None, stream: int = 0):
        self._check(self._lib.asx_normalize_dev(self._h, wave_ptr, numel, float(max_peak), float(min_peak or 0.0),
                                                int(min_peak is not None), stream or None))

    def normalize_scale_dev(self, wave_ptr: int, numel: int, max_peak: float = 1.0, min_peak=None, stream: int = 0) -> float:
        """The float32 factor ``normalize_dev`` with these arguments would multiply the array by (1.0: it would leave it alone).  Reads
        the array's peak -- four bytes -- back, so it waits for ``stream``; the array is not changed."""
        q = C.c_float()
        self._check(self._lib.asx_normalize_scale_dev(self._h, wave_ptr, numel, float(max_peak), float(min_peak or 0.0),
                                                      int(min_peak is not None), C.byref(q), stream or None))
        return q.value

    def residual_dev(self, mix_ptr: int, stem_ptr: int, out_ptr: int, numel: int, stream: int = 0):
        self._check(self._lib.asx_residual_dev(self._h, mix_ptr, stem_ptr, out_ptr, numel, stream or None))

    ENSEMBLE_ALGORITHMS = ("avg_wave", "median_wave", "min_wave", "max_wave", "avg_fft", "median_fft", "min_fft", "max_fft",
                           "uvr_max_spec", "uvr_min_spec", "ensemble_wav")

    def ensemble(self, waveforms, algorithm: str = "avg_wave", weights=None) -> np.ndarray:
        """Ensembler.ensemble (ensembler.py:12-74): list of [2, N] waves (zero-padded to the longest) -> [2, N']."""
        if algorithm not in self.ENSEMBLE_ALGORITHMS:
            raise ValueError(f"Unknown ensemble algorithm: {algorithm}")
        ws = [_f32(w) for w in waveforms]
        if len(ws) == 1:
            return ws[0]
        if any(w.ndim != 2 or w.shape[0] != 2 for w in ws):
            raise ValueError("All waveforms must be stereo [2, N] for the accelerated ensemble")
        n = max(w.shape[1] for w in ws)
        stack = np.zeros((len(ws), 2, n), np.float32)
        for k, w in enumerate(ws):
            stack[k, :, : w.shape[1]] = w
        wl = self.ensemble_weights(weights, len(ws))
        wt = (C.c_double * len(ws))(*wl) if wl is not None else None
        out = np.empty((2, n), np.float32)
        n_out = C.c_int64()
        self._check(self._lib.asx_ensemble(self._h, _ptr(stack), len(ws), n, self.ENSEMBLE_ALGORITHMS.index(algorithm), wt, _ptr(out),
                                           C.byref(n_out)))
        return out.reshape(-1)[: 2 * n_out.value].reshape(2, n_out.value).copy()     # the engine writes planar [2, n_out]

    @staticmethod
    def ensemble_weights(weights, k: int):
        """The weights Ensembler.ensemble ends up using (ensembler.py:32-44), as a list of k floats, or None for equal weights:
        a length mismatch, a non-finite value or a zero sum falls back to equal weights."""
        if weights is None or len(weights) != k:
            return None
        w = np.asarray(weights, np.float64)
        total = np.sum(w)
        if not np.all(np.isfinite(w)) or not np.isfinite(total) or total == 0:
            return None
        return [float(v) for v in w]

    SLOT_LAYOUTS = {"planar": 0, "rows": 1}
    # "pcm16" / "float32": the reference's 16-bit intermediate (pydub's truncating writer) / no round trip; the subtype names: the file a
    # member writes with soundfile, as asx_pcm_encode_dev writes and asx_pcm_decode_dev reads it ("PCM_16" rounds, "pcm16" truncates)
    SLOT_MODES = {"pcm16": 0, "float32": 1, "PCM_16": 16, "PCM_24": 24, "PCM_32": 32, "FLOAT": 0x120}

    @classmethod
    def _slot_mode(cls, mode) -> int:
        if not isinstance(mode, str) or mode not in cls.SLOT_MODES:
            raise ValueError(f"unknown slot mode {mode!r} (one of {tuple(cls.SLOT_MODES)})")
        return cls.SLOT_MODES[mode]

    def ensemble_slot_dev(self, stem_ptr: int, n_samples: int, layout: str, max_peak: float, min_peak, stack_ptr: int, k: int,
                          n_max: int, mode: str = "pcm16", stream: int = 0, want_peak: bool = True):
        """asx_ensemble_slot_dev: a device stem (``layout`` "planar" [2, n] or "rows" [n, 2]) -> slot ``k`` of the device stack
        [K, 2, n_max] through the member's file round trip (``mode`` "pcm16": normalise, int16, / 32768 -- bit-exact to
        pcm16_*_dev followed by librosa.load), as it is ("float32"), or through the file of that subtype a soundfile writer leaves
        ("PCM_16", "PCM_24", "PCM_32", "FLOAT": bit-exact to pcm_encode_dev followed by pcm_decode_dev); zero padded to ``n_max``.
        Returns the peak after normalisation (the raw peak for "float32"; synchronises the stream) or None.  An unknown ``mode``
        raises ValueError."""
        mode_code = self._slot_mode(mode)
        pk = C.c_float()
        self._check(self._lib.asx_ensemble_slot_dev(self._h, stem_ptr or None, n_samples, self.SLOT_LAYOUTS[layout], float(max_peak),
                                                    float(min_peak or 0.0), int(min_peak is not None), mode_code,
                                                    stack_ptr or None, k, n_max, C.byref(pk) if want_peak else None, stream or None))
        return pk.value if want_peak else None

    def ensemble_dev(self, stack_ptr: int, k: int, n_samples: int, algorithm: str, weights, out_ptr: int, stream: int = 0) -> int:
        """asx_ensemble_dev: a device stack [k, 2, n] -> ``out`` [2, n_out] on the device (room for [2, n]); returns n_out
        (n, or 1024 * (n // 1024) for the uvr_* algorithms).  ``weights`` as Ensembler.ensemble treats them."""
        if algorithm not in self.ENSEMBLE_ALGORITHMS:
            raise ValueError(f"Unknown ensemble algorithm: {algorithm}")
        w = self.ensemble_weights(weights, k)
        wt = (C.c_double * k)(*w) if w is not None else None
        n_out = C.c_int64()
        self._check(self._lib.asx_ensemble_dev(self._h, stack_ptr or None, k, n_samples, self.ENSEMBLE_ALGORITHMS.index(algorithm), wt,
                                               out_ptr or None, C.byref(n_out), stream or None))
        return int(n_out.value)

    def ensemble_batch_dev(self, jobs, algorithm, weights, max_peak: float, min_peak, silent_below: float = 1e-6, mode: str = "pcm16",
                           stream: int = 0, modes=None):
        """asx_ensemble_batch_dev: the ensembles of many (file, stem group) jobs in one call.  ``jobs``: a list of
        ``(contributors, out_ptr, out_capacity)`` with ``contributors`` = [(stem_ptr, n_samples, "planar" | "rows")], 1 .. 8 of them,
        and ``out`` a device buffer of 2 * out_capacity floats, out_capacity >= the longest contributor.  Per job, bit for bit what
        ``ensemble_slot_dev`` per contributor (dropping those whose peak is below ``silent_below`` and padding the rest to the
        longest left) followed by ``ensemble_dev`` gives; a lone contributor left comes out as its slot image.  ``weights`` as
        Ensembler.ensemble treats them: used by a job with exactly that many contributors left, equal weights otherwise.
        ``mode``: the slot mode of every contributor; ``modes`` (asx_ensemble_batch_modes_dev): per job the list of its contributors'
        modes instead -- members of one ensemble can write the same file in different formats.  An unknown name raises ValueError.
        Returns per job ``(n_out, live, [peak_after per contributor])``: ``out`` holds planar [2, n_out]; n_out == 0: no result,
        nothing written.  Synchronises the stream once (for the peaks); the combine itself is only enqueued."""
        if isinstance(algorithm, str):
            if algorithm not in self.ENSEMBLE_ALGORITHMS:
                raise ValueError(f"Unknown ensemble algorithm: {algorithm}")
            algorithm = self.ENSEMBLE_ALGORITHMS.index(algorithm)
        jobs = list(jobs)
        mode_code, mode_table = self._slot_mode(mode), None
        if modes is not None:
            modes = [list(m) for m in modes]
            if len(modes) != len(jobs) or any(len(m) != len(list(job[0])) for m, job in zip(modes, jobs)):
                raise ValueError("modes must hold one mode per contributor of every job")
            mode_table = (C.c_int32 * (ENS_MAX_K * max(1, len(jobs))))()
            for j, m in enumerate(modes):
                for c, name in enumerate(m):
                    code = self._slot_mode(name)
                    if c < ENS_MAX_K:
                        mode_table[j * ENS_MAX_K + c] = code
        w = self.ensemble_weights(weights, len(weights)) if weights is not None and 0 < len(weights) <= ENS_MAX_K else None
        wt = (C.c_double * len(w))(*w) if w is not None else None
        arr = (_EnsJob * max(1, len(jobs)))()
        for j, (contributors, out_ptr, capacity) in enumerate(jobs):
            contributors = list(contributors)
            arr[j].k = len(contributors)
            for c, (ptr, n, layout) in enumerate(contributors[:ENS_MAX_K]):
                arr[j].stem_dev[c], arr[j].n_samples[c], arr[j].layout[c] = ptr or None, int(n), self.SLOT_LAYOUTS[layout]
            arr[j].out_dev, arr[j].out_capacity = out_ptr or None, int(capacity)
        if mode_table is not None:
            self._check(self._lib.asx_ensemble_batch_modes_dev(self._h, arr, len(jobs), mode_table, int(algorithm), wt, len(w) if w is not None else 0,
                                                               float(max_peak), float(min_peak or 0.0), int(min_peak is not None),
                                                               float(silent_below), stream or None))
        else:
            self._check(self._lib.asx_ensemble_batch_dev(self._h, arr, len(jobs), int(algorithm), wt, len(w) if w is not None else 0,
                                                         mode_code, float(max_peak), float(min_peak or 0.0), int(min_peak is not None),
                                                         float(silent_below), stream or None))
        return [(int(arr[j].n_out), int(arr[j].live), [float(arr[j].peak_after[c]) for c in range(min(arr[j].k, ENS_MAX_K))])
                for j in range(len(jobs))]

    def mixdown_batch_dev(self, jobs, stream: int = 0):
        """asx_mixdown_batch_dev: weighted sums of device-resident stems, all jobs in one launch.  ``jobs``: a list of
        ``(sources, out_ptr, out_layout, n_out)`` with ``sources`` = [(ptr, "planar" | "rows", n_samples, weight)], 1 .. 8 of them; ``out``
        a device buffer of 2 * n_out floats.  Per sample acc = fl(w_0 x_0), acc = fl(acc + fl(w_k x_k)) in list order, float32, a source
        shorter than n_out zero-extended.  Only enqueues work on ``stream``."""
        jobs = list(jobs)
        arr = (_MixJob * max(1, len(jobs)))()
        for j, (sources, out_ptr, out_layout, n_out) in enumerate(jobs):
            sources = list(sources)
            if not 1 <= len(sources) <= MIX_MAX_K:
                raise ValueError(f"a mix-down takes 1 .. {MIX_MAX_K} sources, not {len(sources)}")
            arr[j].k = len(sources)
            for k, (ptr, layout, n, w) in enumerate(sources):
                arr[j].src[k].x, arr[j].src[k].layout, arr[j].src[k].n, arr[j].src[k].w = ptr or None, self.STEM_LAYOUTS[layout], int(n), float(w)
            arr[j].out, arr[j].out_layout, arr[j].n_out = out_ptr or None, self.STEM_LAYOUTS[out_layout], int(n_out)
        self._check(self._lib.asx_mixdown_batch_dev(self._h, arr, len(jobs), stream or None))

    def mixdown(self, sources, n_out: int = None, out_layout: str = "planar") -> np.ndarray:
        """asx_mixdown: one job of ``mixdown_batch_dev`` on host arrays.  ``sources``: [(float32 array [2, n] or [n, 2], "planar" | "rows",
        weight)]; returns [2, n_out] or [n_out, 2] (``n_out``: the longest source unless given)."""
        sources = [(np.ascontiguousarray(a, np.float32), layout, float(w)) for a, layout, w in sources]
        if not 1 <= len(sources) <= MIX_MAX_K:
            raise ValueError(f"a mix-down takes 1 .. {MIX_MAX_K} sources, not {len(sources)}")
        for a, layout, _ in sources:
            if a.ndim != 2 or a.shape[1 if layout == "rows" else 0] != 2:
                raise ValueError(f"mixdown expects {'[n, 2]' if layout == 'rows' else '[2, n]'} sources, got {a.shape}")
        ns = [a.shape[0 if layout == "rows" else 1] for a, layout, _ in sources]
        n_out = max(ns) if n_out is None else int(n_out)
        k = len(sources)
        out = np.empty((n_out, 2) if out_layout == "rows" else (2, n_out), np.float32)
        ptrs = (C.c_void_p * k)(*[a.ctypes.data if a.size else None for a, _, _ in sources])
        self._check(self._lib.asx_mixdown(self._h, ptrs, (C.c_int32 * k)(*[self.STEM_LAYOUTS[layout] for _, layout, _ in sources]),
                                          (C.c_int64 * k)(*ns), (C.c_float * k)(*[w for _, _, w in sources]), k, _ptr(out),
                                          self.STEM_LAYOUTS[out_layout], n_out))
        return out

    @staticmethod
    def _phase_weights(bin_weights) -> np.ndarray:
        w = np.ascontiguousarray(bin_weights, np.float32)
        if w.shape != (PHASE_BINS,):
            raise ValueError(f"the phase fix takes one weight per bin, {PHASE_BINS} of them, not an array of shape {w.shape}")
        return w

    def _phase_job(self, job) -> _PhaseJob:
        (t_ptr, t_layout, n), (s_ptr, s_layout, n_src), (o_ptr, o_layout) = job
        return _PhaseJob(t_ptr or None, s_ptr or None, o_ptr or None, int(n), int(n_src), self.STEM_LAYOUTS[t_layout], self.STEM_LAYOUTS[s_layout],
                         self.STEM_LAYOUTS[o_layout], 0)

    def phase_fix_batch_dev(self, jobs, bin_weights, hop: int = 512, stream: int = 0):
        """asx_phase_fix_batch_dev: the STFT magnitudes of a target stem on phases blended towards a source stem's, device-resident stems,
        one launch per stage over all jobs.  ``jobs``: a list of ``((target_ptr, layout, n), (source_ptr, layout, n_source), (out_ptr,
        layout))``, layouts "planar" [2, n] or "rows" [n, 2]; the source is zero-extended or cut to the target's ``n``, ``out`` holds
        2 * n floats.  ``bin_weights``: 1025 float32, the blend per bin of the 2048-point STFT (phasefix.bin_weights).  Only enqueues work
        on ``stream``."""
        jobs = list(jobs)
        w = self._phase_weights(bin_weights)
        arr = (_PhaseJob * max(1, len(jobs)))()
        for j, job in enumerate(jobs):
            arr[j] = self._phase_job(job)
        self._check(self._lib.asx_phase_fix_batch_dev(self._h, arr, len(jobs), _ptr(w), int(hop), stream or None))

    def phase_fix_dev(self, target, source, out, bin_weights, hop: int = 512, stream: int = 0):
        """asx_phase_fix_dev: one job of ``phase_fix_batch_dev`` -- ``target`` = (ptr, layout, n), ``source`` = (ptr, layout, n_source),
        ``out`` = (ptr, layout) -- passed by value to the same device functions: the same bits."""
        w = self._phase_weights(bin_weights)
        job = self._phase_job((target, source, out))
        self._check(self._lib.asx_phase_fix_dev(self._h, C.byref(job), _ptr(w), int(hop), stream or None))

    def phase_fix(self, target, source, bin_weights, hop: int = 512, target_layout: str = "rows", source_layout: str = "rows",
                  out_layout: str = "rows") -> np.ndarray:
        """asx_phase_fix: one job on host arrays (upload, the same launches, download).  ``target`` / ``source``: float32 [n, 2] ("rows") or
        [2, n] ("planar"); returns the result in ``out_layout`` with the target's length."""
        w = self._phase_weights(bin_weights)
        arrays = []
        for a, layout, what in ((target, target_layout, "target"), (source, source_layout, "source")):
            a = np.ascontiguousarray(a, np.float32)
            if a.ndim != 2 or a.shape[1 if layout == "rows" else 0] != 2:
                raise ValueError(f"phase_fix expects a {'[n, 2]' if layout == 'rows' else '[2, n]'} {what}, got {a.shape}")
            arrays.append((a, a.shape[0 if layout == "rows" else 1]))
        (t, n), (s, n_src) = arrays
        out = np.empty((n, 2) if out_layout == "rows" else (2, n), np.float32)
        self._check(self._lib.asx_phase_fix(self._h, _ptr(t) if n else None, self.STEM_LAYOUTS[target_layout], n, _ptr(s) if n_src else None,
                                            self.STEM_LAYOUTS[source_layout], n_src, _ptr(w), int(hop), _ptr(out) if n else None,
                                            self.STEM_LAYOUTS[out_layout]))
        return out

    def invert_stem(self, mixture: np.ndarray, stem: np.ndarray) -> np.ndarray:
        """spec_utils.invert_stem(mixture [2, N], stem [2, N]) -> [N', 2]."""
        m, st = _f32(mixture), _f32(stem)
        n = min(m.shape[1], st.shape[1])
        m, st = np.ascontiguousarray(m[:, :n]), np.ascontiguousarray(st[:, :n])
        out = np.empty((2, n), np.float32)
        n_out = C.c_int64()
        self._check(self._lib.asx_invert_stem(self._h, _ptr(m), _ptr(st), n, _ptr(out), C.byref(n_out)))
        return np.ascontiguousarray(out.reshape(-1)[: 2 * n_out.value].reshape(2, n_out.value).T)

    def invert_stem_dev(self, mix_ptr: int, stem_ptr: int, n_samples: int, stem_layout: str, stem_scale: float, out_ptr: int,
                        out_capacity: int, stream: int = 0) -> int:
        """asx_invert_stem_dev: spec_utils.invert_stem(mix, stem * stem_scale) with every array in HBM.  ``mix`` planar [2, n],
        ``stem`` "planar" [2, n] or "rows" [n, 2], ``out`` rows with room for [out_capacity, 2].  Returns n_out =
        1024 * (n // 1024); only enqueues work on ``stream``."""
        n_out = C.c_int64()
        self._check(self._lib.asx_invert_stem_dev(self._h, mix_ptr or None, stem_ptr or None, int(n_samples), self.SLOT_LAYOUTS[stem_layout],
                                                  float(stem_scale), out_ptr or None, int(out_capacity), C.byref(n_out), stream or None))
        return int(n_out.value)

    def invert_stem_batch_dev(self, songs, stem_scale: float, stream: int = 0) -> list:
        """asx_invert_stem_batch_dev: ``invert_stem_dev`` for a list of ``(mix_ptr, stem_ptr, n_samples, stem_layout, out_ptr,
        out_capacity)`` with one launch per stage over all songs; every result equals the single call's bit for bit.  Returns the
        list of n_out."""
        songs = list(songs)
        arr = (_InvertSong * max(1, len(songs)))()
        for i, (mix_ptr, stem_ptr, n, layout, out_ptr, capacity) in enumerate(songs):
            arr[i] = _InvertSong(mix_ptr or None, stem_ptr or None, out_ptr or None, int(n), int(capacity), 0, self.SLOT_LAYOUTS[layout])
        self._check(self._lib.asx_invert_stem_batch_dev(self._h, arr, len(songs), float(stem_scale), stream or None))
        return [int(arr[i].n_out) for i in range(len(songs))]

    def debug_fetch(self, name: str, shape) -> np.ndarray:
        out = np.empty(shape, np.float32)
        self._check(self._lib.asx_debug_fetch(self._h, name.encode(), _ptr(out), out.size))
        return out

    # -- plan ---------------------------------------------------------------
    def plan(self, n_samples: int, is_match_mix: bool = False) -> dict:
        p = _Plan()
        self._check(self._lib.asx_plan_query(self._h, n_samples, ASX_FLAG_MATCH_MIX if is_match_mix else 0,
                                             C.byref(p)))
        return {k: getattr(p, k) for k, _ in _Plan._fields_ if k != "reserved"}

    # -- the path -----------------------------------------------------------
    def demix(self, mix: np.ndarray, is_match_mix: bool = False) -> np.ndarray:
        mix = _f32(mix)
        if mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
        out = np.empty_like(mix)
        self._check(self._lib.asx_demix(self._h, _ptr(mix), mix.shape[1], _ptr(out),
                                        ASX_FLAG_MATCH_MIX if is_match_mix else 0))
        return out

    def demix_dev(self, mix_ptr: int, n_samples: int, out_ptr: int, is_match_mix: bool = False, stream: int = 0):
        self._check(self._lib.asx_demix_dev(self._h, mix_ptr, n_samples, out_ptr,
                                            ASX_FLAG_MATCH_MIX if is_match_mix else 0, stream or None))

    def demix_chunks_dev(self, mix_ptr: int, n_samples: int, k0: int, k1: int, chunk_out_ptr: int,
                         is_match_mix: bool = False, stream: int = 0):
        self._check(self._lib.asx_demix_chunks_dev(self._h, mix_ptr, n_samples, k0, k1, chunk_out_ptr,
                                                   ASX_FLAG_MATCH_MIX if is_match_mix else 0, stream or None))

    def finalize_dev(self, chunk_out_ptr: int, n_samples: int, out_ptr: int, is_match_mix: bool = False,
                     stream: int = 0):
        self._check(self._lib.asx_finalize_dev(self._h, chunk_out_ptr, n_samples, out_ptr,
                                               ASX_FLAG_MATCH_MIX if is_match_mix else 0, stream or None))

    def separate(self, mix: np.ndarray, max_peak: float, min_peak, compensate: float):
        """Stem algebra of MDXSeparator.separate on the device.  ``mix`` (float32 [2,N], C-contiguous) is
        normalised IN PLACE like the reference does; returns (primary [N,2], secondary [N,2])."""
        if mix.dtype != np.float32 or not mix.flags.c_contiguous or mix.ndim != 2 or mix.shape[0] != 2:
            raise ValueError("mix must be a C-contiguous float32 array of shape [2, N]")
        n = mix.shape[1]
        primary = np.empty((n, 2), np.float32)
        secondary = np.empty((n, 2), np.float32)
        self._check(self._lib.asx_separate(self._h, _ptr(mix), n, float(max_peak),
                                           float(min_peak) if min_peak is not None else 0.0,
                                           int(min_peak is not None), float(compensate), _ptr(primary),
                                           _ptr(secondary)))
        return primary, secondary

    def separate_dev(self, mix_ptr: int, n_samples: int, max_peak: float, min_peak, compensate: float,
                     primary_ptr: int, secondary_ptr: int, stream: int = 0):
        self._check(self._lib.asx_separate_dev(self._h, mix_ptr, n_samples, float(max_peak),
                                               float(min_peak) if min_peak is not None else 0.0,
                                               int(min_peak is not None), float(compensate), primary_ptr,
                                               secondary_ptr, stream or None))

    # -- a batch of songs in one call: the chunks of all of them pooled per launch ------------------------------------
    def demix_batch_dev(self, songs, is_match_mix: bool = False, stream: int = 0):
        """``songs``: a list of ``(mix_ptr, out_ptr, n_samples)`` -- device pointers to float32 [2, n_samples] each.  Every
        ``out`` equals what ``demix_dev`` writes for that song alone, bit for bit (asx_demix_batch_dev)."""
        songs = list(songs)
        arr = (_Song * max(1, len(songs)))()
        for i, (mix_ptr, out_ptr, n) in enumerate(songs):
            arr[i] = _Song(mix_ptr or None, out_ptr or None, int(n))
        self._check(self._lib.asx_demix_batch_dev(self._h, arr, len(songs), ASX_FLAG_MATCH_MIX if is_match_mix else 0,
                                                  stream or None))

    def separate_batch_dev(self, songs, max_peak: float, min_peak, compensate: float, stream: int = 0):
        """``songs``: a list of ``(mix_ptr, primary_ptr, secondary_ptr, n_samples)``; per song what ``separate_dev`` does
        (mix [2, n] normalised in place, stems [n, 2]), all songs through one pooled demix (asx_separate_batch_dev)."""
        songs = list(songs)
        arr = (_SongStems * max(1, len(songs)))()
        for i, (mix_ptr, p_ptr, s_ptr, n) in enumerate(songs):
            arr[i] = _SongStems(mix_ptr or None, p_ptr or None, s_ptr or None, int(n))
        self._check(self._lib.asx_separate_batch_dev(self._h, arr, len(songs), float(max_peak),
                                                     float(min_peak) if min_peak is not None else 0.0,
                                                     int(min_peak is not None), float(compensate), stream or None))

    def _torch_stream(self):
        import torch
        dev = torch.device("cuda", self.device)
        return torch, dev, torch.cuda.current_stream(dev)

    def demix_batch(self, mixes, is_match_mix: bool = False) -> list:
        """``demix`` for a list of float32 [2, N_i] arrays in one pooled call; returns the list of [2, N_i] results.  Device
        staging buffers come from torch (the plumbing layer), as in the file-level path."""
        host = []
        for mix in mixes:
            mix = _f32(mix)
            if mix.ndim != 2 or mix.shape[0] != 2:
                raise ValueError(f"Expected a 2-channel audio signal, but got shape {mix.shape}")
            host.append(mix)
        if not host:
            return []
        torch, dev, st = self._torch_stream()
        with torch.cuda.stream(st):
            d_mix = [torch.from_numpy(m).to(dev) for m in host]
            d_out = [torch.empty_like(m) for m in d_mix]
            self.demix_batch_dev([(m.data_ptr() if m.numel() else 0, o.data_ptr() if o.numel() else 0, m.shape[1])
                                  for m, o in zip(d_mix, d_out)], is_match_mix, st.cuda_stream)
            outs = [o.cpu().numpy() for o in d_out]
        return outs

    def separate_batch(self, mixes, max_peak: float, min_peak, compensate: float) -> list:
        """``separate`` for a list of mixes (each float32 [2, N_i], C-contiguous, normalised IN PLACE) in one pooled call;
        returns ``[(primary [N_i, 2], secondary [N_i, 2]), ...]``."""
        for mix in mixes:
            if not isinstance(mix, np.ndarray) or mix.dtype != np.float32 or not mix.flags.c_contiguous or mix.ndim != 2 or mix.shape[0] != 2:
                raise ValueError("mix must be a C-contiguous float32 array of shape [2, N]")
        if not len(mixes):
            return []
        torch, dev, st = self._torch_stream()
        with torch.cuda.stream(st):
            d_mix = [torch.from_numpy(m).to(dev) for m in mixes]
            d_p = [torch.empty((m.shape[1], 2), dtype=torch.float32, device=dev) for m in mixes]
            d_s = [torch.empty((m.shape[1], 2), dtype=torch.float32, device=dev) for m in mixes]
            ptr = lambda t: t.data_ptr() if t.numel() else 0  # noqa: E731
            self.separate_batch_dev([(ptr(m), ptr(p), ptr(s), m.shape[1]) for m, p, s in zip(d_mix, d_p, d_s)],
                                    max_peak, min_peak, compensate, st.cuda_stream)
            res = []
            for m, dm, p, s in zip(mixes, d_mix, d_p, d_s):
                m[...] = dm.cpu().numpy()
                res.append((p.cpu().numpy(), s.cpu().numpy()))
        return res

    # -- stage hooks ----------------------------------------------------------
    def stft(self, wave: np.ndarray) -> np.ndarray:
        wave = _f32(wave)
        B, ch, Cn = wave.shape
        assert ch == 2
        T = Cn // self.cfg.hop_length + 1
        out = np.empty((B, 4, self.cfg.dim_f, T), np.float32)
        self._check(self._lib.asx_stft(self._h, _ptr(wave), B, Cn, _ptr(out)))
        return out

    def istft(self, spec: np.ndarray) -> np.ndarray:
        spec = _f32(spec)
        B, c4, Fq, T = spec.shape
        assert c4 == 4 and Fq == self.cfg.dim_f
        out = np.empty((B, 2, self.cfg.hop_length * (T - 1)), np.float32)
        self._check(self._lib.asx_istft(self._h, _ptr(spec), B, T, _ptr(out)))
        return out

    def net_forward(self, spec: np.ndarray) -> np.ndarray:
        spec = _f32(spec)
        out = np.empty_like(spec)
        self._check(self._lib.asx_net_forward(self._h, _ptr(spec), spec.shape[0], _ptr(out)))
        return out

    def run_model(self, wave: np.ndarray, is_match_mix: bool = False) -> np.ndarray:
        wave = _f32(wave)
        out = np.empty_like(wave)
        self._check(self._lib.asx_run_model(self._h, _ptr(wave), wave.shape[0], _ptr(out),
                                            ASX_FLAG_MATCH_MIX if is_match_mix else 0))
        return out

    def op_conv(self, op: str, x, w, b, aux=None, relu=True) -> np.ndarray:
        x, w, b = _f32(x), _f32(w), _f32(b)
        B, cin, t, f = x.shape
        if op == "up":
            cout = w.shape[1]
            shape = (B, cout, 2 * t, 2 * f)
        elif op == "down":
            cout = w.shape[0]
            shape = (B, cout, t // 2, f // 2)
        else:
            cout = w.shape[0]
            shape = (B, cout, t, f)
        aux = _f32(aux) if aux is not None else None
        y = np.empty(shape, np.float32)
        self._check(self._lib.asx_op_conv(self._h, op.encode(), _ptr(x), B, cin, t, f, _ptr(w), _ptr(b), cout,
                                          _optptr(aux), int(relu), _ptr(y)))
        return y

    def op_tdf(self, x, w, bias, scale, shift, res=None) -> np.ndarray:
        x, w, scale, shift = _f32(x), _f32(w), _f32(scale), _f32(shift)
        B, c, t, k = x.shape
        n = w.shape[0]
        bias = _f32(bias) if bias is not None else None
        res = _f32(res) if res is not None else None
        y = np.empty((B, c, t, n), np.float32)
        self._check(self._lib.asx_op_tdf(self._h, _ptr(x), B, c, t, k, _ptr(w), _optptr(bias), n, _ptr(scale),
                                         _ptr(shift), _optptr(res), _ptr(y)))
        return y

    def op_tdf_block(self, x, w0, scale0, shift0, w1, scale1, shift1, return_hidden=False):
        """x + tdf(x) of a TDF block with a bottleneck (two linears, launched as the net launches them); with return_hidden also the
        bottleneck activations as fp32 (decoded from the pair image when the first linear wrote one)."""
        x, w0, w1 = _f32(x), _f32(w0), _f32(w1)
        scale0, shift0, scale1, shift1 = _f32(scale0), _f32(shift0), _f32(scale1), _f32(shift1)
        B, c, t, f = x.shape
        n8 = w0.shape[0]
        if w0.shape != (n8, f) or w1.shape != (f, n8):
            raise AsxError(f"op_tdf_block: W0 {w0.shape} / W1 {w1.shape} do not fit rows of length {f}")
        y = np.empty((B, c, t, f), np.float32)
        h = np.empty((B, c, t, n8), np.float32) if return_hidden else None
        self._check(self._lib.asx_op_tdf_block(self._h, _ptr(x), B, c, t, f, _ptr(w0), _ptr(scale0), _ptr(shift0), n8, _ptr(w1),
                                               _ptr(scale1), _ptr(shift1), _ptr(y), _optptr(h)))
        return (y, h) if return_hidden else y

    def op_attention(self, qkv, gate, B, T, Fb, axis="time", exact=False, variant="auto", out=None):
        """One Roformer attention launch (asx_op_attention): qkv [M, 3 * heads * 64], gate [M, gate_ld] (gate_ld >= heads), tokens
        [B, T, Fb] along `axis` ("time" or "freq").  `out` [M, heads * 64] is uploaded before the launch (elements the kernel does not
        own keep their contents); default NaN.  Returns (out, name of the variant that ran)."""
        qkv, gate = _f32(qkv), _f32(gate)
        M, w = qkv.shape
        if w % 192 != 0 or gate.ndim != 2 or gate.shape[0] != M:
            raise AsxError(f"op_attention: qkv {qkv.shape} / gate {gate.shape} are not [M, 3 * heads * 64] / [M, gate_ld]")
        heads = w // 192
        if axis not in ("time", "freq"):
            raise AsxError(f"op_attention: axis must be 'time' or 'freq', got {axis!r}")
        out = np.full((M, heads * 64), np.nan, np.float32) if out is None else np.array(out, np.float32, order="C")
        if out.shape != (M, heads * 64):
            raise AsxError(f"op_attention: out {out.shape} is not [{M}, {heads * 64}]")
        res = C.c_int32(-1)
        self._check(self._lib.asx_op_attention(self._h, _ptr(qkv), _ptr(gate), M, B, T, Fb, 0 if axis == "time" else 1, heads,
                                               gate.shape[1], int(exact), variant.encode(), _ptr(out), C.byref(res)))
        return out, ATTN_VARIANTS[res.value]

    def op_mha(self, q, k, v, B, nq, nk, heads, dh, decay=None, exact=False, variant="auto", out=None):
        """One multi-head attention launch (asx_op_mha): q [B * nq, ldq], k / v [B * nk, ld], optional LocalState decay logits
        [B * nq, ldd]; head h owns columns [h * dh, (h + 1) * dh).  `out` [B * nq, ldo] (ldo >= heads * dh) is uploaded before the
        launch; default NaN of width heads * dh.  Returns (out, name of the variant that ran)."""
        q, k, v = _f32(q), _f32(k), _f32(v)
        if q.shape[0] != B * nq or k.shape[0] != B * nk or v.shape[0] != B * nk:
            raise AsxError(f"op_mha: q {q.shape} / k {k.shape} / v {v.shape} do not hold {B} x {nq} queries and {B} x {nk} keys")
        decay = _f32(decay) if decay is not None else None
        if decay is not None and decay.shape[0] != B * nq:
            raise AsxError(f"op_mha: decay {decay.shape} does not have {B * nq} rows")
        out = np.full((B * nq, heads * dh), np.nan, np.float32) if out is None else np.array(out, np.float32, order="C")
        if out.ndim != 2 or out.shape[0] != B * nq:
            raise AsxError(f"op_mha: out {out.shape} does not have {B * nq} rows")
        res = C.c_int32(-1)
        self._check(self._lib.asx_op_mha(self._h, _ptr(q), q.shape[1], _ptr(k), k.shape[1], _ptr(v), v.shape[1], _optptr(decay),
                                         decay.shape[1] if decay is not None else 0, B, nq, nk, heads, dh, int(exact),
                                         variant.encode(), _ptr(out), out.shape[1], C.byref(res)))
        return out, ATTN_VARIANTS[res.value]

    def op_hd_lstm_layer(self, xp, whh, N, H, steps, out=None):
        """The recurrence of one bidirectional LSTM layer of the HDemucs BLSTM (asx_op_hd_lstm_layer): `steps` launches of
        hd_lstm_step_kernel from zero state.  xp [steps * N, 2, 4H], whh [2, 4H, H]; `out` [steps * N, 2H] is uploaded before the
        launches, default NaN.  Returns (out, final cell state [2, N, H])."""
        xp, whh = _f32(xp), _f32(whh)
        if xp.size != steps * N * 8 * H or whh.size != 8 * H * H:
            raise AsxError(f"op_hd_lstm_layer: xp {xp.shape} / whh {whh.shape} are not [{steps * N}, 2, {4 * H}] / [2, {4 * H}, {H}]")
        out = np.full((steps * N, 2 * H), np.nan, np.float32) if out is None else np.array(out, np.float32, order="C")
        if out.shape != (steps * N, 2 * H):
            raise AsxError(f"op_hd_lstm_layer: out {out.shape} is not [{steps * N}, {2 * H}]")
        c = np.full((2, N, H), np.nan, np.float32)
        self._check(self._lib.asx_op_hd_lstm_layer(self._h, _ptr(xp), _ptr(whh), N, H, steps, _ptr(out), _ptr(c)))
        return out, c

    def op_hd_lstm_frames(self, h, ntot, n_off, rows=None, unframe=False):
        """The framing kernels of the HDemucs BLSTM (asx_op_hd_lstm_frames) on h [B, T, H].  unframe False: hd_lstm_frame_kernel writes
        this group's rows of `rows` [steps * ntot, H] (uploaded first, default NaN); returns (rows, steps, nfr).  unframe True:
        hd_lstm_unframe_kernel adds the stitched rows of `rows` to h; returns (h, steps, nfr)."""
        h = np.array(h, np.float32, order="C")
        B, T, H = h.shape
        steps, nfr = C.c_int32(-1), C.c_int32(-1)
        if rows is None:
            if unframe:
                raise AsxError("op_hd_lstm_frames: unframe needs rows")
            rows = np.full((min(T, 200) * ntot, H), np.nan, np.float32)
        rows = np.array(rows, np.float32, order="C")
        if rows.ndim != 2 or rows.shape != (min(T, 200) * ntot, H):
            raise AsxError(f"op_hd_lstm_frames: rows {rows.shape} is not [{min(T, 200) * ntot}, {H}]")
        self._check(self._lib.asx_op_hd_lstm_frames(self._h, int(unframe), _ptr(h), B, T, H, ntot, n_off, _ptr(rows), C.byref(steps),
                                                    C.byref(nfr)))
        return (h if unframe else rows), steps.value, nfr.value

    def op_vr_lstm(self, xp, whh, W, B, hs, out=None):
        """The recurrence of the VR 5.1 LSTMModule (asx_op_vr_lstm): one vr_lstm_seq_kernel<hs> launch.  xp [W, B, 2, 4 * hs],
        whh [2, 4 * hs, hs]; `out` [W, B, 2 * hs] is uploaded first, default NaN."""
        xp, whh = _f32(xp), _f32(whh)
        if xp.size != W * B * 8 * hs or whh.size != 8 * hs * hs:
            raise AsxError(f"op_vr_lstm: xp {xp.shape} / whh {whh.shape} are not [{W}, {B}, 2, {4 * hs}] / [2, {4 * hs}, {hs}]")
        out = np.full((W, B, 2 * hs), np.nan, np.float32) if out is None else np.array(out, np.float32, order="C")
        if out.shape != (W, B, 2 * hs):
            raise AsxError(f"op_vr_lstm: out {out.shape} is not [{W}, {B}, {2 * hs}]")
        self._check(self._lib.asx_op_vr_lstm(self._h, _ptr(xp), _ptr(whh), W, B, hs, _ptr(out)))
        return out

    def op_vr_lstm_layout(self, src, B, H, W, ld, ch0, dst=None, out=False):
        """The layout kernels of the VR 5.1 LSTMModule (asx_op_vr_lstm_layout).  out False: vr_lstm_in_kernel, channel ch0 of src
        [B, H, W, ld] -> [W, B, H].  out True: vr_lstm_out_kernel, src [W, B, H] -> channels ch0 .. ch0+3 of `dst` [B, H, W, ld]
        (uploaded first, default NaN)."""
        src = _f32(src)
        s_shape, d_shape = ((W, B, H), (B, H, W, ld)) if out else ((B, H, W, ld), (W, B, H))
        if src.shape != s_shape:
            raise AsxError(f"op_vr_lstm_layout: src {src.shape} is not {s_shape}")
        dst = np.full(d_shape, np.nan, np.float32) if dst is None else np.array(dst, np.float32, order="C")
        if dst.shape != d_shape:
            raise AsxError(f"op_vr_lstm_layout: dst {dst.shape} is not {d_shape}")
        self._check(self._lib.asx_op_vr_lstm_layout(self._h, int(out), _ptr(src), B, H, W, ld, ch0, _ptr(dst)))
        return dst

    def op_gconv(self, x, w, b, y, res=None, variant="auto", **desc):
        """One gathered-convolution launch (asx_op_gconv, include/asx.h): `desc` holds the fields of asx_gconv_desc (mode as "dense" /
        "glu" / "convt" or its number; fields left out are 0, taps / dilations / strides default to 1), x / y / res the flat host
        tensors the views live in.  `y` is uploaded before the launch and returned updated.  Returns (y, (kernel name, N tile, lowai))."""
        x, w, b = _f32(x), _f32(w), _f32(b)
        y = np.array(y, np.float32, order="C")
        res = _f32(res) if res is not None else None
        d = _GconvDesc()
        for k in ("KO", "KI", "DO", "DI", "SO", "SI", "So"):
            setattr(d, k, 1)
        for k, v in desc.items():
            if k == "mode" and isinstance(v, str):
                v = GCONV_MODES[v]
            if not hasattr(d, k):
                raise AsxError(f"op_gconv: asx_gconv_desc has no field {k!r}")
            setattr(d, k, int(v))
        d.res = 0 if res is None else 1
        OR = d.OR or d.O
        convt = d.mode == 2
        nx = d.B * (d.x_bs or d.O * d.I * d.ldc)
        ny = d.B * d.O * d.Iout * d.ldy if convt else d.B * (d.y_bs or OR * d.IR * d.ldy)
        nw = (2 * d.So if convt else d.KO * d.KI * (2 if d.mode == 1 else 1)) * d.Cin * d.Cout
        nb = d.Cout * (2 if d.mode == 1 else 1)
        nr = 0 if res is None else (d.res_mod or (d.B * d.O * d.Iout if convt else d.B * OR * d.IR)) * d.ldr
        if x.size != nx or y.size != ny or w.size != nw or b.size != nb or (res is not None and res.size != nr):
            raise AsxError(f"op_gconv: x {x.size} / y {y.size} / w {w.size} / b {b.size} / res {None if res is None else res.size} floats, "
                           f"the descriptor wants {nx} / {ny} / {nw} / {nb} / {nr}")
        ran = (C.c_int32 * 3)(0, 0, 0)
        self._check(self._lib.asx_op_gconv(self._h, C.byref(d), _ptr(x), _ptr(w), _ptr(b), _optptr(res), variant.encode(), _ptr(y), ran))
        return y, (GCONV_VARIANTS[ran[0]] if ran[0] else None, int(ran[1]), int(ran[2]))

    def _stft_desc(self, keep, **kw):
        """asx_stft_desc from keywords (fields left out are 0, sign 1; mode as "chunks" / "song" / "pool" or its number; starts / song_of /
        song_len / n_act as sequences).  `keep` collects the arrays the descriptor points into."""
        d = _StftDesc()
        d.sign = 1.0
        for k, v in kw.items():
            if not hasattr(d, k):
                raise AsxError(f"asx_stft_desc has no field {k!r}")
            if k in ("starts", "song_len", "n_act", "song_of"):
                if v is None:
                    continue
                a = np.ascontiguousarray(v, dtype=np.int32 if k == "song_of" else np.int64)
                keep[k] = a
                setattr(d, k, a.ctypes.data_as(C.POINTER(C.c_int32 if k == "song_of" else C.c_int64)))
            elif k == "sign":
                d.sign = float(v)
            else:
                setattr(d, k, int(STFT_MODES[v] if k == "mode" and isinstance(v, str) else v))
        return d

    def op_stft(self, wave, spec, **desc):
        """One forward STFT launch (asx_op_stft, include/asx.h): `desc` holds the fields of asx_stft_desc (spec_floats is taken from
        `spec`), `wave` the flat host samples the mode asks for.  `spec` is uploaded before the launch and returned updated.
        Returns (spec, (kernel name, seam launches))."""
        wave = _f32(wave).reshape(-1)
        spec = np.array(spec, np.float32, order="C")
        keep = {}
        d = self._stft_desc(keep, spec_floats=spec.size, **desc)
        if d.mode == 0:
            want = d.b * 2 * d.c
        else:
            lens = keep.get("song_len")
            if lens is None or lens.size != (1 if d.mode == 1 else d.n_songs) or "starts" not in keep or keep["starts"].size != d.b or \
                    (d.mode == 2 and ("song_of" not in keep or keep["song_of"].size != d.b)):
                raise AsxError(f"op_stft: mode {d.mode} needs song_len [{1 if d.mode == 1 else d.n_songs}], starts [b]" +
                               (" and song_of [b]" if d.mode == 2 else ""))
            want = 2 * int(lens.sum())
        if wave.size != want:
            raise AsxError(f"op_stft: wave holds {wave.size} floats, the descriptor wants {want}")
        ran = (C.c_int32 * 2)(0, 0)
        self._check(self._lib.asx_op_stft(self._h, C.byref(d), _ptr(wave), _ptr(spec), ran))
        return spec, (STFT_KERNELS[ran[0]], int(ran[1]))

    def op_istft(self, spec, wave, mask=None, **desc):
        """One inverse launch (asx_op_istft: istft_kernel + ola_kernel, or the fused fast path): `spec` the flat host spectrum, `mask`
        [b, n_inst, t, dim_f, 2, 2] for layout 2, `wave` [b * max(n_inst, 1), 2, c] uploaded first and returned updated.
        Returns (wave, (kernel name, seam launches))."""
        spec = _f32(spec).reshape(-1)
        wave = np.array(wave, np.float32, order="C")
        mask = _f32(mask).reshape(-1) if mask is not None else None
        keep = {}
        d = self._stft_desc(keep, spec_floats=spec.size, **desc)
        S = max(d.n_inst, 1)
        if wave.size != d.b * S * 2 * d.c or (mask is not None and mask.size != d.b * S * d.t * self.cfg.dim_f * 4):
            raise AsxError(f"op_istft: wave {wave.size} / mask {None if mask is None else mask.size} floats do not fit the descriptor")
        if "n_act" in keep and keep["n_act"].size != d.b * S:
            raise AsxError("op_istft: n_act needs one entry per output chunk")
        ran = (C.c_int32 * 2)(0, 0)
        self._check(self._lib.asx_op_istft(self._h, C.byref(d), _ptr(spec), _optptr(mask), _ptr(wave), ran))
        return wave, (STFT_KERNELS[ran[0]], int(ran[1]))

    def op_ht_spec(self, nfft, seg, el=0, lv=None, spec=None):
        """One ht_stft_kernel launch (asx_op_ht_spec): seg [B, 2, L] -> [B, T = ceil(L / hop), nfft / 2, 2 (channel), 2 (re, im)];
        el / lv: pad1d's zero extension (default none).  `spec` (default NaN) is uploaded first."""
        seg = _f32(seg)
        B, _, L = seg.shape
        hop = nfft // 4
        shape = (B, -(-L // hop), nfft // 2, 2, 2)
        spec = np.full(shape, np.nan, np.float32) if spec is None else np.array(spec, np.float32, order="C")
        if seg.shape[1] != 2 or spec.shape != shape:
            raise AsxError(f"op_ht_spec: seg {seg.shape} / spec {spec.shape}, expected [B, 2, L] / {shape}")
        self._check(self._lib.asx_op_ht_spec(self._h, int(nfft), _ptr(seg), B, L, int(el), int(L if lv is None else lv), _ptr(spec)))
        return spec

    def op_ht_ispec(self, nfft, x, acc_f, n_stat, xt, acc_t, out=None):
        """ht_istft_kernel + ht_ola_kernel (asx_op_ht_ispec): x [B, T, nfft / 2, 4 S], xt [B, L, 2 S] -> out [B, S, 2, L]; acc_f / acc_t
        [B, 2] float64 (sum, sum of squares) over n_stat spectrogram values / 2 L samples.  `out` (default NaN) is uploaded first."""
        x, xt = _f32(x), _f32(xt)
        B, T, nh, c4 = x.shape
        S, L = c4 // 4, xt.shape[1]
        acc_f = np.ascontiguousarray(acc_f, np.float64)
        acc_t = np.ascontiguousarray(acc_t, np.float64)
        out = np.full((B, S, 2, L), np.nan, np.float32) if out is None else np.array(out, np.float32, order="C")
        if nh != nfft // 2 or c4 != 4 * S or xt.shape != (B, L, 2 * S) or acc_f.shape != (B, 2) or acc_t.shape != (B, 2) or out.shape != (B, S, 2, L):
            raise AsxError(f"op_ht_ispec: x {x.shape} / xt {xt.shape} / acc {acc_f.shape} {acc_t.shape} / out {out.shape} do not fit")
        dp = C.POINTER(C.c_double)
        self._check(self._lib.asx_op_ht_ispec(self._h, int(nfft), _ptr(x), B, T, S, acc_f.ctypes.data_as(dp), float(n_stat), _ptr(xt),
                                              acc_t.ctypes.data_as(dp), L, _ptr(out)))
        return out

    def op_dconv(self, y, p, along_outer, d, part=3, h=None):
        """One DConv layer (asx_op_dconv) on y [B, O, I, C] channels-last; p: dict of the layer's torch tensors w1 [hid, C, 3], b1, g1w,
        g1b [hid], w2 [2C, hid(, 1)], b2, g2w, g2b [2C], ls [C].  part 1 / 2 / 3 = head / tail / both; `h` [B * O * I, hp] is the
        head's output (uploaded first, default NaN) and the tail's input.  Returns (y, h, arrival counters left non-zero)."""
        y = np.array(y, np.float32, order="C")
        B, O, I, Cc = y.shape
        t = {k: _f32(p[k]) for k in ("w1", "b1", "g1w", "g1b", "w2", "b2", "g2w", "g2b", "ls")}
        hid = t["b1"].size
        hp = (hid + 3) & ~3
        if t["w1"].size != hid * Cc * 3 or t["w2"].size != 2 * Cc * hid or t["b2"].size != 2 * Cc or t["g1w"].size != hid or \
                t["g1b"].size != hid or t["g2w"].size != 2 * Cc or t["g2b"].size != 2 * Cc or t["ls"].size != Cc:
            raise AsxError(f"op_dconv: the layer's tensors do not fit C = {Cc}, hid = {hid}")
        if h is None:
            if part == 2:
                raise AsxError("op_dconv: part 2 alone needs h")
            h = np.full((B * O * I, hp), np.nan, np.float32)
        h = np.array(h, np.float32, order="C")
        if h.shape != (B * O * I, hp):
            raise AsxError(f"op_dconv: h {h.shape} is not [{B * O * I}, {hp}]")
        left = C.c_int32(-1)
        self._check(self._lib.asx_op_dconv(self._h, _ptr(y), B, O, I, Cc, hid, int(bool(along_outer)), int(d), int(part), _ptr(t["w1"]),
                                           _ptr(t["b1"]), _ptr(t["g1w"]), _ptr(t["g1b"]), _ptr(t["w2"]), _ptr(t["b2"]), _ptr(t["g2w"]),
                                           _ptr(t["g2b"]), _ptr(t["ls"]), _ptr(h), C.byref(left)))
        return y, h, left.value

    def op_rownorm(self, kind, x, d, gamma=None, beta=None, pos=None, y=None, in_place=False):
        """One row normalisation launch (asx_op_rownorm) over the first d columns of x [M, lda].  "rms": rof_rmsnorm into y [M, ldy]
        (default NaN, uploaded first), or in place on one device buffer holding x; "rms_factor": rof_rownorm -> r [M]; "layer": ht_ln
        with gamma, beta and the optional position table pos [pos_mod, d] read at row % pos_mod (dense rows, lda == d)."""
        x = _f32(x)
        M, lda = x.shape
        if kind == "rms_factor":
            y = np.full(M, np.nan, np.float32) if y is None else np.array(y, np.float32, order="C")
            ldy, want = 0, (M,)
        else:
            y = np.full((M, lda if in_place else d), np.nan, np.float32) if y is None else np.array(y, np.float32, order="C")
            ldy, want = (y.shape[1] if y.ndim == 2 else -1), (M, y.shape[-1])
        gamma, beta, pos = (None if a is None else _f32(a) for a in (gamma, beta, pos))
        if y.shape != want or any(a is not None and a.size != d for a in (gamma, beta)) or (pos is not None and (pos.ndim != 2 or pos.shape[1] != d)):
            raise AsxError(f"op_rownorm: x {x.shape} / y {y.shape} / gamma, beta, pos do not fit d = {d}")
        self._check(self._lib.asx_op_rownorm(self._h, kind.encode(), _ptr(x), M, int(d), lda, _optptr(gamma), _optptr(beta), _optptr(pos),
                                             0 if pos is None else pos.shape[0], int(bool(in_place)), _ptr(y), ldy))
        return y

    def op_group_stats(self, x, gdiv, ld, cn, g2):
        """One ht_stats launch (asx_op_group_stats) over x [G1, R, P]: the float64 (sum, sum of squares) pairs [G1, g2, 2] of the groups
        of gdiv consecutive plane elements, counting the first cn of every ld."""
        x = _f32(x)
        G1, R, P = x.shape
        acc = np.full((G1, int(g2), 2), np.nan, np.float64)
        self._check(self._lib.asx_op_group_stats(self._h, _ptr(x), G1, R, P, int(gdiv), int(ld), int(cn), int(g2),
                                                 acc.ctypes.data_as(C.POINTER(C.c_double))))
        return acc

    def op_group_norm(self, family, x, gamma=None, beta=None, aux=None, mul=None, y=None, stats=None, **desc):
        """Statistics + apply of one normalisation as the nets launch it (asx_op_group_norm, include/asx.h): `desc` holds the fields of
        asx_group_norm_desc the family reads (mode as "gelu" / "glu" / "none", norm as in the model's config, act by name); b and the
        sizes the shape of x gives are taken from x.  y (default NaN) and stats are uploaded first.  Returns y, or (y, stats) for "v3"."""
        x = _f32(x)
        d = _GroupNormDesc()
        for k, v in desc.items():
            if k == "mode":
                v = HD_GN_MODES[v] if isinstance(v, str) else v
            elif k == "norm":
                v = v if isinstance(v, int) else v3_norm_code(v)
            elif k == "act":
                v = V3_ACTS[v] if isinstance(v, str) else v
            setattr(d, k, float(v) if k == "alpha" else int(v))
        d.b = x.shape[0]
        if family in ("ht", "std"):
            _, d.r, d.c = x.shape
            shape = x.shape
        elif family in ("time", "hd_time"):
            d.p = x.shape[2]
            shape = (d.b, (d.p + 1) // 2 * 2 if family == "hd_time" else d.p, 2)
        elif family == "hd":
            d.c = x.shape[2]
            if not d.r:
                d.r = x.shape[1]
            d.rin = x.shape[1]
            shape = (d.b, d.r, d.c // 2 if d.mode == 1 else d.c)
        elif family == "v3":
            _, d.ctot, d.p = x.shape
            if not d.c:
                d.c = d.ctot
            shape = (d.b, d.c, d.p)
        elif family == "mdx":
            _, d.c, d.p = x.shape
            shape = x.shape
        else:
            raise AsxError(f"op_group_norm: unknown family {family!r}")
        gamma, beta, aux, mul = (None if a is None else _f32(a) for a in (gamma, beta, aux, mul))
        y = np.full(shape, np.nan, np.float32) if y is None else np.array(y, np.float32, order="C")
        if family == "v3":
            stats = np.full((d.b, d.c, 2), np.nan, np.float32) if stats is None else np.array(stats, np.float32, order="C")
        else:
            stats = None
        if y.shape != tuple(shape) or any(a is not None and a.shape != y.shape for a in (aux, mul)) or \
                any(a is not None and a.size != d.c for a in (gamma, beta)) or (stats is not None and stats.shape != (d.b, d.c, 2)):
            raise AsxError(f"op_group_norm({family}): x {x.shape} / y {y.shape} / the other tensors do not fit")
        self._check(self._lib.asx_op_group_norm(self._h, family.encode(), C.byref(d), _ptr(x), _optptr(gamma), _optptr(beta), _optptr(aux),
                                                _optptr(mul), _ptr(y), _optptr(stats)))
        return (y, stats) if family == "v3" else y

    # -- profiling --------------------------------------------------------------
    def profile_enable(self, on: bool = True):
        self._check(self._lib.asx_profile_enable(self._h, int(on)))

    def profile_launches(self):
        """Per-launch records of the current profile: [(class name, ms, flops, bytes)] in launch order."""
        n = C.c_int32()
        self._check(self._lib.asx_profile_launches(self._h, None, 0, C.byref(n)))
        recs = (_LaunchRec * max(1, n.value))()
        self._check(self._lib.asx_profile_launches(self._h, recs, n.value, C.byref(n)))
        return [(PROF_CLASSES[r.cls & 0xff], float(r.ms), float(r.flops), float(r.bytes)) for r in recs[: n.value]]

    def profile_launches_ex(self):
        """As profile_launches with a fifth field: the 16-bit MFMA products per multiply-add the launch executed -- 6 (bf16 x 6), 3 (fp16 x 3)
        or 0 (fp32 MFMA / VALU kernels) -- bits 8..15 of asx_launch_rec.cls (ABI 7)."""
        n = C.c_int32()
        self._check(self._lib.asx_profile_launches(self._h, None, 0, C.byref(n)))
        recs = (_LaunchRec * max(1, n.value))()
        self._check(self._lib.asx_profile_launches(self._h, recs, n.value, C.byref(n)))
        return [(PROF_CLASSES[r.cls & 0xff], float(r.ms), float(r.flops), float(r.bytes), (r.cls >> 8) & 0xff) for r in recs[: n.value]]

    def profile_read(self) -> dict:
        p = _Profile()
        self._check(self._lib.asx_profile_read(self._h, C.byref(p)))
        return {name: {"launches": int(p.launches[i]), "ms": float(p.ms[i]), "flops": float(p.flops[i]),
                       "bytes": float(p.bytes[i])} for i, name in enumerate(PROF_CLASSES)}
