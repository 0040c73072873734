#!/usr/bin/env python3
"""The accuracy yardstick of the single-product arithmetic (engine option "gemm_f16x1", plugin knob asx_autocast) from the REFERENCE classes
(build container only): how far the reference's own reduced-precision mode -- `torch.autocast(dtype=torch.float16)`, what its
`Separator(use_autocast=True)` wraps `separate()` in -- moves BSRoformer / MelBandRoformer away from their fp32 forward, on the CPU, on the
seeded weights and inputs of make_golden_roformer.py / make_golden_melroformer.py.  Writes tests/golden/autocast_yardstick.json (data only):
per configuration r_ref = rel_rms(autocast forward, fp32 forward).  tests/test_gpu_roformer_autocast.py holds the engine's
rel_rms(option on, option off) to it.

Absent third-party deps are stubbed as in make_golden_melroformer.py.

    python tests/golden/make_golden_autocast.py
"""
import importlib.machinery
import json
import os
import sys
import types
import typing

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"


class ConfigDict(dict):
    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = ConfigDict(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def main():
    sys.path.insert(0, ROOT)
    from oracle import roformer_oracle as R
    for name in ["onnx", "onnxruntime", "onnx2torch", "soundfile", "audioread"]:
        _stub(name)
    filt = _stub("librosa.filters", mel=lambda sr, n_fft, n_mels: R.mel_filter_stub(sr, n_fft, n_mels))
    _stub("librosa", filters=filt)
    _stub("pydub", AudioSegment=object)
    _stub("ml_collections", ConfigDict=ConfigDict)
    _stub("beartype", beartype=lambda f: f)
    _stub("beartype.typing", Tuple=typing.Tuple, Optional=typing.Optional, List=typing.List, Callable=typing.Callable)
    _stub("rotary_embedding_torch", RotaryEmbedding=R.RotaryEmbedding)
    for name, path in [("audio_separator", REF + "/audio_separator"), ("audio_separator.separator", REF + "/audio_separator/separator")]:
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        pkg.__spec__ = importlib.machinery.ModuleSpec(name, None, is_package=True)
        sys.modules[name] = pkg
    from audio_separator.separator.uvr_lib_v5.roformer.bs_roformer import BSRoformer
    from audio_separator.separator.uvr_lib_v5.roformer.mel_band_roformer import MelBandRoformer

    bs = R.RoformerConfig(dim=32, depth=2, heads=2, dim_head=64, freqs_per_bands=(2, 2, 4, 8, 17), stft_n_fft=64,
                          stft_hop_length=16, stft_win_length=64, dim_t=21, sample_rate=100, mlp_expansion_factor=2)
    mel = R.RoformerConfig.mel_config(dim=32, depth=2, heads=2, dim_head=64, num_bands=6, stft_n_fft=64, stft_hop_length=16,
                                      stft_win_length=64, dim_t=21, sample_rate=100, mlp_expansion_factor=2)
    golden = {"bs_roformer": np.load(os.path.join(HERE, "roformer_small.npz"))["fwd1"],
              "mel_band_roformer": np.load(os.path.join(HERE, "melroformer_small.npz"))["fwd1"]}
    out = {"what": "rel_rms(reference forward under torch.autocast('cpu', dtype=torch.float16), reference fp32 forward)", "torch": torch.__version__,
           "configs": {}}
    for key, cls, cfg, seed, wseed in (("bs_roformer", BSRoformer, bs, 7, 81), ("mel_band_roformer", MelBandRoformer, mel, 17, 181)):
        net = cls(**cfg.model_kwargs(), flash_attn=False)
        net.load_state_dict(R.make_roformer_state(cfg, seed), strict=True)
        net.eval()
        w = torch.tensor((0.4 * np.random.default_rng(wseed).standard_normal((2, 2, 320))).astype(np.float32))
        with torch.no_grad():
            y32 = net(w).float().numpy()
            with torch.autocast("cpu", dtype=torch.float16):
                y16 = net(w).float().numpy()
        assert np.array_equal(y32, golden[key]) or rel_rms(y32, golden[key]) < 1e-6, "the fp32 forward is not the committed golden's"
        assert np.isfinite(y16).all()
        out["configs"][key] = {"weights_seed": seed, "input_seed": wseed, "r_ref": rel_rms(y16, y32)}
        print(key, out["configs"][key])
    with open(os.path.join(HERE, "autocast_yardstick.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
