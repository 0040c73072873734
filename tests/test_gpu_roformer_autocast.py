"""The Roformer forward and the MDXC plugin on the single-product arithmetic (engine option "gemm_f16x1", ``common_config["asx_autocast"]``):
which kernels a forward launches, how far the option moves the result -- held to the reference's own autocast run, measured on the CPU by
tests/golden/make_golden_autocast.py -- and the knob's three values at file level."""
import filecmp
import json
import os

import numpy as np
import pytest

from oracle import roformer_oracle as R
from tests import separate_cases as SC

pytestmark = pytest.mark.gpu

# the tiny configurations of tests/test_gpu_roformer.py (and their golden seeds)
BS = R.RoformerConfig(dim=32, depth=2, heads=2, dim_head=64, freqs_per_bands=(2, 2, 4, 8, 17), stft_n_fft=64,
                      stft_hop_length=16, stft_win_length=64, dim_t=21, sample_rate=100, mlp_expansion_factor=2)
MEL = R.RoformerConfig.mel_config(dim=32, depth=2, heads=2, dim_head=64, num_bands=6, stft_n_fft=64, stft_hop_length=16,
                                  stft_win_length=64, dim_t=21, sample_rate=100, mlp_expansion_factor=2)
CONFIGS = {"bs_roformer": (BS, 7, 81), "mel_band_roformer": (MEL, 17, 181)}
COUNTERS = ("tdf3_launches", "tdf3h_launches", "tdf3s_launches", "attn6_launches", "attn6h_launches", "attn6s_launches")


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-30))


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


@pytest.fixture(scope="module")
def yardstick(golden_dir):
    with open(os.path.join(golden_dir, "autocast_yardstick.json")) as fh:
        return json.load(fh)["configs"]


def demixer(A, cfg, seed, **common):
    return A.MDXCDemixer({"model_data": cfg.as_model_data(), "torch_device": 0, "secondary_stem_name": cfg.instruments[1], **common},
                         {"overlap": 8}, state_dict=R.make_roformer_state(cfg, seed))


def counted(eng, fn):
    c0 = [eng.counter(k) for k in COUNTERS]
    y = fn()
    return y, dict(zip(COUNTERS, (eng.counter(k) - b for k, b in zip(COUNTERS, c0))))


@pytest.mark.parametrize("key", list(CONFIGS))
def test_forward_counters_and_yardstick(A, yardstick, key):
    """One rof_forward.  Option on: every launch of the split-operand row GEMM and of the attention is a single-product one (the rise of tdf3s equals
    that of tdf3h, attn6s that of attn6h).  Option off: neither counter moves and the output is an untouched engine's, bit for bit.
    r_dev = rel_rms(on, off) <= r_ref, the reference's own rel_rms(autocast, fp32) on the same weights and input, margin 1: the engine keeps
    activations, norms and softmax in fp32 where autocast stores fp16, so it must not be further from fp32 than the reference's mode; and
    r_dev >= 100 x rel_rms(off, off again) -- the option does something (two runs are bit-identical: the floor is 0, and r_dev > 0 is asked)."""
    cfg, seed, wseed = CONFIGS[key]
    w = (0.4 * np.random.default_rng(wseed).standard_normal((2, 2, 320))).astype(np.float32)
    eng = demixer(A, cfg, seed).engine
    untouched = demixer(A, cfg, seed).engine.rof_forward(w)
    assert eng.option("gemm_f16x1") == 0
    y_off, n_off = counted(eng, lambda: eng.rof_forward(w))
    assert n_off["tdf3s_launches"] == 0 and n_off["attn6s_launches"] == 0, n_off
    assert n_off["tdf3h_launches"] > 0 and n_off["attn6h_launches"] > 0, n_off
    assert np.array_equal(y_off, untouched), "option off: not the bits of an untouched engine"
    eng.set_option("gemm_f16x1", 1)
    y_on, n_on = counted(eng, lambda: eng.rof_forward(w))
    assert n_on["tdf3s_launches"] == n_on["tdf3h_launches"] == n_off["tdf3h_launches"], (n_on, n_off)
    assert n_on["attn6s_launches"] == n_on["attn6h_launches"] == n_off["attn6h_launches"], (n_on, n_off)
    assert n_on["tdf3_launches"] == n_off["tdf3_launches"] and n_on["attn6_launches"] == n_off["attn6_launches"]
    assert np.array_equal(y_on, eng.rof_forward(w)), "two single-product forwards differ"
    eng.set_option("gemm_f16x1", 0)
    y_off2, n_off2 = counted(eng, lambda: eng.rof_forward(w))
    assert n_off2["tdf3s_launches"] == 0 and n_off2["attn6s_launches"] == 0
    assert np.array_equal(y_off2, y_off), "option back to 0: not the fp32-grade bits"
    r_ref = yardstick[key]["r_ref"]
    r_dev, floor = rel_rms(y_on, y_off), rel_rms(y_off2, y_off)
    print(f"{key}: r_dev = rel_rms(gemm_f16x1 on, off) = {r_dev:.4e}; r_ref = rel_rms(reference autocast fp16, fp32) = {r_ref:.4e}; off vs off again {floor:.1e}")
    assert np.isfinite(y_on).all()
    assert r_dev <= r_ref, (r_dev, r_ref)
    assert r_dev > 0 and r_dev >= 100 * floor, (r_dev, floor)


# ---- file level, through MDXCSeparator ------------------------------------------------------------------------------------------------
def plugin(tmp, out_dir, **common_over):
    _, cls, common, arch, wav, _ = SC.cases("roformer", str(tmp))[0]
    return SC.plugin_class(cls)(common_config=dict(common, output_dir=str(out_dir), **common_over), arch_config=dict(arch)), wav


def blobs(out_dir, names):
    assert names
    return [open(os.path.join(str(out_dir), os.path.basename(n)), "rb").read() for n in names]


@pytest.fixture()
def file_env(monkeypatch):
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")


def test_off_ignores_an_ambient_autocast(tmp_path, file_env):
    import torch
    inst, wav = plugin(tmp_path, tmp_path / "plain")
    assert inst.asx_autocast == "off"
    want = blobs(tmp_path / "plain", inst.separate(wav, None))
    assert inst.last_arithmetic == "fp16x3"
    inst.output_dir = str(tmp_path / "ambient")
    with torch.autocast("cuda", dtype=torch.float16):
        assert torch.is_autocast_enabled("cuda")
        got = blobs(tmp_path / "ambient", inst.separate(wav, None))
    assert inst.last_arithmetic == "fp16x3" and inst.engine.option("gemm_f16x1") == 0
    assert got == want, "asx_autocast='off' inside torch.autocast: not the bytes of 'off' outside it"
    inst.clear_gpu_cache()


def test_follow_and_fp16(tmp_path, file_env):
    """"follow" = "fp16" inside torch.autocast("cuda") and "off" outside it, on ONE instance, in that order and reversed; "fp16" through
    separate, separate_many([p, p]) and stems_dev + write_audio gives the same bytes; last_arithmetic says what ran."""
    import torch
    off, wav = plugin(tmp_path, tmp_path / "off")
    b_off = blobs(tmp_path / "off", off.separate(wav, None))
    off.clear_gpu_cache()
    fp16, _ = plugin(tmp_path, tmp_path / "fp16", asx_autocast="fp16")
    s0 = fp16._demixer().engine.counter("tdf3s_launches")
    names = fp16.separate(wav, None)
    b_fp16 = blobs(tmp_path / "fp16", names)
    assert fp16.last_arithmetic == "fp16x1" and fp16._demixer().engine.counter("tdf3s_launches") > s0
    assert b_fp16 != b_off, "the single-product arithmetic wrote the fp32-grade bytes"
    # separate_many([p, p])
    fp16.output_dir = str(tmp_path / "fp16_many")
    many = fp16.separate_many([wav, wav])
    assert len(many) == 2 and not fp16.batch_errors and fp16.last_arithmetic == "fp16x1"
    assert blobs(tmp_path / "fp16_many", many[0]) == b_fp16 and blobs(tmp_path / "fp16_many", many[1]) == b_fp16
    # stems_dev + write_audio
    fp16.output_dir = str(tmp_path / "fp16_stems")
    os.makedirs(fp16.output_dir, exist_ok=True)
    stems = fp16.stems_dev(wav)
    assert fp16.last_arithmetic == "fp16x1"
    written = []
    for name, t, layout in stems:
        assert layout == "planar"
        path = fp16.get_stem_output_path(name, None)
        fp16.write_audio(path, np.ascontiguousarray(t.cpu().numpy().T))
        written.append(path)
    assert sorted(os.path.basename(p) for p in written) == sorted(os.path.basename(n) for n in names)
    assert sorted(blobs(tmp_path / "fp16_stems", written)) == sorted(b_fp16)
    fp16.clear_gpu_cache()
    # follow: outside, inside, outside again -- and on a fresh instance inside first
    for order in (("out", "in", "out"), ("in", "out", "in")):
        inst, _ = plugin(tmp_path, tmp_path / "follow", asx_autocast="follow")
        for i, where in enumerate(order):
            inst.output_dir = str(tmp_path / f"follow_{'_'.join(order)}_{i}")
            if where == "in":
                with torch.autocast("cuda", dtype=torch.float16):
                    got = blobs(inst.output_dir, inst.separate(wav, None))
                assert got == b_fp16 and inst.last_arithmetic == "fp16x1" and inst.engine.option("gemm_f16x1") == 1, (order, i)
            else:
                got = blobs(inst.output_dir, inst.separate(wav, None))
                assert got == b_off and inst.last_arithmetic == "fp16x3" and inst.engine.option("gemm_f16x1") == 0, (order, i)
        inst.clear_gpu_cache()


def test_ensemble_of_an_fp16_and_an_off_member(A, tmp_path, file_env):
    """each member sets its own engine: the device path gives the bytes of via_files=True"""
    first, wav = plugin(tmp_path, tmp_path / "m", asx_autocast="fp16")
    second, _ = plugin(tmp_path, tmp_path / "m", model_name="model_bs_roformer_small_b")
    members = [first, second]
    by_files = A.EnsembleSeparator(members, "avg_wave", None, via_files=True)
    by_files.output_dir = str(tmp_path / "files")
    want = by_files.separate(wav, None)
    assert by_files.last_path_taken == "files" and len(want) == 2
    assert first.engine.option("gemm_f16x1") == 1 and second.engine.option("gemm_f16x1") == 0
    on_device = A.EnsembleSeparator(members, "avg_wave", None)
    on_device.output_dir = str(tmp_path / "device")
    got = on_device.separate(wav, None)
    assert on_device.last_path_taken == "device"
    assert [os.path.basename(f) for f in got] == [os.path.basename(f) for f in want]
    for a, b in zip(got, want):
        assert os.path.isfile(a) and filecmp.cmp(a, b, shallow=False), os.path.basename(a)
    for m in members:
        m.clear_gpu_cache()
