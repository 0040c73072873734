"""``common_config["asx_complement_rate"]`` without a GPU:

* the knob's validation and the refusals (an unknown value, "input" without ``asx_output_rate="input"``, MDX with ``invert_using_spec``,
  DemucsSeparator, VRSeparator), each naming its reason;
* the float32 restatement of the complement (tests/complement_ref.py), the yardstick of the GPU tests, against a float64 evaluation
  within 6 * 2^-24 on random data of the magnitudes the bound is worked out for;
* the host-array route of the plugins on the oracle-backed engine double (tests/fake_engine.py) extended by the float64 definition of the
  converter (tests/resample_ref.py): which stem is written from what, the per-file state, ``separate_many`` against the loop, and a
  file that the host decoder converts (``asx_input_resample`` = "host"): its own mix is kept too, or the plugin warns once per file."""
import logging
import math
import os

import numpy as np
import pytest

import audio_separator_amd as A
from audio_separator_amd import audio_io
from tests import complement_ref as CR
from tests import fake_engine
from tests import resample_ref as RR
from tests import separate_cases as SC

ON = dict(asx_input_resample="device", asx_output_rate="input", asx_complement_rate="input")
OFF = dict(asx_input_resample="device", asx_output_rate="input")


def common(tmp_path, **over):
    return SC.common_config("m", "/m/model.onnx", {"primary_stem": "Vocals"}, str(tmp_path / "out"), **over)


def test_setting_default_and_validation(tmp_path, monkeypatch):
    assert A.CommonSeparator.COMPLEMENT_RATE_MODES == ("model", "input")
    assert A.CommonSeparator(common(tmp_path)).asx_complement_rate == "model"
    assert A.CommonSeparator(common(tmp_path, asx_complement_rate="model")).asx_complement_rate == "model"
    assert A.CommonSeparator(common(tmp_path, asx_output_rate="input", asx_complement_rate="model")).asx_complement_rate == "model"
    assert A.CommonSeparator(common(tmp_path, asx_output_rate="input", asx_complement_rate="input")).asx_complement_rate == "input"
    for bad in ("gpu", "file", "48000"):
        with pytest.raises(ValueError, match=r"asx_complement_rate must be one of \('model', 'input'\)"):
            A.CommonSeparator(common(tmp_path, asx_output_rate="input", asx_complement_rate=bad))
    for over in ({}, {"asx_output_rate": "model"}):
        with pytest.raises(ValueError, match="asx_complement_rate='input' requires asx_output_rate='input'"):
            A.CommonSeparator(common(tmp_path, asx_complement_rate="input", **over))
    monkeypatch.setenv("ASX_COMPLEMENT_RATE", "input")                   # no environment override
    assert A.CommonSeparator(common(tmp_path, asx_output_rate="input")).asx_complement_rate == "model"
    assert {"_file_mix", "_mix_scale"} <= set(A.CommonSeparator._PER_FILE)


def test_plugins_without_a_difference_stem_refuse(tmp_path, monkeypatch):
    from audio_separator_amd.architectures.demucs_separator import DemucsSeparator
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    fake_engine.install(monkeypatch)
    mdx = SC.cases("mdx", str(tmp_path))[0]
    with pytest.raises(ValueError, match="asx_complement_rate='input' is not supported with invert_using_spec.*spectral inversion"):
        SC.plugin_class("MDXSeparator")(common_config=dict(mdx[2], invert_using_spec=True, **ON), arch_config=mdx[3])
    SC.plugin_class("MDXSeparator")(common_config=dict(mdx[2], invert_using_spec=True, **OFF), arch_config=mdx[3])
    SC.plugin_class("MDXSeparator")(common_config=dict(mdx[2], **ON), arch_config=mdx[3])
    demucs = SC.common_config("htd", "/m/htd.yaml", {}, str(tmp_path / "out"), sample_rate=8000, **ON)
    with pytest.raises(ValueError, match="asx_complement_rate='input' is not supported by DemucsSeparator: every stem is an output of the model"):
        DemucsSeparator(common_config=demucs, arch_config={})
    assert DemucsSeparator._complement_rate_mode({"asx_complement_rate": "model"}) == "model"
    vr = SC.common_config("m", "/m/model.pth", {"vr_model_param": "4band_v3"}, str(tmp_path / "out"), asx_complement_rate="input")
    with pytest.raises(ValueError, match="asx_complement_rate='input' is not supported by VRSeparator: .*refuses asx_output_rate='input'"):
        VRSeparator(common_config=vr, arch_config={})
    with pytest.raises(ValueError, match="is not supported by VRSeparator"):
        VRSeparator(common_config=dict(vr, asx_output_rate="input"), arch_config={})


def test_float32_restatement_against_float64():
    """The yardstick of the GPU tests: three float32 roundings on |s mix| <= 1, |k y| <= 1.65 and a difference <= 2.65."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for s, k in [(1.0, 1.0), (0.8125, 1.035), (float(np.float32(0.9 / 1.37)), 1.0), (1.0, 1.1)]:
        mix = rng.uniform(-1.0, 1.0, (2, 200_000)).astype(np.float32)
        y = rng.uniform(-1.5, 1.5, (2, 200_000)).astype(np.float32)
        y[:, ::7] = np.float32(1.5) * np.sign(y[:, ::7])                  # the extremes the bound is worked out for
        mix[:, ::14] = -np.sign(y[:, ::14])
        c = CR.complement_f32(mix, y, s, k)
        assert c.dtype == np.float32
        err = float(np.abs(c.astype(np.float64) - CR.complement_f64(mix, y, s, k)).max())
        worst = max(worst, err)
        assert err <= CR.ROUNDING_BOUND, (s, k, err)
    assert CR.ROUNDING_BOUND == 6.0 * 2.0 ** -24
    print(f"float32 restatement: max error {worst:.3e} of {CR.ROUNDING_BOUND:.3e}")
    # no fused multiply-add: a case where fl(a - fl(k y)) and the exactly rounded a - k y differ
    a, yv, kv = np.float32(1.0), np.float32(1.0 + 2.0 ** -23), np.float32(1.0 + 2.0 ** -23)
    assert CR.complement_f32(np.array([a]), np.array([yv]), 1.0, kv)[0] == np.float32(a - np.float32(kv * yv))


# ---- the plugins' host-array route on an engine double ------------------------------------------------------------------------------
class ConverterEngine(fake_engine.OracleEngine):
    """The oracle-backed double plus the rational converter by its float64 definition, rounded to float32"""
    complement_calls = []

    @staticmethod
    def resample_rational_plan(sr_in, sr_out, n_in=1):
        if sr_in == sr_out:
            raise A.AsxError("equal rates")
        L, M, _, T, _ = RR.design(sr_in, sr_out)
        return RR.plan_n_out(n_in, L, M), L, M, T

    def mdxc_demix_batch(self, mixes, overlap):
        return [self.mdxc_demix(m, overlap) for m in mixes]

    def resample_rational(self, x, sr_in, sr_out):
        return RR.reference(x, sr_in, sr_out).astype(np.float32)

    def resample_rational_stem(self, x, sr_in, sr_out, n_out, layout="planar"):
        return RR.reference(x, sr_in, sr_out, n_out, layout).astype(np.float32)

    def resample_rational_complement(self, x, sr_in, sr_out, n_out, mix, mix_scale=1.0, stem_scale=1.0, layout="planar", want_stem=True):
        type(self).complement_calls.append((np.asarray(x).shape, sr_in, sr_out, n_out, np.asarray(mix).shape, mix_scale, stem_scale, layout, want_stem))
        y = self.resample_rational_stem(x, sr_in, sr_out, n_out, layout)
        c = CR.complement_f32(np.ascontiguousarray(np.asarray(mix, np.float32)[:, :n_out]), y, mix_scale, stem_scale)
        return (y if want_stem else None), c


def install(monkeypatch):
    fake_engine.install(monkeypatch)
    from audio_separator_amd import mdx, mdxc
    for mod in (mdx, mdxc):
        monkeypatch.setattr(mod, "Engine", ConverterEngine)
    ConverterEngine.complement_calls = []


def case_by_tag(tag, tmp, **over):
    for family in ("mdx", "mdxc"):
        for case in SC.cases(family, str(tmp)):
            if case[0] == tag:
                return (case[0], case[1], dict(case[2], **over), case[3], case[4], case[5])
    raise KeyError(tag)


def write_input(case, tmp, rate, gain, name=None):
    x, model_rate = audio_io.read_wav(case[4])
    reps = int(math.ceil(rate / model_rate))
    x = np.concatenate([x if r % 2 == 0 else x[:, ::-1] for r in range(reps)], axis=1).astype(np.float64) * gain
    x += 0.05 * np.sin(2.0 * np.pi * 0.47 * np.arange(x.shape[1]))
    d = os.path.join(str(tmp), f"in_{rate}_{gain:g}")
    os.makedirs(d, exist_ok=True)
    path = os.path.join(d, name or os.path.basename(case[4]))
    audio_io.write_wav(path, np.ascontiguousarray(x.T.astype(np.float32)), rate, "FLOAT")
    return path


def run(case, wav, sub, **over):
    _, cls, cfg, arch, _, _ = case
    out_dir = os.path.join(cfg["output_dir"], sub)
    inst = SC.plugin_class(cls)(common_config=dict(cfg, output_dir=out_dir, **over), arch_config=arch)
    calls, real = [], inst.write_audio

    def write_audio(stem_path, stem_source):
        calls.append((stem_path, np.array(stem_source, copy=True)))
        real(stem_path, stem_source)
    inst.write_audio = write_audio
    names = inst.separate(wav, None)
    assert inst._file_mix is None and inst._complement is None
    blobs = []
    for n in names:
        with open(os.path.join(out_dir, n), "rb") as f:
            blobs.append(f.read())
    return inst, names, calls, blobs


@pytest.mark.parametrize("tag,gain", [("mdx_plain", 0.5), ("mdx_plain", 1.5), ("mdxc_one", 0.5), ("mdxc_one", 1.5)])
def test_host_route_writes_the_complement_from_the_files_mix(tmp_path, monkeypatch, tag, gain):
    install(monkeypatch)
    case = case_by_tag(tag, tmp_path, use_soundfile=True)
    wav = write_input(case, tmp_path, 48000, gain)
    F = audio_io.wav_info(wav)["frames"]
    _, names_off, calls_off, blobs_off = run(case, wav, "off", **OFF)
    assert ConverterEngine.complement_calls == []
    inst, names, calls, blobs = run(case, wav, "on", **ON)
    assert names == names_off and len(names) == 2
    for (p, a), (q, b) in zip(calls, calls_off):                       # what write_audio is handed stays at the model's rate
        assert p == q and np.array_equal(a, b)
    assert blobs[1] == blobs_off[1] and blobs[0] != blobs_off[0]
    mdx = case[1] == "MDXSeparator"
    k = case[2]["model_data"]["compensate"] if mdx else 1.0
    # one fused call for the pair, at the complement (written first), against the file's [2, F] mix
    mix_f, rate = audio_io.read_wav(wav)
    eng = inst.engine
    peak = np.abs(eng.resample_rational(mix_f, rate, 44100)).max()
    s = float(np.float32(0.9) / peak) if peak > np.float32(0.9) else 1.0
    assert (s < 1.0) == (gain == 1.5)
    n = calls[1][1].shape[0]
    assert ConverterEngine.complement_calls == [((n, 2), 44100, 48000, F, (2, F), s, float(k), "rows", True)]
    y, c = eng.resample_rational_complement(calls[1][1], 44100, 48000, F, mix_f, s, k, layout="rows")
    if not mdx:
        c = eng.normalize(c, 0.9, 0.0)
    for stem, blob in ((c, blobs[0]), (y, blobs[1])):
        path = str(tmp_path / "composed.wav")
        audio_io.write_wav(path, eng.normalize(np.ascontiguousarray(stem.T), 0.9, 0.0), 48000, "FLOAT")
        with open(path, "rb") as f:
            assert f.read() == blob
    if gain == 0.5 and max(np.abs(y).max(), np.abs(c).max()) < 0.9:    # the null test, where no normalise engages
        got_c, _ = audio_io.read_wav(os.path.join(case[2]["output_dir"], "on", names[0]))
        got_p, _ = audio_io.read_wav(os.path.join(case[2]["output_dir"], "on", names[1]))
        miss = np.abs(float(np.float32(k)) * got_p.astype(np.float64) + got_c - mix_f.astype(np.float64)).max()
        assert miss <= CR.ROUNDING_BOUND, miss
        off_c, _ = audio_io.read_wav(os.path.join(case[2]["output_dir"], "off", names[0]))
        assert np.abs(float(np.float32(k)) * got_p.astype(np.float64) + off_c - mix_f.astype(np.float64)).max() > 0.02


def test_only_the_wanted_stem_is_computed_or_kept(tmp_path, monkeypatch):
    install(monkeypatch)
    # the model stem alone: nothing is kept, no fused call
    case = case_by_tag("mdx_plain", tmp_path, output_single_stem="Vocals")
    wav = write_input(case, tmp_path, 48000, 0.5)
    _, names, _, blobs = run(case, wav, "voc_on", **ON)
    _, names_off, _, blobs_off = run(case, wav, "voc_off", **OFF)
    assert ConverterEngine.complement_calls == [] and names == names_off and blobs == blobs_off and len(names) == 1
    # the complement alone: the fused call stores no converted model stem; the file is the one of the two-stem run
    _, both_names, _, both = run(case_by_tag("mdx_plain", tmp_path), wav, "both", **ON)
    ConverterEngine.complement_calls = []
    _, names, _, blobs = run(case_by_tag("mdx_plain", tmp_path, output_single_stem="Instrumental"), wav, "inst_on", **ON)
    assert [c[-1] for c in ConverterEngine.complement_calls] == [False]
    assert names == both_names[:1] and blobs == both[:1]


def test_a_model_without_a_residual_row_says_so_once(tmp_path, monkeypatch, caplog):
    install(monkeypatch)
    logger = logging.getLogger("asx_complement_rate_host_test")
    case = case_by_tag("mdxc_two", tmp_path, logger=logger)
    wav = write_input(case, tmp_path, 48000, 0.5)
    _, cls, cfg, arch, _, _ = case
    inst = SC.plugin_class(cls)(common_config=dict(cfg, output_dir=os.path.join(cfg["output_dir"], "two"), **ON), arch_config=arch)
    with caplog.at_level(logging.INFO, logger="asx_complement_rate_host_test"):
        first = inst.separate(wav, None)
        second = inst.separate(wav, None)
    notes = [r for r in caplog.records if "asx_complement_rate='input' does nothing" in r.getMessage()]
    assert len(notes) == 1 and first == second and inst._file_mix is None and ConverterEngine.complement_calls == []


def test_separate_many_restores_each_files_mix_and_factor(tmp_path, monkeypatch):
    """MDXC: its pooled call has a host-array form (MDX always pools on the device: tests/test_gpu_complement_rate.py)"""
    install(monkeypatch)
    case = case_by_tag("mdxc_one", tmp_path)
    _, cls, cfg, arch, _, _ = case
    files = [write_input(case, tmp_path, rate, gain, name=f"song{rate}.wav") for rate, gain in ((44100, 0.5), (48000, 1.5), (96000, 0.5))]

    def go(sub, many):
        out_dir = os.path.join(cfg["output_dir"], sub)
        inst = SC.plugin_class(cls)(common_config=dict(cfg, output_dir=out_dir, **ON), arch_config=arch)
        ConverterEngine.complement_calls = []
        if many:
            results = inst.separate_many(files)
            assert inst.batch_errors == {}, inst.batch_errors
        else:
            results = [inst.separate(f, None) for f in files]
        assert inst._file_mix is None and inst._complement is None
        blobs = []
        for names in results:
            assert len(names) == 2
            for n in names:
                with open(os.path.join(out_dir, n), "rb") as f:
                    blobs.append(f.read())
        return blobs, [(c[2], c[5]) for c in ConverterEngine.complement_calls]
    one, calls_one = go("one", False)
    many, calls_many = go("many", True)
    assert one == many and calls_one == calls_many
    assert [r for r, _ in calls_one] == [48000, 96000] and calls_one[0][1] < 1.0 and calls_one[1][1] == 1.0


def host_loader(eng_cls):
    """A stand-in for librosa.load behind audio_io.load (librosa is optional): RIFF/WAVE at its own rate, or converted to ``sr`` by the
    double's converter -- which converter brings the mix to the model's rate does not matter to the complement"""
    def load(path, sr=44100, mono=False, res_type=None):
        x, file_sr = audio_io.read_wav(path)
        if sr is not None and sr != file_sr:
            x, file_sr = RR.reference(x, file_sr, sr).astype(np.float32), sr
        return (x[0] if x.shape[0] == 1 else x), file_sr
    return load


@pytest.mark.parametrize("tag", ["mdx_plain", "mdxc_one"])
def test_a_file_the_host_decoder_converts_keeps_its_own_mix(tmp_path, monkeypatch, tag):
    """asx_input_resample at its default, "host": the stems are converted back all the same, so the knob must act -- same files as with
    asx_input_resample="device" here, where both converters are the double's"""
    install(monkeypatch)
    monkeypatch.setattr(audio_io, "load", host_loader(ConverterEngine))
    case = case_by_tag(tag, tmp_path, use_soundfile=True)
    wav = write_input(case, tmp_path, 48000, 0.5)
    F = audio_io.wav_info(wav)["frames"]
    _, names_dev, _, blobs_dev = run(case, wav, "dev", **ON)
    ConverterEngine.complement_calls = []
    host_on = dict(ON, asx_input_resample="host")
    _, names, _, blobs = run(case, wav, "host_on", **host_on)
    assert len(ConverterEngine.complement_calls) == 1 and ConverterEngine.complement_calls[0][3:5] == (F, (2, F))
    assert names == names_dev and blobs == blobs_dev
    _, _, _, blobs_off = run(case, wav, "host_off", **dict(OFF, asx_input_resample="host"))
    assert blobs[1] == blobs_off[1] and blobs[0] != blobs_off[0]
    # the null test on the written FLOAT files
    k = float(np.float32(case[2]["model_data"]["compensate"] if case[1] == "MDXSeparator" else 1.0))
    mix_f, _ = audio_io.read_wav(wav)
    c, _ = audio_io.read_wav(os.path.join(case[2]["output_dir"], "host_on", names[0]))
    p, _ = audio_io.read_wav(os.path.join(case[2]["output_dir"], "host_on", names[1]))
    assert max(np.abs(c).max(), np.abs(p).max()) < 0.9
    assert np.abs(k * p.astype(np.float64) + c - mix_f.astype(np.float64)).max() <= CR.ROUNDING_BOUND


def test_a_decode_that_leaves_no_file_mix_is_said_once_per_file(tmp_path, monkeypatch, caplog):
    """the second decode disagrees with the header (here: one frame short): the complement is written as without the knob, with a warning"""
    install(monkeypatch)
    good = host_loader(ConverterEngine)

    def short(path, sr=44100, mono=False, res_type=None):
        x, rate = good(path, sr, mono, res_type)
        return (x[..., :-1] if sr is None else x), rate
    monkeypatch.setattr(audio_io, "load", short)
    logger = logging.getLogger("asx_complement_rate_host_warn")
    case = case_by_tag("mdx_plain", tmp_path, logger=logger)
    wav = write_input(case, tmp_path, 48000, 0.5)
    with caplog.at_level(logging.WARNING, logger="asx_complement_rate_host_warn"):
        _, names, _, blobs = run(case, wav, "short_on", **dict(ON, asx_input_resample="host"))
    warnings = [r for r in caplog.records if "asx_complement_rate='input', but the file's own mix was not kept" in r.getMessage()]
    assert len(warnings) == 1 and ConverterEngine.complement_calls == []
    _, names_off, _, blobs_off = run(case, wav, "short_off", **dict(OFF, asx_input_resample="host"))
    assert names == names_off and blobs == blobs_off
