"""``common_config["asx_output_rate"]`` and the writer-side form of the rational polyphase converter, without a GPU:

* tests/resample_ref.py -- the float64 definition for any pair of rates, any n_out and either layout -- equals the restatement of
  tests/test_gpu_resample.py for the seven -> 44 100 Hz pairs and is held against csrc/resample_plan.h's own resample_plan_evaluate
  (tests/host/resample_stem_host.cpp, compiled with g++), also past the plan's n_out;
* the length rule min(F, ceil(n r_f / r_m)) gives back exactly the file's F frames;
* the plan's tile fits 64 KiB of LDS for the upsampling pairs;
* the knob's validation, the refusals of VRSeparator and EnsembleSeparator, and the host-array route of ``write_audio`` through an engine
  double."""
import logging
import math
import os
import subprocess
import types

import numpy as np
import pytest

import audio_separator_amd as A
from audio_separator_amd import audio_io
from tests import resample_ref as RR
from tests import separate_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "resample_stem_host.cpp")

MODEL = 44100
TO_MODEL = [48000, 96000, 22050, 32000, 88200, 8000, 192000]            # the pairs of tests/test_gpu_resample.py
UP = [48000, 88200, 96000, 192000]                                     # 44 100 -> these: L > M
FROM_MODEL = UP + [32000, 22050]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("resample_stem") / "resample_stem_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", out, SRC], check=True)
    return out


def noise(n, channels, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (channels, n))


@pytest.mark.parametrize("sr_in", TO_MODEL)
def test_generalised_restatement_equals_the_input_direction_one(sr_in):
    from tests import test_gpu_resample as old
    assert RR.design(sr_in, MODEL)[:4] == old.design(sr_in)[:4]
    np.testing.assert_array_equal(RR.design(sr_in, MODEL)[4], old.design(sr_in)[4])
    L, M, _, T, _ = RR.design(sr_in, MODEL)
    assert RR.tile_outputs(L, M, T) == old.tile_outputs(L, M, T)
    for n in (1, 2, T - 1, 1501):
        x = noise(n, 2, n).astype(np.float32)
        np.testing.assert_array_equal(RR.reference(x, sr_in, MODEL), old.reference(x, sr_in))
        # rows input is planar input of the transposed data
        np.testing.assert_array_equal(RR.reference(np.ascontiguousarray(x.T), sr_in, MODEL, layout="rows"), old.reference(x, sr_in))


@pytest.mark.parametrize("sr_in,sr_out", [(r, MODEL) for r in TO_MODEL] + [(MODEL, r) for r in FROM_MODEL])
def test_restatement_against_the_plan_headers_own_evaluation(exe, sr_in, sr_out):
    """Any n_out: shorter than the plan's, the plan's, and past it until the filter has left the input (exact zeros from there in both).
    Bound: the two designs' taps agree to 1e-12 (tests/test_host_resample_plan.py), an output sums at most T products of inputs in
    [-1, 1] -- T * 1e-12 -- plus the float64 rounding of the two summation orders, T * 2^-52 * max |tap| < 1e-13."""
    L, M, half, T, _ = RR.design(sr_in, sr_out)
    for n_in in (1, T + 3, 700):
        plan = RR.plan_n_out(n_in, L, M)
        zero = RR.zero_from(n_in, L, M, half)
        assert zero >= plan
        x = noise(n_in, 1, n_in + sr_in)[0]
        for n_out in sorted({1, max(plan - 1, 1), plan, plan + 3, zero + 5}):
            r = subprocess.run([exe, "eval", str(sr_in), str(sr_out), str(n_in), str(n_out)], input=x.tobytes(), capture_output=True)
            assert r.returncode == 0, r.stderr
            got = np.frombuffer(r.stdout, np.float64)
            ref = RR.reference(x, sr_in, sr_out, n_out)
            assert got.shape == ref.shape == (n_out,)
            assert np.abs(got - ref).max() <= T * 1e-12 + 1e-13, (n_in, n_out, float(np.abs(got - ref).max()))
            assert not got[zero:].any() and not ref[zero:].any()
        # ... and zero_from is sharp where the last tap is not itself 0
        full = RR.reference(np.ones(n_in), sr_in, sr_out, zero + 1)
        assert full[zero] == 0.0 and (zero == 0 or np.abs(full[max(zero - 2 * L, 0):zero]).max() > 0.0)


@pytest.mark.parametrize("file_rate", FROM_MODEL + [8000, 176400])
def test_length_rule_gives_back_the_files_frame_count(file_rate):
    """A file of F frames enters as n = ceil(F r_m / r_f) samples at the model's rate (librosa's length); min(F, ceil(n r_f / r_m)) is F."""
    rng = np.random.default_rng(file_rate)
    sweep = list(range(1, 2000)) + [int(v) for v in rng.integers(2000, 1 << 33, 4000)] + [4 * 60 * file_rate, (1 << 36) - 1]
    for F in sweep:
        n = -(-F * MODEL // file_rate)
        assert RR.output_frames(n, F, file_rate, MODEL) == F
        # a shorter stem (MDX invert_using_spec: 1024 * (n // 1024) samples) gets its share, never more than the file
        short = 1024 * (n // 1024)
        got = RR.output_frames(short, F, file_rate, MODEL)
        assert got == min(F, -(-short * file_rate // MODEL)) and got <= F and F - got <= -(-1024 * file_rate // MODEL)


@pytest.mark.parametrize("sr_out", FROM_MODEL)
def test_tile_rule_fits_the_lds_for_the_output_pairs(exe, sr_out):
    r = subprocess.run([exe, "plan", str(MODEL), str(sr_out)], capture_output=True)
    assert r.returncode == 0, r.stdout
    L, M, half, T, J, K, span, lds = (int(v) for v in r.stdout.split()[1:])
    g = math.gcd(MODEL, sr_out)
    assert (L, M) == (sr_out // g, MODEL // g) and (L, M, half, T) == RR.design(MODEL, sr_out)[:4]
    assert (J, K, span) == RR.tile(L, M, T)[:3] and bool(lds) == (L * T <= 2048)
    assert J % L == 0 and J >= L and K == 8 and span == J // L * K * M + T
    floats = span + (L * T if lds else 0)
    print(f"{MODEL} -> {sr_out}: L {L} M {M} T {T} J {J} K {K}: {4 * floats} bytes of LDS")
    assert 4 * floats <= 65536 and floats == RR.tile(L, M, T)[3]


def test_free_n_out_is_checked_by_the_plan(exe):
    def check(n_in, n_out):
        r = subprocess.run([exe, "check", "44100", "48000", str(n_in), str(n_out)], capture_output=True)
        return r.returncode, r.stdout.decode()
    assert check(1, 1) == (0, "ok\n") and check(1 << 40, 1 << 40)[0] == 0 and check(5, 1 << 40)[0] == 0
    for n_in, n_out, name in ((0, 5, "n_in"), ((1 << 40) + 1, 5, "n_in"), (5, 0, "n_out"), (5, (1 << 40) + 1, "n_out"), (5, -1, "n_out")):
        rc, out = check(n_in, n_out)
        assert rc == 3 and out.startswith(f"error {name} = "), (n_in, n_out, out)


# ---- the knob --------------------------------------------------------------------------------------------------------------------
class WriterDouble:
    """What write_audio asks of an engine on the host-array route: the plan, the stem converter (a marker array of the asked length)
    and the int16 pass."""

    def __init__(self, refuse=()):
        self.calls, self.refuse = [], set(refuse)

    def resample_rational_plan(self, sr_in, sr_out, n_in=1):
        if sr_in == sr_out or (sr_in, sr_out) in self.refuse:
            raise A.AsxError("refused")
        g = math.gcd(sr_in, sr_out)
        return -(-n_in * (sr_out // g) // (sr_in // g)), sr_out // g, sr_in // g, 189

    def resample_rational_stem(self, x, sr_in, sr_out, n_out, layout="planar"):
        self.calls.append((x.shape, sr_in, sr_out, n_out, layout))
        return np.full((2, n_out), 0.25, np.float32)

    def pcm16(self, stem, max_peak=1.0, min_peak=None):
        a = np.asarray(stem, np.float32)
        return (a * 32767).astype(np.int16), float(np.abs(a).max())

    def normalize(self, wave, max_peak=1.0, min_peak=None):
        return np.asarray(wave, np.float32)


def separator(tmp_path, engine=None, **over):
    s = A.CommonSeparator(SC.common_config("m", "/m/model.onnx", {"primary_stem": "Vocals"}, str(tmp_path / "out"), **over))
    s.engine = engine
    return s


def song(tmp_path, rate, n=1600):
    path = str(tmp_path / f"song_{rate}.wav")
    t = np.arange(n) / rate
    x = np.stack([0.5 * np.sin(2 * np.pi * 440 * t), 0.3 * np.sin(2 * np.pi * 660 * t)], axis=1).astype(np.float32)
    audio_io.write_wav(path, x, rate, "PCM_16")
    return path


def test_setting_default_and_validation(tmp_path, monkeypatch):
    assert A.CommonSeparator.OUTPUT_RATE_MODES == ("model", "input")
    assert separator(tmp_path).asx_output_rate == "model"
    assert separator(tmp_path, asx_output_rate="model").asx_output_rate == "model"
    assert separator(tmp_path, asx_output_rate="input").asx_output_rate == "input"
    for bad in ("gpu", "device", "48000"):
        with pytest.raises(ValueError, match=r"asx_output_rate must be one of \('model', 'input'\)"):
            separator(tmp_path, asx_output_rate=bad)
    monkeypatch.setenv("ASX_OUTPUT_RATE", "input")                       # no environment override
    assert separator(tmp_path).asx_output_rate == "model"
    assert {"_file_rate", "_file_frames"} <= set(A.CommonSeparator._PER_FILE)


def test_vr_and_ensemble_refuse_the_input_rate(tmp_path):
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    common = SC.common_config("m", "/m/model.pth", {"vr_model_param": "4band_v3"}, str(tmp_path / "out"), asx_output_rate="input")
    with pytest.raises(ValueError, match="asx_output_rate='input' is not supported by VRSeparator"):
        VRSeparator(common_config=common, arch_config={})
    assert VRSeparator._output_rate_mode({"asx_output_rate": "model"}) == "model"

    def member(**kw):
        m = dict(sample_rate=44100, normalization_threshold=0.9, amplification_threshold=0.0, model_path="/m/a.onnx", model_name="a",
                 logger=None, output_dir="out", output_format="WAV")
        m.update(kw)
        return types.SimpleNamespace(**m)
    with pytest.raises(ValueError, match="asx_output_rate='input' is not supported in an ensemble"):
        A.EnsembleSeparator([member(), member(asx_output_rate="input")])
    A.EnsembleSeparator([member(), member(asx_output_rate="model")])


@pytest.mark.parametrize("use_soundfile", [False, True])
def test_host_array_route_converts_before_the_writer(tmp_path, use_soundfile):
    """prepare_mix records the file's rate and frames; write_audio converts a host stem to min(F, ceil(n r_f / r_m)) frames and every
    container gets the file's rate.  The array the caller handed over is not touched."""
    eng = WriterDouble()
    s = separator(tmp_path, eng, asx_output_rate="input", asx_input_resample="device", use_soundfile=use_soundfile)
    eng.resample_rational = lambda x, a, b: np.full((2, eng.resample_rational_plan(a, b, x.shape[1])[0]), 0.5, np.float32)
    path = song(tmp_path, 48000)
    s._begin_file(path)
    mix = s.prepare_mix(path)
    assert (s._file_rate, s._file_frames) == (48000, 1600) and mix.shape == (2, 1470)
    stem = np.full((1470, 2), 0.125, np.float32)
    short = stem[:1024]
    s.write_audio("full.wav", stem)
    s.write_audio("short.wav", short)
    assert eng.calls == [((1470, 2), 44100, 48000, 1600, "rows"), ((1024, 2), 44100, 48000, 1115, "rows")]
    assert np.all(stem == 0.125)
    for name, frames in (("full.wav", 1600), ("short.wav", 1115)):
        info = audio_io.wav_info(str(tmp_path / "out" / name))
        assert (info["samplerate"], info["frames"], info["subtype"]) == (48000, frames, "PCM_16")
    assert s.file_timings["resample_out"] > 0.0
    s.clear_file_specific_paths()
    assert (s._file_rate, s._file_frames) == (None, None)


def test_nothing_is_converted_at_the_models_rate_or_without_the_knob(tmp_path, caplog):
    stem = np.full((1600, 2), 0.125, np.float32)
    for rate, over in ((44100, {"asx_output_rate": "input"}), (48000, {}), (48000, {"asx_output_rate": "model"})):
        eng = WriterDouble()
        s = separator(tmp_path, eng, **over)
        path = song(tmp_path, rate)
        s._begin_file(path)
        s._probe_file_rate(path)
        s.input_bit_depth = 16
        with caplog.at_level(logging.WARNING):
            s.write_audio("same.wav", stem)
        info = audio_io.wav_info(str(tmp_path / "out" / "same.wav"))
        assert (info["samplerate"], info["frames"]) == (44100, 1600)
        assert eng.calls == [] and "resample_out" not in s.file_timings
        assert "asx_output_rate" not in caplog.text


def test_unknown_rate_or_refused_pair_warns_once_per_file(tmp_path, caplog):
    stem = np.full((1600, 2), 0.125, np.float32)
    for refuse, probe in (((), False), ({(44100, 44056)}, True)):
        eng = WriterDouble(refuse=refuse)
        s = separator(tmp_path, eng, asx_output_rate="input")
        s.logger = logging.getLogger("asx_output_rate_test")
        path = song(tmp_path, 44056)
        s._begin_file(path)
        if probe:
            s._probe_file_rate(path)
        s.input_bit_depth, s._file_seconds = 16, 1.0
        caplog.clear()
        with caplog.at_level(logging.WARNING, logger="asx_output_rate_test"):
            s.write_audio("a.wav", stem)
            s.write_audio("b.wav", stem)
        warnings = [r for r in caplog.records if "asx_output_rate='input'" in r.getMessage()]
        assert len(warnings) == 1 and "written at 44100 Hz" in warnings[0].getMessage()
        assert eng.calls == []
        for name in ("a.wav", "b.wav"):
            info = audio_io.wav_info(str(tmp_path / "out" / name))
            assert (info["samplerate"], info["frames"]) == (44100, 1600)
