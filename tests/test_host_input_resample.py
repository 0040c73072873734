"""The host logic of ``common_config["asx_input_resample"]`` without a GPU: the setting and its environment override, the host-array
path of ``prepare_mix`` (audio_io.read_wav, then the engine's converter) through an engine double that records its calls, the files and
plugins the feature leaves alone, and the ensemble's refusal of members whose settings differ."""
import types

import numpy as np
import pytest

import audio_separator_amd as A
from audio_separator_amd import audio_io
from tests import separate_cases as SC


class ConverterDouble:
    """What CommonSeparator asks of an engine on the host path: the plan (the rule of the library) and the conversion (here: a marker
    array of the planned length, so the test can see that prepare_mix returned the converter's result)."""

    def __init__(self, refuse=()):
        self.calls, self.refuse = [], set(refuse)

    def resample_rational_plan(self, sr_in, sr_out, n_in=1):
        import math
        if sr_in == sr_out or (sr_in, sr_out) in self.refuse:
            raise A.AsxError("refused")
        g = math.gcd(sr_in, sr_out)
        return -(-n_in * (sr_out // g) // (sr_in // g)), sr_out // g, sr_in // g, 205

    def resample_rational(self, x, sr_in, sr_out):
        self.calls.append((x.shape, sr_in, sr_out))
        return np.full((x.shape[0], self.resample_rational_plan(sr_in, sr_out, x.shape[1])[0]), 0.25, np.float32)


def separator(tmp_path, engine=None, **over):
    s = A.CommonSeparator(SC.common_config("m", "/m/model.onnx", {"primary_stem": "Vocals"}, str(tmp_path / "out"), **over))
    s.engine = engine
    return s


def song(tmp_path, rate, channels=2, n=1600, subtype="PCM_16"):
    path = str(tmp_path / f"song_{rate}_{channels}.wav")
    t = np.arange(n) / rate
    x = np.stack([0.5 * np.sin(2 * np.pi * 440 * t), 0.3 * np.sin(2 * np.pi * 660 * t)], axis=1).astype(np.float32)[:, :channels]
    audio_io.write_wav(path, x, rate, subtype)
    return path


def test_setting_default_config_environment(tmp_path, monkeypatch):
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    assert separator(tmp_path).asx_input_resample == "host"
    assert separator(tmp_path, asx_input_resample="device").asx_input_resample == "device"
    monkeypatch.setenv("ASX_INPUT_RESAMPLE", "device")
    assert separator(tmp_path, asx_input_resample="host").asx_input_resample == "device"
    monkeypatch.setenv("ASX_INPUT_RESAMPLE", "")                     # empty: not an override
    assert separator(tmp_path).asx_input_resample == "host"
    monkeypatch.setenv("ASX_INPUT_RESAMPLE", "gpu")
    with pytest.raises(ValueError, match="asx_input_resample"):
        separator(tmp_path)
    monkeypatch.delenv("ASX_INPUT_RESAMPLE")
    with pytest.raises(ValueError, match="asx_input_resample"):
        separator(tmp_path, asx_input_resample="soxr")


@pytest.mark.parametrize("channels", [1, 2])
def test_host_path_reads_the_file_and_converts_with_the_engine(tmp_path, monkeypatch, channels):
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    eng = ConverterDouble()
    s = separator(tmp_path, eng, asx_input_resample="device", asx_profile_file=False)
    mix = s.prepare_mix(song(tmp_path, 48000, channels))
    assert eng.calls == [((channels, 1600), 48000, 44100)]
    assert mix.shape == (2, 1470) and np.all(np.asarray(mix) == 0.25)          # mono is duplicated behind the converter
    assert (s.input_subtype, s.input_bit_depth) == ("PCM_16", 16)


def test_files_the_feature_leaves_alone(tmp_path, monkeypatch):
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    no_librosa = audio_io._optional("librosa") is None
    # the setting is "host": as before
    eng = ConverterDouble()
    s = separator(tmp_path, eng)
    if no_librosa:
        with pytest.raises(audio_io.AudioIOError, match="48000 Hz"):
            s.prepare_mix(song(tmp_path, 48000))
    # a file at the model's rate never reaches the converter
    s = separator(tmp_path, eng, asx_input_resample="device")
    assert s.prepare_mix(song(tmp_path, 44100)).shape == (2, 1600)
    # a pair the plan refuses: as before
    s = separator(tmp_path, ConverterDouble(refuse={(44056, 44100)}), asx_input_resample="device")
    if no_librosa:
        with pytest.raises(audio_io.AudioIOError, match="44056 Hz"):
            s.prepare_mix(song(tmp_path, 44056))
    # an engine without the converter (an older double): as before
    s = separator(tmp_path, object(), asx_input_resample="device")
    if no_librosa:
        with pytest.raises(audio_io.AudioIOError, match="48000 Hz"):
            s.prepare_mix(song(tmp_path, 48000))
    assert eng.calls == []
    # a silent file still raises the reference's error, from the converted (all-zero) mix
    class Zero(ConverterDouble):
        def resample_rational(self, x, sr_in, sr_out):
            return np.zeros_like(super().resample_rational(x, sr_in, sr_out))
    silent = str(tmp_path / "silent.wav")
    audio_io.write_wav(silent, np.zeros((800, 2), np.int16), 48000, "PCM_16")
    with pytest.raises(ValueError, match="empty or not valid"):
        separator(tmp_path, Zero(), asx_input_resample="device").prepare_mix(silent)


def test_vr_stays_out():
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    assert VRSeparator._resamples_input_files is False and MDXSeparator._resamples_input_files is True
    vr = types.SimpleNamespace(asx_input_resample="device", engine=ConverterDouble(), sample_rate=44100, _resamples_input_files=False)
    assert A.CommonSeparator._resample_plan(vr, 48000) is None


def test_ensemble_refuses_members_whose_settings_differ():
    def member(**kw):
        m = dict(sample_rate=44100, normalization_threshold=0.9, amplification_threshold=0.0, model_path="/m/a.onnx", model_name="a",
                 logger=None, output_dir="out", output_format="WAV")
        m.update(kw)
        return types.SimpleNamespace(**m)
    with pytest.raises(ValueError, match="asx_input_resample"):
        A.EnsembleSeparator([member(asx_input_resample="device"), member(asx_input_resample="host")])
    with pytest.raises(ValueError, match="asx_input_resample"):
        A.EnsembleSeparator([member(asx_input_resample="device"), member()])         # a member without the attribute reads "host"
    A.EnsembleSeparator([member(asx_input_resample="device"), member(asx_input_resample="device")])
    A.EnsembleSeparator([member(), member(asx_input_resample="host")])
