"""CommonSeparator's bit-depth and stem-order contract, on CPU: the input's sample format is detected when a file is decoded
and kept when the stems are written (both writer paths, with the built-in WAV writer standing in for pydub / soundfile), and a
``target_instrument`` listed second in ``training.instruments`` swaps the primary / secondary stem names.  The writer's
normalise / quantise step runs on the oracle-backed engine double of tests/fake_engine.py."""
import numpy as np
import pytest

import audio_separator_amd as A
from audio_separator_amd import audio_io
from tests import separate_cases as SC
from tests.fake_engine import OracleEngine

SUBTYPE_DEPTH = {"PCM_16": 16, "PCM_24": 24, "PCM_32": 32}


@pytest.fixture(autouse=True)
def builtin_containers(monkeypatch):
    """No pydub / soundfile: the built-in RIFF/WAVE writer is the container on both writer paths."""
    real = audio_io._optional
    monkeypatch.setattr(audio_io, "_optional", lambda name: None if name in ("pydub", "soundfile") else real(name))


def _separator(tmp_path, model_data=None, **over):
    s = A.CommonSeparator(SC.common_config("bitdepth_model", "/m/model.onnx", model_data or {"primary_stem": "Vocals"}, str(tmp_path / "out"),
                                           **over))
    s.engine = OracleEngine(A.MDXConfig())
    return s


def _song(tmp_path, name, subtype, n=2048, sr=44100):
    t = np.arange(n) / sr
    x = np.stack([0.5 * np.sin(2 * np.pi * 440 * t), 0.3 * np.sin(2 * np.pi * 660 * t)], axis=1).astype(np.float32)
    p = str(tmp_path / name)
    audio_io.write_wav(p, x, sr, subtype)
    return p


@pytest.mark.parametrize("subtype", sorted(SUBTYPE_DEPTH))
def test_bit_depth_detected_from_file(tmp_path, subtype):
    s = _separator(tmp_path)
    mix = s.prepare_mix(_song(tmp_path, "in.wav", subtype))
    assert mix.shape == (2, 2048)
    assert (s.input_bit_depth, s.input_subtype) == (SUBTYPE_DEPTH[subtype], subtype)


def test_array_input_defaults_to_16_bit(tmp_path):
    s = _separator(tmp_path)
    s.prepare_mix(np.zeros((64, 2), np.float32))
    assert (s.input_bit_depth, s.input_subtype) == (16, "PCM_16")


def test_bit_depth_follows_each_file(tmp_path):
    """One instance, several inputs: every decoded file sets the depth anew; an array input keeps what the last file set."""
    s = _separator(tmp_path)
    for i, subtype in enumerate(("PCM_24", "PCM_16", "PCM_32", "PCM_24")):
        s.prepare_mix(_song(tmp_path, f"in{i}.wav", subtype))
        assert (s.input_bit_depth, s.input_subtype) == (SUBTYPE_DEPTH[subtype], subtype)
    s.prepare_mix(np.ones((64, 2), np.float32))
    assert (s.input_bit_depth, s.input_subtype) == (24, "PCM_24")


@pytest.mark.parametrize("use_soundfile", [False, True], ids=["pydub_path", "soundfile_path"])
@pytest.mark.parametrize("subtype", sorted(SUBTYPE_DEPTH))
def test_stems_keep_the_input_bit_depth(tmp_path, subtype, use_soundfile):
    s = _separator(tmp_path, use_soundfile=use_soundfile)
    mix = s.prepare_mix(_song(tmp_path, "in.wav", subtype))
    s.write_audio("stem.wav", mix.T)
    info = audio_io.info(str(tmp_path / "out" / "stem.wav"))
    assert (info["subtype"], info["channels"], info["frames"], info["samplerate"]) == (subtype, 2, 2048, 44100)
    y, _ = audio_io.read_wav(str(tmp_path / "out" / "stem.wav"))
    want = mix / np.abs(mix).max() * 0.9 if np.abs(mix).max() > 0.9 else mix       # normalisation_threshold 0.9
    assert np.abs(y - want).max() < 2 / 32767                                       # 16-bit quantisation at most


@pytest.mark.parametrize("instruments,target,names", [
    (["vocals", "other"], "vocals", ("vocals", "other")),          # target listed first: no swap
    (["other", "vocals"], "vocals", ("vocals", "other")),          # target listed second: swapped
    (["vocals", "other"], None, ("vocals", "other")),              # no target: instruments order
    (["vocals", "other"], "drums", ("vocals", "other")),           # target not among the instruments: instruments order
])
def test_target_instrument_stem_swap(tmp_path, instruments, target, names):
    s = _separator(tmp_path, model_data={"training": {"instruments": instruments, "target_instrument": target}})
    assert (s.primary_stem_name, s.secondary_stem_name) == names
