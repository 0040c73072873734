"""The host logic of FLAC output in CommonSeparator.write_audio_pydub without a GPU, through an engine double that records its calls:
who compresses a ``.flac`` stem (``common_config["asx_output_encoder"]``, its environment override, the presence of pydub), the stream
width for each input bit depth, the MD5 handed to audio_io.write_flac, and the formats that still need pydub."""
import hashlib
import sys
import types

import numpy as np
import pytest

import audio_separator_amd as A
from audio_separator_amd import audio_io
from tests import flac_ref as F
from tests import separate_cases as SC


class EncoderDouble:
    """pcm16 quantises like the engine does for in-range stems; flac_encode returns one marker frame per 4096 samples"""
    FLAC_BLOCK_SIZE = 4096

    def __init__(self):
        self.calls = []

    def pcm16(self, a, max_peak, min_peak):
        a = np.asarray(a, np.float32)
        return (a * 32767).astype(np.int16), float(np.abs(a).max())

    def flac_encode(self, pcm, samplerate, bits_per_sample=16, block_size=4096):
        assert pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[1] == 2
        self.calls.append((pcm.copy(), samplerate, bits_per_sample, block_size))
        nb = -(-pcm.shape[0] // block_size)
        return np.full(20 * nb, 0xAB, np.uint8), np.full(nb, 20, np.int32)


def separator(tmp_path, engine, **over):
    s = A.CommonSeparator(SC.common_config("m", "/m/model.onnx", {"primary_stem": "Vocals"}, str(tmp_path / "out"), **over))
    s.engine = engine
    return s


def stem(n=5000):
    t = np.arange(n) / 44100.0
    return np.stack([0.5 * np.sin(2 * np.pi * 440 * t), 0.25 * np.sin(2 * np.pi * 660 * t)], 1).astype(np.float32)


@pytest.fixture
def no_pydub(monkeypatch):
    monkeypatch.setitem(sys.modules, "pydub", None)          # "import pydub" raises ImportError
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)


@pytest.fixture
def fake_pydub(monkeypatch):
    exports = []

    class AudioSegment:
        def __init__(self, data, frame_rate, sample_width, channels):
            self.data = data

        def export(self, path, **params):
            exports.append((path, params))
            with open(path, "wb") as f:
                f.write(b"pydub")
    monkeypatch.setitem(sys.modules, "pydub", types.SimpleNamespace(AudioSegment=AudioSegment))
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    return exports


def test_setting_default_config_environment(tmp_path, monkeypatch):
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    assert separator(tmp_path, None).asx_output_encoder == "host"
    assert separator(tmp_path, None, asx_output_encoder="device").asx_output_encoder == "device"
    monkeypatch.setenv("ASX_OUTPUT_ENCODER", "device")
    assert separator(tmp_path, None, asx_output_encoder="host").asx_output_encoder == "device"
    monkeypatch.setenv("ASX_OUTPUT_ENCODER", "")                      # empty: not an override
    assert separator(tmp_path, None).asx_output_encoder == "host"
    monkeypatch.setenv("ASX_OUTPUT_ENCODER", "gpu")
    with pytest.raises(ValueError, match="asx_output_encoder"):
        separator(tmp_path, None)
    monkeypatch.delenv("ASX_OUTPUT_ENCODER")
    with pytest.raises(ValueError, match="asx_output_encoder"):
        separator(tmp_path, None, asx_output_encoder="ffmpeg")


@pytest.mark.parametrize("depth,bits", [(None, 16), (16, 16), (24, 24), (32, 24)])
def test_without_pydub_flac_reaches_the_encoder(tmp_path, no_pydub, depth, bits):
    eng = EncoderDouble()
    s = separator(tmp_path, eng)
    s.input_bit_depth = depth
    x = stem()
    s.write_audio("a_(Vocals).flac", x)
    (pcm, rate, got_bits, block), = eng.calls
    assert (rate, got_bits, block) == (44100, bits, 4096) and np.array_equal(pcm, (x * 32767).astype(np.int16))
    assert s.last_write_path == "flac_device_upload" and s.file_timings["flac_encode"] >= 0.0
    data = open(tmp_path / "out" / "a_(Vocals).flac", "rb").read()
    info, _, first = F.parse_container(data)
    assert data[first:] == bytes([0xAB]) * 40
    assert (info["bits_per_sample"], info["channels"], info["samplerate"], info["total_samples"]) == (bits, 2, 44100, 5000)
    assert (info["min_blocksize"], info["max_blocksize"], info["min_framesize"], info["max_framesize"]) == (4096, 4096, 20, 20)
    assert info["md5"] == hashlib.md5(F.pcm_bytes(pcm.astype(np.int64) << (bits - 16), bits)).digest()


def test_int16_stems_and_silent_stems(tmp_path, no_pydub):
    eng = EncoderDouble()
    s = separator(tmp_path, eng)
    q = (stem(300) * 32767).astype(np.int16)
    s.write_audio("q.flac", q)
    assert np.array_equal(eng.calls[0][0], q)
    s.write_audio("silent.flac", np.zeros((300, 2), np.float32))
    assert len(eng.calls) == 1 and not (tmp_path / "out" / "silent.flac").exists()


def test_writes_inside_separate_are_drained(tmp_path, no_pydub, monkeypatch):
    eng = EncoderDouble()
    s = separator(tmp_path, eng)
    started = []
    real = audio_io.write_flac

    def slow(*a, **k):
        import threading
        started.append(threading.current_thread().name)
        real(*a, **k)
    monkeypatch.setattr(audio_io, "write_flac", slow)
    with s._writing():
        s.write_audio("w.flac", stem(100))
    assert started == ["asx-wav-writer"] and (tmp_path / "out" / "w.flac").exists() and s._pending_writes == []
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    with s._writing():
        s.write_audio("v.flac", stem(100))
    assert started[1] != "asx-wav-writer"


def test_with_pydub_the_export_call_still_wins(tmp_path, fake_pydub):
    eng = EncoderDouble()
    s = separator(tmp_path, eng)
    s.write_audio("a.flac", stem())
    assert eng.calls == [] and len(fake_pydub) == 1
    path, params = fake_pydub[0]
    assert path.endswith("a.flac") and params == {"format": "flac", "parameters": ["-sample_fmt", "s16"]}
    assert s.last_write_path is None and "flac_encode" not in s.file_timings


def test_with_pydub_and_the_device_setting_the_encoder_wins(tmp_path, fake_pydub, monkeypatch):
    eng = EncoderDouble()
    s = separator(tmp_path, eng, asx_output_encoder="device")
    s.write_audio("a.flac", stem())
    s.write_audio("a.wav", stem())
    assert len(eng.calls) == 1 and [p for p, _ in fake_pydub] == [str(tmp_path / "out" / "a.wav")]
    assert open(tmp_path / "out" / "a.flac", "rb").read(4) == b"fLaC"
    monkeypatch.setenv("ASX_OUTPUT_ENCODER", "device")       # the process-wide override
    eng2 = EncoderDouble()
    separator(tmp_path, eng2).write_audio("b.flac", stem())
    assert len(eng2.calls) == 1 and len(fake_pydub) == 1


@pytest.mark.parametrize("ext", ["mp3", "m4a", "ogg"])
def test_other_formats_still_need_pydub(tmp_path, no_pydub, ext):
    eng = EncoderDouble()
    s = separator(tmp_path, eng, asx_output_encoder="device")
    with pytest.raises(audio_io.AudioIOError, match="pydub"):
        s.write_audio(f"a.{ext}", stem())
    assert eng.calls == []
