"""The device FLAC decoder (asx_flac_decode_scan_dev / asx_flac_decode_finish_dev, csrc/kernels_flac_dec.h) end to end.  Decoding is exact
integer arithmetic, so every comparison is for equality: mix * 2^(bits-1) against the integers of tests/flac_ref.py (the fixtures) or of
the stream's own description (tests/flac_synth.py, pinned to flac_ref by tests/test_host_flac_synth.py), and the frame and byte counts.

The damaged streams are the decoder's error path -- a frame that fails its CRC or runs past its bound ends the chain -- and the same
bytes pass through the host-compiled kernel under a sanitizer in tests/test_host_flac_decode_kernel.py.

File level: a .flac input takes the plugins' file fast path and leaves stem files byte-identical to those of the same samples as WAV."""
import os
import shutil

import numpy as np
import pytest

from tests import flac_ref as F
from tests import flac_synth as Y
from tests import separate_cases as SC
from tests.test_gpu_flac import CONTENTS, RATE
from tests.test_gpu_separate_rates import rewritten, separate_once

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac")
FIXTURES = ("mardy20s_87.flac", "ref_levee_drums_vocals_8.flac", "sing_sing_sing_brass_178.flac")
STREAMS = sorted(Y.streams())


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(), device=0)
    yield e
    e.close()


def _ints(mix, bits):
    x = mix.astype(np.float64) * (1 << (bits - 1))
    assert mix.dtype == np.float32 and np.array_equal(x, np.rint(x))
    return x.astype(np.int64)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(eng, name):
    with open(os.path.join(FIX, name), "rb") as f:
        data = f.read()
    info, pcm, frames = F.decode(data)
    first = frames[0]["offset"]
    mix, d = eng.flac_decode(data[first:], info, details=True)
    assert np.array_equal(_ints(mix, info["bits_per_sample"]), pcm.T)
    assert (d["n_samples"], d["n_frames"], d["bytes_consumed"]) == (pcm.shape[0], len(frames), len(data) - first)
    assert d["peak"] == float(np.abs(mix).max())


@pytest.mark.parametrize("name", STREAMS)
def test_builder_stream(eng, name):
    """intact streams decode to their description; damaged ones to the frames before the damage"""
    s = Y.streams()[name]
    mix, d = eng.flac_decode(Y.audio(s), s["info"], details=True)
    assert np.array_equal(_ints(mix, s["info"]["bits_per_sample"]), Y.planar(s))
    assert (d["n_samples"], d["n_frames"], d["bytes_consumed"]) == (s["pcm"].shape[0], s["n_frames"], s["bytes_consumed"])


@pytest.mark.parametrize("bits", [16, 24])
def test_round_trip_with_the_device_encoder(eng, tmp_path, bits):
    from audio_separator_amd import audio_io
    for name, pcm in CONTENTS.items():
        frames, sizes = eng.flac_encode(pcm, RATE, bits, 4096)
        path = str(tmp_path / f"{bits}.flac")
        audio_io.write_flac(path, frames, sizes, RATE, bits, pcm.shape[0])
        info = audio_io.flac_stream(path)
        with open(path, "rb") as f:
            data = f.read()
        assert info["audio_offset"] == 42 and info["audio_bytes"] == frames.size and info["bits_per_sample"] == bits
        mix, d = eng.flac_decode(data[info["audio_offset"]:], info, details=True)
        assert np.array_equal(_ints(mix, bits), pcm.astype(np.int64).T << (bits - 16)), name
        assert (d["n_frames"], d["bytes_consumed"]) == (len(sizes), frames.size), name


def test_two_decodes_are_bit_identical(eng):
    with open(os.path.join(FIX, "mardy20s_87.flac"), "rb") as f:
        data = f.read()
    info, _, first = F.parse_container(data)
    a = eng.flac_decode(data[first:], info)
    b = eng.flac_decode(data[first:], info)
    assert a.tobytes() == b.tobytes()


def test_calls_refuse_bad_arguments(eng):
    import audio_separator_amd as A
    import torch
    s = Y.streams()["verbatim"]
    info = s["info"]
    audio = torch.frombuffer(bytearray(Y.audio(s)), dtype=torch.uint8).cuda()
    mix = torch.empty((2, s["pcm"].shape[0]), dtype=torch.float32, device="cuda")
    fresh = A.Engine(A.MDXConfig(), device=0)
    try:
        with pytest.raises(A.AsxError, match="scan"):                     # a finish without a scan
            fresh.flac_decode_finish_dev(mix.data_ptr(), mix.shape[1])
        for bad, word in ((dict(info, bits_per_sample=32), "bits per sample"), (dict(info, channels=3), "channels"),
                          (dict(info, max_blocksize=16385), "block size"), (dict(info, samplerate=0), "sample rate")):
            with pytest.raises(A.AsxError, match=word):
                fresh.flac_decode_scan_dev(audio.data_ptr(), audio.numel(), bad)
        with pytest.raises(A.AsxError, match="empty"):
            fresh.flac_decode_scan_dev(audio.data_ptr(), 0, info)
        with pytest.raises(A.AsxError, match="aligned"):
            fresh.flac_decode_scan_dev(audio.data_ptr() + 1, audio.numel() - 1, info)
        with pytest.raises(A.AsxError, match="null"):
            fresh.flac_decode_scan_dev(0, audio.numel(), info)
        with pytest.raises(A.AsxError, match="scan"):                     # none of the refused scans counts as one
            fresh.flac_decode_finish_dev(mix.data_ptr(), mix.shape[1])
        found = fresh.flac_decode_scan_dev(audio.data_ptr(), audio.numel(), info)
        assert found == {"n_samples": s["pcm"].shape[0], "n_frames": s["n_frames"], "bytes_consumed": s["bytes_consumed"]}
        with pytest.raises(A.AsxError, match="n_samples"):
            fresh.flac_decode_finish_dev(mix.data_ptr(), mix.shape[1] - 1)
        with pytest.raises(A.AsxError, match="null"):
            fresh.flac_decode_finish_dev(0, mix.shape[1])
        peak = fresh.flac_decode_finish_dev(mix.data_ptr(), mix.shape[1])
        assert np.array_equal(_ints(mix.cpu().numpy(), 16), Y.planar(s)) and peak == float(mix.abs().max())
    finally:
        fresh.close()
    lib = A.engine.load_library()
    assert lib.asx_flac_decode_scan_dev(None, None, 0, 0, 0, 0, 0, 0, None, None, None, None) != 0       # a null engine is an error
    assert lib.asx_flac_decode_finish_dev(None, None, 0, None, None) != 0


# ---- file level ---------------------------------------------------------------------------------------------------------------
def _as_flac(eng, wav, path, bits):
    """the 16-bit stereo WAV's samples as a FLAC file of `bits` bits (24: every value shifted left by 8), written by the device encoder"""
    from audio_separator_amd import audio_io
    i = audio_io.wav_info(wav)
    assert i["subtype"] == "PCM_16" and i["channels"] == 2
    x, sr = audio_io.read_wav(wav)
    pcm = np.ascontiguousarray(np.rint(x.T.astype(np.float64) * 32768.0), np.int16)
    frames, sizes = eng.flac_encode(pcm, sr, bits, 4096)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    audio_io.write_flac(path, frames, sizes, sr, bits, pcm.shape[0])
    return path


def _as_wav(wav, path, subtype):
    """the 16-bit WAV's samples as a WAV file of another width: int16 is widened bit-exactly (v << 8 for PCM_24), as the FLAC file's are"""
    from audio_separator_amd import audio_io
    x, sr = audio_io.read_wav(wav)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    audio_io.write_wav(path, np.ascontiguousarray(np.rint(x.T.astype(np.float64) * 32768.0), np.int16), sr, subtype)
    return path


@pytest.mark.parametrize("bits", [16, 24])
def test_mdx_separates_a_flac_file(eng, tmp_path, monkeypatch, bits):
    from audio_separator_amd import audio_io
    monkeypatch.delenv("ASX_FILE_FASTPATH", raising=False)
    case = SC.cases("mdx", str(tmp_path))[0]
    base = os.path.basename(case[4])
    wav = _as_wav(case[4], str(tmp_path / "w" / base), f"PCM_{bits}")
    flac = _as_flac(eng, case[4], str(tmp_path / "f" / (os.path.splitext(base)[0] + ".flac")), bits)
    names_w, _, blobs_w, t_w, state_w = separate_once(case, wav, "wav")
    names_f, _, blobs_f, t_f, state_f = separate_once(case, flac, "flac")
    assert names_f == names_w and blobs_f == blobs_w and len(blobs_f) >= 2
    assert "flac_decode" in t_f and "read" in t_f and "h2d_decode" not in t_f and "flac_decode" not in t_w
    assert state_f == state_w == (f"PCM_{bits}", bits, 3000 / 44100.0)
    if audio_io._optional("librosa") is None:
        monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
        with pytest.raises(audio_io.AudioIOError, match="decoded on the device"):
            separate_once(case, flac, "off")


def test_a_silent_flac_is_refused_like_a_silent_wav(eng, tmp_path):
    from audio_separator_amd import audio_io
    case = SC.cases("mdx", str(tmp_path))[0]
    frames, sizes = eng.flac_encode(np.zeros((5000, 2), np.int16), 44100, 16, 4096)
    path = str(tmp_path / "silent.flac")
    audio_io.write_flac(path, frames, sizes, 44100, 16, 5000)
    with pytest.raises(ValueError, match="is empty or not valid"):
        separate_once(case, path, "silent")


@pytest.mark.parametrize("family,index", [("vr", 0), ("mdxc", 0)])
def test_other_plugins_separate_a_flac_file(eng, tmp_path, family, index):
    case = SC.cases(family, str(tmp_path))[index]
    flac = _as_flac(eng, case[4], str(tmp_path / "f" / (os.path.splitext(os.path.basename(case[4]))[0] + ".flac")), 16)
    names_w, _, blobs_w, t_w, _ = separate_once(case, case[4], "wav")
    names_f, _, blobs_f, t_f, _ = separate_once(case, flac, "flac")
    assert "h2d_decode" in t_w and "flac_decode" in t_f, (t_w, t_f)
    assert names_f == names_w and blobs_f == blobs_w and len(blobs_f) >= 1


def test_separate_many_pools_flac_and_wav(eng, tmp_path):
    import audio_separator_amd as A
    tmp = str(tmp_path)
    src = os.path.join(SC.AUDIO, "mdx_in.wav")
    flac = _as_flac(eng, src, str(tmp_path / "in" / "song_a.flac"), 16)
    wav = str(tmp_path / "in" / "song_b.wav")
    shutil.copyfile(src, wav)
    members = []
    for case in (SC.cases("mdx", tmp)[0], SC.cases("mdxc", tmp)[1]):
        _, cls, common, arch, _, _ = case
        members.append(SC.plugin_class(cls)(common_config=dict(common), arch_config=arch))
    ens = A.EnsembleSeparator(members, "avg_wave")
    ens.output_dir = str(tmp_path / "many")
    assert ens._runs([flac, wav]) == [[0, 1]]
    out_f, out_w = ens.separate_many([flac, wav])
    assert ens.last_path_taken == "device" and len(out_f) == len(out_w) >= 2
    for a, b in zip(out_f, out_w):
        assert a != b
        with open(a, "rb") as fa, open(b, "rb") as fb:
            assert fa.read() == fb.read()


def test_a_flac_at_another_rate(eng, tmp_path, monkeypatch):
    from audio_separator_amd import audio_io
    monkeypatch.delenv("ASX_INPUT_RESAMPLE", raising=False)
    case = SC.cases("mdx", str(tmp_path))[0]
    wav, frames = rewritten(case, tmp_path, 48000)
    flac = _as_flac(eng, wav, str(tmp_path / "f48" / (os.path.splitext(os.path.basename(wav))[0] + ".flac")), 16)
    assert audio_io.flac_stream(flac)["samplerate"] == 48000
    names_w, _, blobs_w, t_w, _ = separate_once(case, wav, "wav48", asx_input_resample="device")
    names_f, _, blobs_f, t_f, state = separate_once(case, flac, "flac48", asx_input_resample="device")
    assert names_f == names_w and blobs_f == blobs_w
    assert "flac_decode" in t_f and "resample" in t_f and state == ("PCM_16", 16, frames / 48000.0)
    if audio_io._optional("librosa") is None:
        with pytest.raises(audio_io.AudioIOError, match="48000 Hz"):
            separate_once(case, flac, "flac48_host")
