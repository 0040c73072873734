"""The device FLAC encoder (asx_flac_encode / asx_flac_encode_dev, csrc/kernels_flac.h) end to end.  FLAC is lossless, so every check of
the samples is exact: tests/flac_ref.py (an independent decoder that verifies every CRC) must restore exactly what went in.

Compression is checked against the reference's own writer: the PCM of an ffmpeg-written file, re-encoded on the device at block 4096, must
come out below what fixed predictors alone can reach (so LPC is searched and chosen) and within 1 % of the file's own audio-frame bytes.
The 1 % is room for float rounding choosing slightly different coefficients than a float64 CPU estimate of the same search, which gave
0.984 x the file's bytes for the whole file (fixed predictors only: 1.143 x); the committed fixture is the file's first 178 frames (the whole
file is larger than a committed file may be), for which the host-compiled kernel gives 0.982 x and fixed predictors alone 1.120 x.
Measured on the MI355X: 0.9818 x (profiles/NOTES.md)."""
import hashlib
import os

import numpy as np
import pytest

from tests import flac_ref as F
from tests import separate_cases as SC

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac")
N3 = 3 * 4096 + 17
RATE = 44100


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(), device=0)
    yield e
    e.close()


def _contents():
    rng = np.random.default_rng(7)
    t = np.arange(N3)
    c = {}
    for n in (1, 17, 4095, 4096, 4097, N3):
        c[f"noise_{n}"] = rng.integers(-20, 21, (n, 2))
    c["silence"] = np.zeros((N3, 2))
    c["constant_-3"] = np.full((N3, 2), -3)
    a = rng.integers(-3000, 3001, N3)
    c["left_equals_right"] = np.stack([a, a], 1)
    sq = np.where(rng.integers(0, 2, N3) > 0, 32767, -32767)
    c["left_is_minus_right_full_scale"] = np.stack([sq, -sq], 1)        # S = +-65534; with -32768: -65535 below
    c["left_is_minus_right_full_scale"][5] = (-32768, 32767)
    c["left_is_minus_right_full_scale"][6] = (32767, -32768)
    c["right_silent"] = np.stack([a, np.zeros(N3, np.int64)], 1)
    c["ramp"] = np.stack([t - 6000, 6000 - t], 1)
    s = np.rint(100 * np.sin(2 * np.pi * 440 * t / RATE))
    c["sine_440_amplitude_100"] = np.stack([s, np.roll(s, 11)], 1)
    ny = np.rint(32767 * np.sin(2 * np.pi * 21900 * t / RATE + 0.3))
    c["near_nyquist_full_scale"] = np.stack([ny, np.roll(ny, 3)], 1)
    alt = np.where(t % 2 == 0, 32767, -32768)
    c["alternating_extremes"] = np.stack([alt, -alt - 1], 1)
    c["white_noise_full_scale"] = rng.integers(-32768, 32768, (N3, 2))
    imp = np.zeros((N3, 2), np.int64)
    imp[100, 0], imp[5000, 1], imp[9000, 0] = 32767, -32768, -32768
    c["three_impulses"] = imp
    return {k: np.ascontiguousarray(v, np.int16) for k, v in c.items()}


CONTENTS = _contents()


def _round_trip(eng, pcm, bits, tmp_path):
    from audio_separator_amd import audio_io
    n = pcm.shape[0]
    plan = eng.flac_plan(n, 2, bits, 4096)
    frames, sizes = eng.flac_encode(pcm, RATE, bits, 4096)
    assert sizes.shape == (plan["n_blocks"],) and int(sizes.sum()) == frames.size <= plan["max_bytes"]
    assert int(sizes.max()) <= plan["frame_stride"]
    want = pcm.astype(np.int64) << (bits - 16)
    raw = F.pcm_bytes(want, bits)
    path = str(tmp_path / "out.flac")
    audio_io.write_flac(path, frames, sizes, RATE, bits, n, hashlib.md5(raw).digest())
    with open(path, "rb") as f:
        info, got, decoded = F.decode(f.read())                        # raises on any CRC-8 / CRC-16 mismatch
    assert got.shape == want.shape and np.array_equal(got, want)
    assert [d["size"] for d in decoded] == sizes.tolist() and [d["number"] for d in decoded] == list(range(len(sizes)))
    assert all(d["bits_per_sample"] == bits and d["samplerate"] == RATE and not d["variable"] for d in decoded)
    assert [d["blocksize"] for d in decoded] == [4096] * (n // 4096) + ([n % 4096] if n % 4096 else [])
    assert (info["bits_per_sample"], info["channels"], info["samplerate"], info["total_samples"]) == (bits, 2, RATE, n)
    assert info["md5"] == hashlib.md5(raw).digest()
    assert (info["min_framesize"], info["max_framesize"]) == (int(sizes.min()), int(sizes.max()))
    assert info["min_blocksize"] == info["max_blocksize"] == 4096
    if bits == 24:
        assert all(s["wasted"] in (7, 8) for d in decoded for s in d["subframes"])
    return frames, sizes, decoded


@pytest.mark.parametrize("bits", [16, 24])
@pytest.mark.parametrize("name", list(CONTENTS))
def test_exact_round_trip(eng, tmp_path, name, bits):
    pcm = CONTENTS[name]
    frames, sizes, decoded = _round_trip(eng, pcm, bits, tmp_path)
    kinds = [s["type"] for d in decoded for s in d["subframes"]]
    if name in ("silence", "constant_-3"):
        assert set(kinds) == {"CONSTANT"}
    if name == "white_noise_full_scale":
        assert set(kinds) == {"VERBATIM"}
    if name == "near_nyquist_full_scale":
        assert "LPC" in kinds
    if name == "three_impulses":
        params = [s["params"] for d in decoded for s in d["subframes"] if s["type"] not in ("CONSTANT", "VERBATIM")]
        assert params and all(len(set(p)) > 1 for p in params)           # the impulse's partition takes another parameter than the silent ones
    if name in ("left_equals_right", "right_silent"):
        assert frames.size < 1.1 * pcm.shape[0] * 2                      # one channel's worth, not two


def test_two_encodes_are_byte_identical(eng):
    pcm = CONTENTS["near_nyquist_full_scale"]
    a, sa = eng.flac_encode(pcm, RATE, 16, 4096)
    b, sb = eng.flac_encode(pcm, RATE, 16, 4096)
    assert np.array_equal(a, b) and np.array_equal(sa, sb)


def test_other_block_sizes_and_rates(eng, tmp_path):
    """a block size with a table code (4608), two with explicit 8- and 16-bit sizes, rates with explicit header fields"""
    pcm = CONTENTS[f"noise_{N3}"]
    for block, rate in ((4608, 48000), (100, 12345), (1000, 655350), (16, 1000000)):
        frames, sizes = eng.flac_encode(pcm, rate, 16, block)
        got, decoded = F.decode_frames(frames.tobytes(), {"bits_per_sample": 16, "samplerate": rate})
        assert np.array_equal(got, pcm) and [d["size"] for d in decoded] == sizes.tolist()
        assert all(d["samplerate"] == rate for d in decoded) and decoded[0]["blocksize"] == block


def test_device_call_refuses_bad_arguments(eng):
    import audio_separator_amd as A
    import torch
    pcm = torch.zeros((100, 2), dtype=torch.int16, device="cuda")
    out = torch.empty(16, dtype=torch.uint8, device="cuda")
    sizes = torch.empty(1, dtype=torch.int32, device="cuda")
    with pytest.raises(A.AsxError, match="out_capacity"):
        eng.flac_encode_dev(pcm.data_ptr(), 100, RATE, 16, 4096, out.data_ptr(), 16, sizes.data_ptr())
    with pytest.raises(A.AsxError, match="bits per sample"):
        eng.flac_encode_dev(pcm.data_ptr(), 100, RATE, 20, 4096, out.data_ptr(), 16, sizes.data_ptr())
    with pytest.raises(A.AsxError, match="sample rate"):
        eng.flac_encode_dev(pcm.data_ptr(), 100, 0, 16, 4096, out.data_ptr(), 1 << 20, sizes.data_ptr())


def test_compression_against_the_reference_writer(eng):
    """ffmpeg's own file (blocks of 4608, LPC up to order 8) against the device's encode of the same samples at block 4096"""
    with open(os.path.join(FIX, "sing_sing_sing_brass_178.flac"), "rb") as f:
        _, pcm, ref_frames = F.decode(f.read())
    ref_bytes = sum(d["size"] for d in ref_frames)
    assert ref_bytes == 998221
    pcm16 = np.ascontiguousarray(pcm, np.int16)
    frames, sizes = eng.flac_encode(pcm16, RATE, 16, 4096)
    fixed_only = F.fixed_only_bytes(pcm, 4096)
    print(f"device {frames.size} bytes = {frames.size / ref_bytes:.4f} x the file's {ref_bytes}; fixed-only {fixed_only} = {fixed_only / ref_bytes:.4f} x")
    got, decoded = F.decode_frames(frames.tobytes(), {"bits_per_sample": 16, "samplerate": RATE})
    assert np.array_equal(got, pcm)
    assert frames.size < fixed_only
    assert frames.size <= 1.01 * ref_bytes
    assert any(s["type"] == "LPC" for d in decoded for s in d["subframes"])


# ---- file level ---------------------------------------------------------------------------------------------------------------
def _read_wav_ints(path):
    from audio_separator_amd import audio_io
    i = audio_io.wav_info(path)
    x, _ = audio_io.read_wav(path)
    return np.rint(x.T.astype(np.float64) * (1 << (i["bits"] - 1))).astype(np.int64), i["bits"]


def _separate(case, wav, fmt, **over):
    _, cls, common, arch, _, _ = case
    out_dir = os.path.join(common["output_dir"], fmt)
    inst = SC.plugin_class(cls)(common_config=dict(common, output_format=fmt, output_dir=out_dir, **over), arch_config=arch)
    names = inst.separate(wav, None)
    paths = [os.path.join(out_dir, n) for n in names]
    timings, how = dict(inst.file_timings), inst.last_write_path
    inst.clear_gpu_cache()
    inst.clear_file_specific_paths()
    return paths, timings, how


def _same_samples(flac_paths, wav_paths, bits):
    assert len(flac_paths) == len(wav_paths) >= 2
    for fp, wp in zip(flac_paths, wav_paths):
        assert fp.endswith(".flac") and wp.endswith(".wav")
        with open(fp, "rb") as f:
            info, got, _ = F.decode(f.read())
        want, wav_bits = _read_wav_ints(wp)
        assert info["bits_per_sample"] == bits and wav_bits == bits
        assert info["total_samples"] == want.shape[0] and np.array_equal(got, want)


@pytest.mark.parametrize("subtype,bits", [("PCM_16", 16), ("PCM_24", 24)])
def test_mdx_separate_writes_flac(tmp_path, monkeypatch, subtype, bits):
    from audio_separator_amd import audio_io
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    case = SC.cases("mdx", str(tmp_path))[0]
    x, sr = audio_io.read_wav(case[4])
    src = str(tmp_path / f"in_{subtype}.wav")
    audio_io.write_wav(src, np.ascontiguousarray(x.T), sr, subtype)
    flacs, t, how = _separate(case, src, "FLAC")
    assert how == "flac_device_resident" and t.get("flac_encode", 0.0) > 0.0
    wavs, t_wav, _ = _separate(case, src, "WAV")
    assert "flac_encode" not in t_wav
    _same_samples(flacs, wavs, bits)
    # the stems' MD5 is "not computed": their samples never reached the host
    with open(flacs[0], "rb") as f:
        assert F.parse_container(f.read())[0]["md5"] == bytes(16)


def test_synchronous_writes_and_the_upload_path(tmp_path, monkeypatch):
    """ASX_ASYNC_WRITES=0, and a stem that is a host array (the file fast path off): quantised as before, its int16 uploaded, MD5 set"""
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    case = SC.cases("mdx", str(tmp_path))[0]
    flacs, t, how = _separate(case, case[4], "FLAC")
    assert how == "flac_device_upload" and t.get("flac_encode", 0.0) > 0.0
    wavs, _, _ = _separate(case, case[4], "WAV")
    _same_samples(flacs, wavs, 16)
    with open(flacs[0], "rb") as f:
        info, got, _ = F.decode(f.read())
    assert info["md5"] == hashlib.md5(F.pcm_bytes(got, 16)).digest()


def test_planar_stems_write_flac(tmp_path, monkeypatch):
    """MDXC stems are planar [2, N] in HBM: asx_pcm16_dev, then the encoder"""
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    case = SC.cases("mdxc", str(tmp_path))[0]
    flacs, t, how = _separate(case, case[4], "FLAC")
    assert how == "flac_device_resident" and t.get("flac_encode", 0.0) > 0.0
    wavs, _, _ = _separate(case, case[4], "WAV")
    _same_samples(flacs, wavs, 16)


def test_mp3_still_needs_pydub(tmp_path):
    from audio_separator_amd import audio_io
    if audio_io._optional("pydub") is not None:
        pytest.skip("pydub is installed")
    case = SC.cases("mdx", str(tmp_path))[0]
    with pytest.raises(audio_io.AudioIOError, match="pydub"):
        _separate(case, case[4], "MP3")


def test_ensemble_separate_writes_flac(tmp_path, monkeypatch):
    import audio_separator_amd as A
    monkeypatch.delenv("ASX_OUTPUT_ENCODER", raising=False)
    tmp = str(tmp_path)
    wav = os.path.join(SC.AUDIO, "mdx_in.wav")

    def members(fmt):
        out = []
        for case in (SC.cases("mdx", tmp)[0], SC.cases("mdxc", tmp)[1]):
            _, cls, common, arch, _, _ = case
            out.append(SC.plugin_class(cls)(common_config=dict(common, output_format=fmt), arch_config=arch))
        return out
    results = {}
    for fmt in ("FLAC", "WAV"):
        ens = A.EnsembleSeparator(members(fmt), "avg_wave")
        ens.output_dir = str(tmp_path / fmt)
        results[fmt] = ens.separate(wav)
        assert ens.last_path_taken == "device"
        if fmt == "FLAC":
            assert ens.members[-1].last_write_path == "flac_device_resident" and ens.members[-1].file_timings.get("flac_encode", 0.0) > 0.0
    _same_samples(results["FLAC"], results["WAV"], 16)
