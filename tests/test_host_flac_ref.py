"""CPU-side checks of the FLAC writer edge: the reference decoder of tests/flac_ref.py pinned on files other encoders wrote (ffmpeg,
libFLAC), asx_flac_plan (pure host) against the stride formula and its refusals, and the STREAMINFO bytes of audio_io.write_flac.

The fixtures under tests/golden/flac are frame-aligned prefixes, metadata blocks kept: the whole files are larger than a committed file
may be.  STREAMINFO's MD5 covers the whole stream, so each prefix is pinned by the MD5 of ITS samples instead, recorded from a decode of
the whole file whose MD5 matched STREAMINFO (sing_sing_sing_brass.flac: 240 frames, 1 386 248 bytes; mardy20s.flac: 216 frames,
2 478 894 bytes)."""
import hashlib
import os
import struct

import numpy as np
import pytest

import __graft_entry__ as entry
from audio_separator_amd import audio_io
from audio_separator_amd import engine as E
from tests import flac_ref as F

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac")
# file, writer's block size, frames, samples, audio-frame bytes, MD5 of the prefix's PCM
PREFIXES = [("sing_sing_sing_brass_178.flac", 4608, 178, 820224, 998221, "7987f4cfbf443f41c10426a67b910d6c"),
            ("mardy20s_87.flac", 4096, 87, 356352, 993089, "6f8474f8aec05a6dc540d419a79a5a84")]


def read(name):
    with open(os.path.join(FIX, name), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name,block,n_frames,n_samples,audio_bytes,md5", PREFIXES)
def test_decoder_on_files_of_other_encoders(name, block, n_frames, n_samples, audio_bytes, md5):
    """decode() verifies every frame's CRC-8 and CRC-16 (it raises on a mismatch); the samples are pinned by their MD5"""
    info, pcm, frames = F.decode(read(name))
    assert (info["bits_per_sample"], info["channels"], info["samplerate"]) == (16, 2, 44100)
    assert info["min_blocksize"] == info["max_blocksize"] == block
    assert len(frames) == n_frames and pcm.shape == (n_samples, 2)
    assert sum(f["size"] for f in frames) == audio_bytes
    assert [f["number"] for f in frames] == list(range(n_frames)) and all(f["blocksize"] == block for f in frames)
    assert info["min_framesize"] <= min(f["size"] for f in frames) and max(f["size"] for f in frames) <= info["max_framesize"]
    assert hashlib.md5(F.pcm_bytes(pcm, 16)).hexdigest() == md5
    kinds = {s["type"] for f in frames for s in f["subframes"]}
    assert "LPC" in kinds and {f["assignment"] for f in frames} >= {8, 9, 10}


def test_decoder_detects_damage():
    data = bytearray(read("ref_levee_drums_vocals_8.flac"))
    _, _, first = F.parse_container(bytes(data))
    data[first + 2] ^= 0x10                                  # the header: CRC-8
    with pytest.raises(F.FlacError, match="CRC-8"):
        F.decode(bytes(data))
    data[first + 2] ^= 0x10
    data[first + 40] ^= 0x01                                 # the body: CRC-16 (or a code that no longer parses)
    with pytest.raises((F.FlacError, IndexError)):
        F.decode(bytes(data))


def test_24_bit_prefix_wasted_bits():
    info, pcm, frames = F.decode(read("ref_levee_drums_vocals_8.flac"))
    assert info["bits_per_sample"] == 24 and len(frames) == 8 and pcm.shape == (8 * 4608, 2)
    assert all(s["wasted"] == 8 for f in frames for s in f["subframes"])
    assert np.all(pcm % 256 == 0) and np.abs(pcm).max() > 256 and np.abs(pcm).max() < 1 << 23


def test_fixed_only_counter_on_small_cases():
    """digital silence: two CONSTANT subframes per frame; white noise: two VERBATIM ones"""
    n, bs = 2 * 4096 + 100, 4096
    # header 4 + number 1 + CRC-8 1 (+ 1 for the last block's explicit size), subframes 2 x (8 + 16) bits, CRC-16 2
    assert F.fixed_only_bytes(np.zeros((n, 2), np.int64), bs) == 2 * (6 + 6 + 2) + (7 + 6 + 2)
    noise = np.random.default_rng(0).integers(-32768, 32768, (n, 2))
    assert F.fixed_only_bytes(noise, bs) == 2 * (6 + 2 * (1 + 2 * bs) + 2) + (7 + 2 * (1 + 2 * 100) + 2)


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return E.load_library()


def stride_formula(block):
    """header (at most 15 bytes) + 2 x (16 + 17 x block) bits + padding to a byte + CRC-16, rounded up to 16"""
    worst = 15 + (2 * (16 + 17 * block) + 7) // 8 + 2
    return worst, (worst + 15) // 16 * 16


@pytest.mark.parametrize("n,bits,block", [(1, 16, 4096), (4096, 16, 4096), (4097, 24, 4096), (3 * 4096 + 17, 16, 4096), (10_584_000, 24, 4096),
                                          (100_000, 16, 4608), (100, 16, 16), (5000, 24, 1152)])
def test_flac_plan(lib, n, bits, block):
    p = E.Engine.flac_plan(n, 2, bits, block)
    worst, stride = stride_formula(block)
    nb = -(-n // block)
    assert p["n_blocks"] == nb and p["frame_stride"] == stride and stride % 16 == 0
    assert p["max_bytes"] == (nb - 1) * worst + stride_formula(n - (nb - 1) * block)[0] <= nb * stride
    assert p["scratch_bytes"] == nb * stride + 8 * (nb + 1)


@pytest.mark.parametrize("n,channels,bits,block,why", [(1000, 1, 16, 4096, "channels"), (1000, 3, 16, 4096, "channels"), (1000, 2, 8, 4096, "bits"),
                                                        (1000, 2, 32, 4096, "bits"), (1000, 2, 16, 15, "block size"), (1000, 2, 16, 4609, "block size"),
                                                        (1000, 2, 16, 65536, "block size"), (0, 2, 16, 4096, "no samples"), (-5, 2, 16, 4096, "no samples")])
def test_flac_plan_refusals(lib, n, channels, bits, block, why):
    with pytest.raises(E.AsxError, match=why):
        E.Engine.flac_plan(n, channels, bits, block)
    assert lib.asx_flac_plan(n, channels, bits, block, None, None, None, None) != 0


def test_flac_encode_checks_arguments_without_a_device(lib):
    """null pointers are refused before the engine is touched"""
    assert lib.asx_flac_encode_dev(None, None, 10, 44100, 16, 4096, None, 0, None, None, None) != 0
    assert lib.asx_flac_encode(None, None, 10, 44100, 16, 4096, None, 0, None, None) != 0
    assert b"null argument" in lib.asx_last_error()


def test_write_flac_streaminfo_bytes(tmp_path):
    frames = bytes(range(200)) + bytes(57)
    sizes = [120, 80, 57]
    md5 = hashlib.md5(b"pcm").digest()
    path = str(tmp_path / "x.flac")
    audio_io.write_flac(path, frames, sizes, 44100, 24, 2 * 4096 + 9, md5, block_size=4096)
    data = open(path, "rb").read()
    assert data[:4] == b"fLaC" and data[4] == 0x80 and data[5:8] == b"\x00\x00\x22" and data[42:] == frames
    want = struct.pack(">HH", 4096, 4096) + (57).to_bytes(3, "big") + (120).to_bytes(3, "big") + \
        ((44100 << 44) | (1 << 41) | (23 << 36) | (2 * 4096 + 9)).to_bytes(8, "big") + md5
    assert data[8:42] == want
    info = F.parse_streaminfo(data[8:42])
    assert info == {"min_blocksize": 4096, "max_blocksize": 4096, "min_framesize": 57, "max_framesize": 120, "samplerate": 44100,
                    "channels": 2, "bits_per_sample": 24, "total_samples": 2 * 4096 + 9, "md5": md5}
    # numpy inputs, no MD5: sixteen zero bytes
    audio_io.write_flac(path, np.frombuffer(frames, np.uint8), np.asarray(sizes, np.int32), 48000, 16, 5000, None)
    data = open(path, "rb").read()
    assert F.parse_streaminfo(data[8:42])["md5"] == bytes(16) and data[42:] == frames
    assert audio_io.info(path) == {"samplerate": 48000, "channels": 2, "frames": 5000, "subtype": "PCM_16", "bits": 16} or \
        audio_io._optional("soundfile") is not None
    assert audio_io._optional("soundfile") is not None or audio_io.duration(path) == pytest.approx(5000 / 48000)
    with pytest.raises(audio_io.AudioIOError, match="size table"):
        audio_io.write_flac(path, frames, [1, 2], 44100, 16, 100)
    with pytest.raises(audio_io.AudioIOError, match="md5"):
        audio_io.write_flac(path, frames, sizes, 44100, 16, 100, b"short")


def test_info_reads_streaminfo_of_a_reference_file():
    if audio_io._optional("soundfile") is not None:
        pytest.skip("soundfile answers info()")
    i = audio_io.info(os.path.join(FIX, "ref_levee_drums_vocals_8.flac"))
    assert (i["samplerate"], i["channels"], i["subtype"]) == (44100, 2, "PCM_24") and i["frames"] > 8 * 4608
