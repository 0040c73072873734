"""Inputs of the FLAC encoder's int32 form (asx_flac_encode_pcm*: samples of 16 or 24 real bits), shared by the host-compiled kernel's test
and the device's: int32 [n, 2] at 24 bits, and the int16 contents of tests/test_gpu_flac.py for the 16-bit stream."""
import numpy as np

from tests.test_gpu_flac import CONTENTS

N3 = 3 * 4096 + 17
RATE = 44100
TOP = (1 << 23) - 1


def _contents24():
    rng = np.random.default_rng(24)
    t = np.arange(N3)
    c = {}
    c["silence"] = np.zeros((N3, 2))
    c["constant_dc"] = np.stack([np.full(N3, 1234567), np.full(N3, -7654321)], 1)
    s = np.rint(1e-3 * TOP * np.sin(2 * np.pi * 440 * t / RATE))                 # -60 dBFS
    c["sine_-60dbfs"] = np.stack([s, np.roll(s, 11)], 1)
    alt = np.where(t % 2 == 0, TOP, -TOP - 1)
    c["square_near_nyquist_full_scale"] = np.stack([alt, -alt - 1], 1)           # S = +-(2^24 - 1): 25 bits
    c["left_only"] = np.stack([rng.integers(-TOP - 1, TOP + 1, N3), np.zeros(N3, np.int64)], 1)
    c["left_only"][:4, 0] = (-TOP - 1, TOP, -TOP - 1, TOP)
    c["noise_2^19"] = rng.integers(-(1 << 19), (1 << 19) + 1, (N3, 2))
    c["white_noise_full_scale"] = rng.integers(-TOP - 1, TOP + 1, (N3, 2))
    for n in (1, 17, 4097):
        c[f"noise_2^12_{n}"] = rng.integers(-4096, 4097, (n, 2))
    return {k: np.ascontiguousarray(v, np.int32) for k, v in c.items()}


CONTENTS24 = _contents24()
NOISE = ("noise_2^19", "white_noise_full_scale")
# (name, bits, int32 [n, 2])
CASES = [(k, 24, v) for k, v in CONTENTS24.items()] + [(k, 16, v.astype(np.int32)) for k, v in CONTENTS.items()]


def worst_frame(block, bits):
    """header + 2 x (16 + (bits + 1) x block) bits + padding + CRC-16"""
    return 15 + (2 * (16 + (bits + 1) * block) + 7) // 8 + 2


def check_stream(frames, sizes, pcm, bits, block, rate=RATE):
    """decode with tests/flac_ref.py (every CRC verified), samples equal exactly; the frames as the sizes table says; returns the frames' dicts"""
    from tests import flac_ref as F
    got, decoded = F.decode_frames(bytes(frames), {"bits_per_sample": bits, "samplerate": rate})
    assert got.shape == pcm.shape and np.array_equal(got, pcm.astype(np.int64))
    assert [d["size"] for d in decoded] == list(map(int, sizes)) and sum(map(int, sizes)) == len(bytes(frames))
    n = pcm.shape[0]
    assert [d["blocksize"] for d in decoded] == [block] * (n // block) + ([n % block] if n % block else [])
    assert all(d["bits_per_sample"] == bits and d["samplerate"] == rate for d in decoded)
    assert max(map(int, sizes)) <= worst_frame(block, bits)
    return decoded
