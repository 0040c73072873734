"""The int32 form of the block encoder of csrc/kernels_flac.h (asx_flac_encode_pcm_dev's: samples of 16 or 24 real bits, no wasted bits,
Rice method 1 where a partition needs a parameter above 14) compiled for the host -- tools/flac_host_encode.cpp with "pcm32" -- and decoded
by tests/flac_ref.py: samples equal exactly.  And the int16 form of the same text still writes, byte for byte, the frames it wrote before the
width became a parameter (tests/golden/flac_encode_digest.json: SHA-256 of the frames for tests/test_gpu_flac.py's CONTENTS at 16 and at
shifted 24 bits, block 4096, 44.1 kHz, written by the host build of the commit before)."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import flac_wide_cases as W
from tests.test_gpu_flac import CONTENTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def encoder(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("flac_host_wide") / "flac_host_encode")
    subprocess.run([gxx, "-O2", "-std=c++17", "-DASX_FLAC_HOST", os.path.join(ROOT, "tools", "flac_host_encode.cpp"), "-o", exe], check=True)

    def run(pcm, rate, bits, block, tmp, pcm32=True):
        src, out, sizes = (str(tmp / n) for n in ("in.pcm", "out.frames", "out.sizes"))
        np.ascontiguousarray(pcm, np.int32 if pcm32 else np.int16).tofile(src)
        subprocess.run([exe, src, out, sizes, str(rate), str(bits), str(block)] + (["pcm32"] if pcm32 else []), check=True)
        with open(out, "rb") as f:
            return f.read(), np.fromfile(sizes, np.int32)
    return run


@pytest.fixture(scope="module")
def decoded24(encoder, tmp_path_factory):
    """every 24-bit content at block 4096 (three full blocks and a short one), encoded and checked once"""
    tmp = tmp_path_factory.mktemp("wide24")
    out = {}
    for name, pcm in W.CONTENTS24.items():
        frames, sizes = encoder(pcm, W.RATE, 24, 4096, tmp)
        out[name] = (W.check_stream(frames, sizes, pcm, 24, 4096), len(frames))
    return out


def test_24_bit_contents_round_trip(decoded24):
    assert set(decoded24) == set(W.CONTENTS24)
    kinds = {name: {s["type"] for d in dec for s in d["subframes"]} for name, (dec, _) in decoded24.items()}
    assert kinds["silence"] == {"CONSTANT"} and kinds["constant_dc"] == {"CONSTANT"}
    assert kinds["white_noise_full_scale"] == {"VERBATIM"}


def test_no_wasted_bits_on_noise(decoded24):
    for name in W.NOISE:
        assert all(s["wasted"] == 0 for d in decoded24[name][0] for s in d["subframes"]), name


def test_method_1_where_a_partition_needs_more_than_14(decoded24):
    subs = [s for d in decoded24["noise_2^19"][0] for s in d["subframes"] if s["type"] in ("FIXED", "LPC")]
    assert any(s["method"] == 1 and max(p for p in s["params"] if p is not None) > 14 for s in subs)
    # ... and method 0, the smaller field, where none does: the -60 dBFS sine's residuals are a few bits
    subs = [s for d in decoded24["sine_-60dbfs"][0] for s in d["subframes"] if s["type"] in ("FIXED", "LPC")]
    assert subs and all(s["method"] == 0 and max(s["params"]) <= 14 for s in subs)
    assert all(s["partition_order"] <= 5 for dec, _ in decoded24.values() for d in dec for s in d["subframes"] if "method" in s and s["method"] == 1)


def test_the_sine_codes_below_verbatim(decoded24):
    dec, nbytes = decoded24["sine_-60dbfs"]
    verbatim = sum((2 * (8 + 24 * d["blocksize"]) + 7) // 8 for d in dec)
    assert nbytes < verbatim
    assert all(s["type"] in ("FIXED", "LPC") for d in dec for s in d["subframes"])


def test_side_channel_takes_25_bits(decoded24):
    """L = -R - 1 at full scale: whichever pair the frame takes, the samples come back; with a side channel its warm-up samples are 25 bits"""
    dec, _ = decoded24["square_near_nyquist_full_scale"]
    assert all(len(d["subframes"]) == 2 for d in dec)
    assert any(s["bits"] == 25 for dec, _ in decoded24.values() for d in dec for s in d["subframes"])


def test_16_bit_contents_round_trip(encoder, tmp_path):
    for name, pcm in CONTENTS.items():
        frames, sizes = encoder(pcm.astype(np.int32), W.RATE, 16, 4096, tmp_path)
        dec = W.check_stream(frames, sizes, pcm, 16, 4096)
        assert all(s["wasted"] == 0 for d in dec for s in d["subframes"]), name


@pytest.mark.parametrize("block,rate", [(16, 12345), (1000, 96000), (4608, 48000)])
def test_other_block_sizes(encoder, tmp_path, block, rate):
    for name in ("noise_2^19", "square_near_nyquist_full_scale", "sine_-60dbfs", "left_only"):
        pcm = W.CONTENTS24[name][:2 * 4608 + 5]
        frames, sizes = encoder(pcm, rate, 24, block, tmp_path)
        W.check_stream(frames, sizes, pcm, 24, block, rate)


def test_input_outside_the_sample_width_is_refused(encoder, tmp_path):
    with pytest.raises(subprocess.CalledProcessError):
        encoder(np.array([[1 << 23, 0]], np.int32), W.RATE, 24, 4096, tmp_path)


def test_int16_form_writes_the_frames_it_wrote_before(encoder, tmp_path):
    with open(os.path.join(ROOT, "tests", "golden", "flac_encode_digest.json")) as f:
        golden = json.load(f)
    want = golden["frames_sha256"]
    assert set(want) == {f"{name}/{bits}" for name in CONTENTS for bits in (16, 24)}
    for bits in (16, 24):
        for name, pcm in CONTENTS.items():
            frames, _ = encoder(pcm, golden["samplerate"], bits, golden["block_size"], tmp_path, pcm32=False)
            assert hashlib.sha256(frames).hexdigest() == want[f"{name}/{bits}"], (name, bits)
