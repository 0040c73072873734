"""The block encoder of csrc/kernels_flac.h compiled for the host (tools/flac_host_encode.cpp: the same text, the lanes of each phase run
one after another), without a GPU: its integer arithmetic, predictor and Rice choices, bit packing and CRCs, decoded by tests/flac_ref.py.
What this cannot show is the device's own execution (barriers, LDS atomics, the launch): tests/test_gpu_flac.py does."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import flac_ref as F
from tests.test_gpu_flac import CONTENTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def encoder(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("flac_host") / "flac_host_encode")
    subprocess.run([gxx, "-O2", "-std=c++17", "-DASX_FLAC_HOST", os.path.join(ROOT, "tools", "flac_host_encode.cpp"), "-o", exe], check=True)

    def run(pcm, rate, bits, block, tmp):
        src, out, sizes = (str(tmp / n) for n in ("in.s16", "out.frames", "out.sizes"))
        np.ascontiguousarray(pcm, np.int16).tofile(src)
        subprocess.run([exe, src, out, sizes, str(rate), str(bits), str(block)], check=True)
        with open(out, "rb") as f:
            return f.read(), np.fromfile(sizes, np.int32)
    return run


@pytest.mark.parametrize("bits", [16, 24])
def test_host_compiled_kernel_round_trips(encoder, tmp_path, bits):
    for name, pcm in CONTENTS.items():
        frames, sizes = encoder(pcm, 44100, bits, 4096, tmp_path)
        got, decoded = F.decode_frames(frames, {"bits_per_sample": bits, "samplerate": 44100})
        assert np.array_equal(got, pcm.astype(np.int64) << (bits - 16)), name
        assert [d["size"] for d in decoded] == sizes.tolist(), name
        worst = 15 + (2 * (16 + 17 * 4096) + 7) // 8 + 2
        assert sizes.max() <= worst, name


def test_host_compiled_kernel_other_blocks(encoder, tmp_path):
    pcm = CONTENTS["near_nyquist_full_scale"]
    for block, rate in ((4608, 48000), (16, 12345), (1000, 96000)):
        frames, sizes = encoder(pcm, rate, 16, block, tmp_path)
        got, decoded = F.decode_frames(frames, {"bits_per_sample": 16, "samplerate": rate})
        assert np.array_equal(got, pcm) and all(d["samplerate"] == rate for d in decoded)
        assert any(s["type"] == "LPC" for d in decoded for s in d["subframes"]) or block == 16
