"""The decoder of csrc/kernels_flac_dec.h compiled for the host (tools/flac_host_decode.cpp: the same text, the lanes of each phase run one
after another) as a stand-alone program under AddressSanitizer and UBSan, without a GPU: the three fixtures, every stream of
tests/flac_synth.py, and seeded single-bit flips and cuts of a fixture's first frames.  Every buffer of the program has exactly the size
the device's has, so a read or write past one -- in the parse of a false candidate or of a damaged frame -- ends the program with a
report.  What this cannot show is the device's own execution (barriers, the launches): tests/test_gpu_flac_decode.py does."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import flac_ref as F
from tests import flac_synth as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "flac")
FIXTURES = ("mardy20s_87.flac", "ref_levee_drums_vocals_8.flac", "sing_sing_sing_brass_178.flac")


def mutations(seed=20, n_flips=200, n_cuts=50, n_frames=10):
    """(name, audio bytes, frames that survive) of seeded single-bit flips and cuts within the first frames of mardy20s_87.flac"""
    data = open(os.path.join(GOLDEN, "mardy20s_87.flac"), "rb").read()
    info, _, first = F.parse_container(data)
    _, frames = F.decode_frames(data, info, first, max_frames=n_frames)
    starts = [f["offset"] - first for f in frames]
    end = starts[-1] + frames[-1]["size"]
    audio = data[first:first + end]
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_flips):
        bit = int(rng.integers(0, 8 * end))
        a = bytearray(audio)
        a[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((f"flip_{i}_{bit}", bytes(a), int(np.searchsorted(starts, bit >> 3, side="right")) - 1))
    for i in range(n_cuts):
        at = int(rng.integers(1, end))
        out.append((f"cut_{i}_{at}", audio[:at], int(np.searchsorted(starts[1:] + [end], at, side="right"))))
    return info, starts + [end], out


@pytest.fixture(scope="module")
def decoder(tmp_path_factory):
    gxx = shutil.which("g++") or shutil.which("c++")
    if not gxx:
        pytest.skip("no host C++ compiler")
    work = tmp_path_factory.mktemp("flac_host_dec")
    exe = str(work / "flac_host_decode")
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DASX_FLAC_HOST",
                    os.path.join(ROOT, "tools", "flac_host_decode.cpp"), "-o", exe], check=True)

    def run(jobs):
        """jobs: [(name, audio bytes, info)] -> [(mix int64 [2, n], n_frames, bytes_consumed)], one run of the program for all"""
        lines = []
        for i, (_, audio, info) in enumerate(jobs):
            src = str(work / f"{i}.audio")
            with open(src, "wb") as f:
                f.write(audio)
            lines.append(f"{src} {src}.f32 {info['samplerate']} {info['channels']} {info['bits_per_sample']} {info['max_blocksize']} "
                         f"{info['max_framesize']}")
        (work / "jobs.txt").write_text("\n".join(lines) + "\n")
        r = subprocess.run([exe, str(work / "jobs.txt")], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
        rows = [list(map(int, line.split())) for line in r.stdout.splitlines()]
        assert len(rows) == len(jobs)
        out = []
        for i, ((_, _, info), (n, nf, used, _)) in enumerate(zip(jobs, rows)):
            mix = np.fromfile(str(work / f"{i}.audio.f32"), np.float32).reshape(2, n).astype(np.float64) * (1 << (info["bits_per_sample"] - 1))
            assert np.array_equal(mix, np.round(mix))
            out.append((mix.astype(np.int64), nf, used))
        return out
    return run


def test_fixtures(decoder):
    jobs, want = [], []
    for name in FIXTURES:
        data = open(os.path.join(GOLDEN, name), "rb").read()
        info, pcm, frames = F.decode(data)
        first = frames[0]["offset"]
        jobs.append((name, data[first:], info))
        want.append((pcm.T, len(frames), len(data) - first))
    for (name, _, _), (mix, nf, used), (pcm, frames, nbytes) in zip(jobs, decoder(jobs), want):
        assert np.array_equal(mix, pcm) and (nf, used) == (frames, nbytes), name


def test_builder_streams(decoder):
    S = Y.streams()
    jobs = [(name, Y.audio(s), s["info"]) for name, s in sorted(S.items())]
    for (name, _, _), (mix, nf, used) in zip(jobs, decoder(jobs)):
        s = S[name]
        assert np.array_equal(mix, Y.planar(s)) and (nf, used) == (s["n_frames"], s["bytes_consumed"]), name


def test_flips_and_cuts(decoder):
    info, starts, muts = mutations()
    assert sum(m[0].startswith("flip") for m in muts) >= 200 and sum(m[0].startswith("cut") for m in muts) >= 50
    data = open(os.path.join(GOLDEN, "mardy20s_87.flac"), "rb").read()
    pcm = F.decode(data, max_frames=10)[1].T
    got = decoder([(name, audio, info) for name, audio, _ in muts])
    for (name, _, keep), (mix, nf, used) in zip(muts, got):
        assert nf == keep and used == starts[keep] and np.array_equal(mix, pcm[:, :keep * 4096]), name
