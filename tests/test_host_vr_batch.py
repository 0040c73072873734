"""The pool plan of asx_vr_separate_batch_dev as the library builds it (csrc/vr_pool_plan.h, no GPU) against the arithmetic of
oracle.vr_oracle: frames per band as loading_mix gets them (1 + len // hl of a centred STFT, lengths through resample_poly's
ceil(n * up / down)), the shortest band deciding, and the patch count of make_padding.  Everything is integer arithmetic, so
every number is compared for equality.  Plus the CPU-side facts of the feature: which plugins publish ``separate_many`` and that
include/asx.h is still plain C with the new struct."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from oracle import vr_oracle as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vrpool") / "vr_pool_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "vr_pool_host.cpp")], check=True)
    return exe


def even_batches(nk, max_b):
    """engine: the fewest batches of at most max_b, evened out"""
    nbatch = -(-nk // max_b)
    return -(-nk // nbatch)


def run_pool(exe, mp, window, offset, max_batch, lengths, high_end=False):
    bands = mp.param["band"]
    nb = len(bands)
    args = [exe, window, offset, max_batch, int(high_end), bands[nb]["crop_stop"], mp.param["pre_filter_start"], mp.param["pre_filter_stop"], nb]
    for d in range(1, nb + 1):
        args += [bands[d]["sr"], bands[d]["hl"], bands[d]["n_fft"]]
    return subprocess.run([str(a) for a in args] + [str(n) for n in lengths], capture_output=True, text=True)


def parse(out):
    rows = [line.split() for line in out.splitlines()]
    head = [r for r in rows if r[0] == "plan"]
    assert len(head) == 1
    plan = tuple(int(v) for v in head[0][1:])                                     # roi, he_rows, frames, per plain, per tta
    songs = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "song"]       # T, n_out, patches, frame0
    flat = {kind: [(int(r[2]), int(r[3])) for r in rows if r[0] == "patch" and r[1] == kind] for kind in ("plain", "tta")}
    passes = {"plain": [], "tta": []}                                             # kind -> [(j0, B, [(song, k0, slot0, count)])]
    cur = None
    for r in rows:
        if r[0] == "pass":
            cur = (int(r[2]), int(r[3]), [])
            passes[r[1]].append(cur)
        elif r[0] == "run":
            cur[2].append(tuple(int(v) for v in r[1:]))
    return plan, songs, flat, passes


def oracle_song(mp, n, window, offset):
    """-> T, n_out, patches of one song, by the oracle's own functions where it has them"""
    bands = mp.param["band"]
    nb = len(bands)
    length, frames = n, []
    for d in range(nb, 0, -1):
        if d < nb:
            # lr_resample(polyphase) = scipy.signal.resample_poly: ceil(len * target / orig) samples
            ratio = Fraction(bands[d]["sr"], bands[d + 1]["sr"])
            length = -((-length * ratio.numerator) // ratio.denominator)
        frames.append(1 + length // bands[d]["hl"])                               # lr_stft: centred, 1 + len // hop
    T = min(frames)                                                               # combine_spectrograms
    pad_l, pad_r, roi = V.make_padding(T, window, offset)
    patches = (T + pad_l + pad_r - 2 * offset) // roi                            # inference_vr._execute
    return T, bands[nb]["hl"] * (T - 1), patches, roi


def test_frames_match_the_oracle_stft():
    """the frame arithmetic above against the oracle's loading_mix itself, on a few lengths"""
    mp = V.small_params()
    for n in (129, 2047, 2048, 5000):
        X = V.loading_mix(np.zeros((2, n), np.float32), mp)
        assert X.shape[2] == oracle_song(mp, n, 64, 16)[0], n


@pytest.mark.parametrize("params", ["small", "small_v51", "two_band"])
@pytest.mark.parametrize("window,offset", [(64, 16), (32, 8), (48, 24 - 8), (16, 8)])
def test_pool_plan_equals_oracle(host_exe, params, window, offset):
    mp = {"small": V.small_params, "small_v51": V.small_params_v51,
          "two_band": lambda: V.ModelParams({"bins": 96, "band": {1: {"sr": 1500, "hl": 12, "n_fft": 128, "crop_start": 0, "crop_stop": 36},
                                                                  2: {"sr": 8000, "hl": 64, "n_fft": 192, "crop_start": 4, "crop_stop": 64}},
                                             "sr": 8000, "pre_filter_start": 94, "pre_filter_stop": 96})}[params]()
    hl = mp.param["band"][len(mp.param["band"])]["hl"]
    rng = np.random.default_rng(window * 131 + offset)
    roi = window - 2 * offset or window
    checked = 0
    for max_batch in (0, 1, 3, 4, 7, 48):
        lengths = [int(v) for v in rng.integers(2 * hl, 40 * roi * hl // 4, size=int(rng.integers(1, 9)))]
        lengths += [hl * roi + 1, hl * roi - 1, 2 * hl]                           # around an exact multiple of roi frames; the minimum
        r = run_pool(host_exe, mp, window, offset, max_batch, lengths)
        assert r.returncode == 0, (r.stdout, r.stderr)
        plan, songs, flat, passes = parse(r.stdout)
        want = [oracle_song(mp, n, window, offset) for n in lengths]
        assert plan[0] == roi == want[0][3]
        frame0 = 0
        for got, (T, n_out, patches, _) in zip(songs, want):
            assert got == (T, n_out, patches, frame0), (lengths, got)
            frame0 += T
        assert len(songs) == len(lengths) and plan[2] == frame0
        for kind, extra in (("plain", 0), ("tta", 1)):
            # every (song, patch) exactly once, song-major
            assert flat[kind] == [(i, k) for i, w in enumerate(want) for k in range(w[2] + extra)]
            total = len(flat[kind])
            per = even_batches(total, max_batch if max_batch > 0 else 4)
            assert plan[3 if kind == "plain" else 4] == per
            sizes = [per] * (total // per) + ([total % per] if total % per else [])
            assert [(j0, B) for j0, B, _ in passes[kind]] == [(sum(sizes[:i]), b) for i, b in enumerate(sizes)]
            seen = []
            for j0, B, runs in passes[kind]:
                slot = 0
                for song, k0, slot0, count in runs:
                    assert slot0 == slot and count >= 1
                    seen += [(song, k0 + j) for j in range(count)]
                    slot += count
                assert slot == B
                assert all(a[0] != b[0] for a, b in zip(runs, runs[1:]))           # one run per song and pass
            assert seen == flat[kind]
            checked += 1
    assert checked == 12


def test_invalid_songs_are_reported_by_index(host_exe):
    mp = V.small_params()
    ok = 64 * 40
    r = run_pool(host_exe, mp, 64, 16, 3, [ok, ok, "null", ok])
    assert r.returncode == 3 and r.stdout.startswith("error song 2: null wave pointer"), r.stdout
    r = run_pool(host_exe, mp, 64, 16, 3, [ok, 63, ok])                          # one frame
    assert r.returncode == 3 and r.stdout.startswith("error song 1: input too short: 1 frames"), r.stdout
    r = run_pool(host_exe, mp, 64, 16, 3, [ok, 64, ok])                          # two frames: the minimum
    assert r.returncode == 0
    # high_end_process: the top band of small_params keeps 48 - 48 = 0 rows above its crop + 6 of the pre-filter ramp = 6 rows, which
    # fit below pre_filter_start - 10; the frame counts of the top band and the combined spectrogram must agree per song
    r = run_pool(host_exe, mp, 64, 16, 3, [ok, ok + 7], high_end=True)
    assert r.returncode == 0 and parse(r.stdout)[0][1] == 6, r.stdout
    squeezed = V.ModelParams(dict(mp.param, pre_filter_start=12))
    r = run_pool(host_exe, squeezed, 64, 16, 3, [ok], high_end=True)
    assert r.returncode == 3 and r.stdout.startswith("error song 0: high_end_process: 84 mirrored rows do not fit"), r.stdout
    r = run_pool(host_exe, mp, 64, 16, 3, [])                                     # an empty pool is a valid, empty plan
    assert r.returncode == 0 and parse(r.stdout)[0][2] == 0


def test_which_plugins_publish_separate_many():
    from audio_separator_amd.architectures.mdxc_separator import MDXCSeparator
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    from audio_separator_amd.common_separator import CommonSeparator
    assert VRSeparator.separate_many is CommonSeparator._separate_many
    assert not hasattr(MDXCSeparator, "separate_many")
    for hook in ("_prepare_model", "_pooled_stems", "_emit_file", "_load_mix"):
        assert hook in VRSeparator.__dict__, hook
    assert set(CommonSeparator._PER_FILE) < set(VRSeparator._PER_FILE)
    assert {"wav_subtype", "input_audio_subtype"} <= set(VRSeparator._PER_FILE)


def test_header_is_plain_c_with_the_song_struct(tmp_path):
    from audio_separator_amd import engine as E
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed for this check"
    src = ('#include <stdio.h>\n#include "asx.h"\nint main(void) {\n  asx_vr_song s = {0, 0, 0, 0};\n'
           '  int (*f)(asx_engine *, const asx_vr_song *, int32_t, const asx_vr_params *, void *) = asx_vr_separate_batch_dev;\n'
           '  printf("%zu %d %d\\n", sizeof(s), ASX_ABI_VERSION, ASX_VR_POOL_SEGMENTS);\n  return f == 0;\n}\n')
    c = tmp_path / "song.c"
    c.write_text(src)
    obj = tmp_path / "song.o"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(obj)],
                   check=True)
    assert C.sizeof(E._VrSong) == 32 and [n for n, _ in E._VrSong._fields_] == ["wave_dev", "n_samples", "primary_dev", "secondary_dev"]
    assert E.ABI_VERSION == 8 and "asx_vr_separate_batch_dev" in E.SYMBOLS
    assert E.VR_POOL_SEGMENTS == int(__import__("re").search(r"#define\s+ASX_VR_POOL_SEGMENTS\s+(\d+)", open(os.path.join(ROOT, "include", "asx.h")).read()).group(1))
