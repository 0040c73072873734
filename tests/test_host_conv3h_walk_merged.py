"""csrc/conv3h_walk_plan.h with merged output slices -- conv3h_kernel runs the n output slices of a 48 n-channel layer side by side in one
launch per input slice: the groups of workgroups are dealt into walkers of n groups that read one row of the walk table -- compiled with g++
into tests/host/conv3h_walk_merged_host.cpp, once plainly and once with -fsanitize=address,undefined.  The program walks the table the way the
kernel does (conv3h_walk_wg: workgroup -> row, output slice) and checks that every (item, strip, tile row) is taken exactly once per output
slice, that the map is a bijection onto the busy groups, and that n = 1 is the plan of before, entry for entry.  No GPU."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "conv3h_walk_merged_host.cpp")

# tests/test_gpu_conv3h_merged.py's shapes (T 4 / 6 / 12, F 32 / 64 / 288, B 1 / 3 / 11) in tiles, and 55 chunks of the HQ_3 geometry, levels 0 to 2
SHAPES = list(itertools.product((1, 3, 11), (1, 2, 3), (1, 2, 9))) + [(55, 64, 96), (55, 32, 48), (55, 16, 24)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conv3h_walk_merged") / f"conv3h_walk_merged_host_{request.param}")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", out, SRC], check=True)
    return out


@pytest.mark.parametrize("nob", [1, 2, 3, 4])
def test_every_tile_once_per_output_slice_and_the_map_is_a_bijection(exe, nob):
    r = subprocess.run([exe, "check", str(nob)] + [str(v) for s in SHAPES for v in s], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-600:], r.stderr[-2000:])
    lines = [[int(v) for v in ln.split()[1:]] for ln in r.stdout.splitlines() if ln.startswith("shape ")]
    assert len(lines) == 2 * len(SHAPES)                         # both schedules of every shape
    for mode, B, tT, tF, n, bw, walkers, longest, busy, groups in lines:
        assert n == nob and bw in (32, 16, 8) and groups == 256 // bw and walkers == groups // nob and busy == walkers * nob
        if nob in (1, 2, 4):
            assert busy == groups                                # a power of two: no group is left over
        # the lists hold every tile row of every (item, band) once, plus one step per unit: never shorter than the even share
        nbands = -(-tF // bw)
        assert longest * walkers >= B * nbands * tT


def test_benchmark_shapes(exe):
    """55 chunks, levels 1 to 3: wall steps per layer as n x n launches and merged; the program asserts level 1 <= 1368 and level 2 <= 843 and
    that 32 of 32 / 30 of 32 groups are busy."""
    r = subprocess.run([exe, "bench"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-600:], r.stderr[-2000:])
    got = {int(m.group(1)): (int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)))
           for m in re.finditer(r"level (\d): today \d+ x \d+ = (\d+) wall steps.*merged \d+ x \d+ = (\d+) \(bw \d+, (\d+) of (\d+) groups busy\)", r.stdout)}
    assert got[1][0] == 1368 and got[1][1] <= 1368 and got[1][2:] == (32, 32)
    assert got[2][0] == 810 and got[2][1] <= 843 and got[2][2:] == (30, 32)
    assert got[3][0] == 512
