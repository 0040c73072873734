"""csrc/conv3h_walk_plan.h -- the host planner of conv3h_kernel's walk table (which group of workgroups takes which tile rows of which band of
which batch item, in which order) -- compiled with g++ into tests/host/conv3h_walk_host.cpp, once plainly and once with
-fsanitize=address,undefined: coverage, unit validity, the arithmetic walk of schedule 0 against its formula restated here, and the step
counts of the balanced schedule.  No GPU."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "conv3h_walk_host.cpp")

BS = (1, 2, 3, 7, 9, 11, 55)
TILES_T = (1, 3, 4, 16, 32, 64)
TILES_F = (1, 2, 9, 24, 48, 96)
SHAPES = list(itertools.product(BS, TILES_T, TILES_F))


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("conv3h_walk") / f"conv3h_walk_host_{request.param}")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", out, SRC], check=True)
    return out


def plans(exe, gran, mode, shapes):
    """{(B, tilesT, tilesF): (bw, tps, ngroups, longest, [units of group g as (b, band, t0, tiles)])}; the program has checked the table."""
    r = subprocess.run([exe, "plan", str(gran), str(mode)] + [str(v) for s in shapes for v in s], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-2000:])
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        if ln.startswith("plan "):
            B, tT, tF, bw, tps, ng, longest, _ = (int(v) for v in ln.split()[1:])
            cur = (bw, tps, ng, longest, [[] for _ in range(ng)])
            out[(B, tT, tF)] = cur
        elif ln == "table ok":
            cur = None
        else:
            g, b, band, t0, tiles = (int(v) for v in ln.split())
            cur[4][g].append((b, band, t0, tiles))
    assert len(out) == len(shapes)
    return out


def parent_walk(B, tilesT, tilesF):
    """The arithmetic walk as the kernel computed it before the table: the band-width chooser of conv_launch, tps = tilesT bw / 32, XCD x =
    workgroup & 7 takes items x, x + 8, ..., workgroup l = workgroup >> 3 of the XCD segment l // bw.  -> bw, tps, {(x, seg): units}."""
    bw, best = 32, 1e30
    for cand in (32, 16, 8):
        if (tilesT * cand) % 32:
            continue
        tps = tilesT * cand // 32
        bands = -(-tilesF // cand)
        items = B * bands
        cost = (bands * cand) / tilesF * (tps + 1.0) / tps * float((items + 7) // 8) / (items / 8.0)
        if cost < best - 1e-9:
            best, bw = cost, cand
    if best > 1e29:
        bw = 32
    tps = tilesT * bw // 32 if (tilesT * bw) % 32 == 0 else tilesT
    nbands = -(-tilesF // bw)
    items = B * nbands
    walk = {}
    for x in range(8):
        for seg in range(32 // bw):
            walk[(x, seg)] = [(item // nbands, item % nbands, seg * tps, tps) for item in range(x, items, 8)]
    return bw, tps, walk


def steps(units):
    return sum(t + 1 for (_, _, _, t) in units)


def check_cover(B, tilesT, tilesF, plan, gran):
    bw, _, ng, longest, groups = plan
    assert bw in (32, 16, 8) and ng == 256 // bw
    nbands = -(-tilesF // bw)
    seen = set()
    for units in groups:
        for (b, band, t0, tiles) in units:
            assert 0 <= b < B and 0 <= band < nbands and tiles >= 1 and t0 >= 0 and t0 + tiles <= tilesT, (b, band, t0, tiles)
            assert t0 % gran == 0, "a unit starts where the exponent rule does not allow it"
            for t in range(t0, t0 + tiles):                      # contiguous in T by construction; every (b, band, tile) once -> every strip once
                assert (b, band, t) not in seen
                seen.add((b, band, t))
    assert len(seen) == B * nbands * tilesT
    assert longest == max(steps(u) for u in groups)


@pytest.mark.parametrize("gran", [1, 4])
def test_every_tile_is_walked_once_and_balanced_is_never_longer(exe, gran):
    p0 = plans(exe, gran, 0, SHAPES)
    p1 = plans(exe, gran, 1, SHAPES)
    for s in SHAPES:
        check_cover(*s, p0[s], 1)                                # (schedule 0 starts its segments where the formula puts them)
        check_cover(*s, p1[s], gran)
        if gran == 1:                                            # (the kernel's granularity; schedule 0 itself ignores a coarser one)
            assert p1[s][3] <= p0[s][3], (s, p1[s][3], p0[s][3])


def test_schedule_0_is_the_arithmetic_walk(exe):
    p0 = plans(exe, 1, 0, SHAPES)
    for s in SHAPES:
        bw, tps, walk = parent_walk(*s)
        gbw, gtps, ng, longest, groups = p0[s]
        assert (gbw, gtps, ng) == (bw, tps, 8 * (32 // bw)), s
        for (x, seg), units in walk.items():
            assert groups[x * (32 // bw) + seg] == units, (s, x, seg)
        # conv3h_nblocks of the kernel it replaces
        nbands = -(-s[2] // bw)
        items = s[0] * nbands
        assert longest == -(-items // 8) * (tps + 1)


@pytest.mark.parametrize("gran", [1, 4])
def test_benchmark_shapes(exe, gran):
    """55 chunks of the HQ_3 geometry, levels 0 to 2: the arithmetic walk's 1365 / 357 / 105 steps against at most 1345 / 345 / 92."""
    shapes = [(55, 64, 96), (55, 32, 48), (55, 16, 24)]
    p1 = plans(exe, gran, 1, shapes)
    for s, parent, bound in zip(shapes, (1365, 357, 105), (1345, 345, 92)):
        bw, tps, walk = parent_walk(*s)
        assert max(steps(u) for u in walk.values()) == parent
        print(f"{s}: {p1[s][3]} steps (bw {p1[s][0]}) against {parent} (bw {bw})")
        assert p1[s][3] <= bound
