"""The chunk plan of Demucs' apply_model as the library builds it (csrc/apply_plan.h, no GPU) against the oracles' restatement of
apply.py:195-260: oracle.demucs_oracle.segment_plan for v4 (every chunk centred in a full segment) and
oracle.hdemucs_oracle.hd_segment_plan for v3 (every chunk at its own length).  Both sides truncate the same IEEE double product
for the stride and do integer arithmetic from there, so every number is compared for equality."""
import os
import subprocess
from fractions import Fraction

import pytest

from oracle.demucs_oracle import HTConfig, segment_plan
from oracle.hdemucs_oracle import HDConfig, hd_segment_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OVERLAPS = (0.0, 0.1, 0.25, 0.75, 0.99)
# (samplerate, segment in seconds): an even segment of 600 samples with max_shift 100, an odd one of 601 with max_shift 300
GEOMETRIES = ((200, 3), (601, 1))


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("applyplan") / "apply_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "apply_plan_host.cpp")], check=True)
    return exe


def run_plan(exe, n, seg, sr, overlap, centered, shifts, offsets):
    args = [exe, str(n), str(seg), str(sr), repr(float(overlap)), str(int(centered)), str(shifts)] + [str(o) for o in offsets]
    return subprocess.run(args, capture_output=True, text=True)


def parse(out):
    rows = [line.split() for line in out.splitlines()]
    head = [r for r in rows if r[0] == "plan"]
    assert len(head) == 1 and len(rows) == 1 + sum(r[0] in ("shift", "chunk") for r in rows)
    stride, max_shift, segment = (int(v) for v in head[0][1:])
    shifts = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "shift"]     # offset, VL, first, nk
    chunks = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "chunk"]     # start, clen
    return stride, max_shift, segment, shifts, chunks


def reference(n, sr, seconds, overlap, centered, shifts, offsets):
    """-> stride, max_shift, segment, [(offset, VL, first, nk)], [(start, clen)] from the oracle of that generation"""
    if centered:
        plan, stride, max_shift = segment_plan(n, HTConfig(samplerate=sr, segment=Fraction(seconds)), shifts, offsets, overlap)
        seg = sr * seconds
    else:
        plan, stride, max_shift, seg = hd_segment_plan(n, HDConfig(samplerate=sr, segment=seconds), shifts, offsets, overlap)
    assert seg == sr * seconds
    per_shift, chunks = [], []
    for si in range(max(shifts, 1)):
        mine = [row for row in plan if row[0] == si]
        off, vl = mine[0][1], mine[0][2]
        per_shift.append((off, vl, len(chunks), len(mine)))
        for (_, off, vl, o, clen) in mine:
            chunks.append((off + o - ((seg - clen) // 2 if centered else 0) - max_shift, clen))
    return stride, max_shift, seg, per_shift, chunks


def shift_cases(max_shift):
    mid = max_shift // 3 + 1
    assert 0 < mid < max_shift
    return [(0, [])] + [(1, [o]) for o in (0, max_shift, mid)] + [(3, [0, max_shift, mid])]


@pytest.mark.parametrize("centered", [True, False], ids=["v4_centred", "v3_own_length"])
@pytest.mark.parametrize("overlap", OVERLAPS)
@pytest.mark.parametrize("sr,seconds", GEOMETRIES)
def test_plan_equals_oracle(host_exe, sr, seconds, overlap, centered):
    seg = sr * seconds
    stride = int((1 - overlap) * seg)
    assert 1 <= stride <= seg
    lengths = [seg // 2 - 7, 3 * stride - 1, 3 * stride, 3 * stride + 1]          # below one segment; a stride multiple and +- 1
    assert lengths[0] < seg and min(lengths) >= 2
    checked = 0
    for n in lengths:
        for shifts, offsets in shift_cases(sr // 2):
            r = run_plan(host_exe, n, seg, sr, overlap, centered, shifts, offsets)
            assert r.returncode == 0, (n, shifts, offsets, r.stdout, r.stderr)
            got = parse(r.stdout)
            want = reference(n, sr, seconds, overlap, centered, shifts, offsets)
            assert got[:3] == want[:3], (n, shifts, offsets)                        # stride, max_shift, segment
            assert got[3] == want[3], (n, shifts, offsets)                          # per shift: offset, VL, first, nk
            assert got[4] == want[4], (n, shifts, offsets)                          # every starts[k], clen[k]
            assert len(got[4]) == sum(s[3] for s in got[3]) > 0
            checked += 1
    assert checked == 4 * 5


@pytest.mark.parametrize("centered", [True, False], ids=["v4_centred", "v3_own_length"])
def test_rejected_plans(host_exe, centered):
    sr, seg = 200, 600
    for overlap in (1.0, 1.5):                                                      # stride 0, stride < 0
        r = run_plan(host_exe, 1000, seg, sr, overlap, centered, 0, [])
        assert r.returncode == 3 and r.stdout.startswith("error overlap") and "bad stride" in r.stdout, r.stdout
    for offsets in ([sr // 2 + 1], [0, sr // 2 + 1], [-1]):                         # outside [0, max_shift]
        r = run_plan(host_exe, 1000, seg, sr, 0.25, centered, len(offsets), offsets)
        assert r.returncode == 3 and f"outside [0, {sr // 2}]" in r.stdout, r.stdout
    r = run_plan(host_exe, 1000, seg, sr, 0.25, centered, 1, [sr // 2])             # the bound itself is a valid draw
    assert r.returncode == 0

