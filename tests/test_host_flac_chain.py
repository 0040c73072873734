"""The host side of the FLAC decoder (csrc/flac_dec_plan.h, no GPU): the walk that picks the stream's frames out of the candidate records,
and the refusals of the plan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("flacchain") / "flac_chain_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-o", out,
                    os.path.join(ROOT, "tests", "host", "flac_chain_host.cpp")], check=True)
    return out


def chain(exe, audio_bytes, recs):
    """recs: [(pos, end, blocksize, assignment, ok)] -> (n_samples, n_frames, bytes_consumed, [(index, out)])"""
    r = subprocess.run([exe, "chain", str(audio_bytes)] + [str(v) for rec in recs for v in rec], capture_output=True, text=True, check=True)
    rows = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    return rows[0][0], rows[0][1], rows[0][2], list(rows[1:])


def test_straight_chain(exe):
    recs = [(0, 100, 4096, 1, 1), (100, 250, 4096, 10, 1), (250, 300, 17, 8, 1)]
    assert chain(exe, 300, recs) == (8209, 3, 300, [(0, 0), (1, 4096), (2, 8192)])


def test_unordered_input(exe):
    recs = [(250, 300, 17, 8, 1), (0, 100, 4096, 1, 1), (100, 250, 4096, 10, 1)]
    assert chain(exe, 300, recs) == (8209, 3, 300, [(1, 0), (2, 4096), (0, 8192)])


def test_off_chain_candidate_inside_a_frame_is_dropped(exe):
    # candidate 1 is a whole valid frame within frame 0 (a VERBATIM subframe spelling one), candidate 3 one that runs across a boundary
    recs = [(0, 100, 192, 1, 1), (7, 21, 192, 1, 1), (100, 250, 192, 1, 1), (90, 130, 16, 1, 1), (250, 300, 192, 1, 1)]
    assert chain(exe, 300, recs) == (576, 3, 300, [(0, 0), (2, 192), (4, 384)])


def test_break(exe):
    # the frame at 100 failed its CRC-16; the one at 250 is intact but unreachable
    recs = [(0, 100, 4096, 1, 1), (100, 250, 4096, 1, 0), (250, 300, 4096, 1, 1)]
    assert chain(exe, 300, recs) == (4096, 1, 100, [(0, 0)])
    # no candidate at all where the next frame should begin; trailing bytes behind the last frame
    assert chain(exe, 300, [(0, 100, 4096, 1, 1), (101, 250, 4096, 1, 1)]) == (4096, 1, 100, [(0, 0)])
    assert chain(exe, 428, [(0, 100, 4096, 1, 1), (100, 300, 4096, 1, 1)]) == (8192, 2, 300, [(0, 0), (1, 4096)])


def test_no_candidate_at_byte_0(exe):
    assert chain(exe, 300, [(1, 100, 4096, 1, 1), (100, 300, 4096, 1, 1)]) == (0, 0, 0, [])
    assert chain(exe, 300, [(0, 100, 4096, 1, 0), (100, 300, 4096, 1, 1)]) == (0, 0, 0, [])


def test_empty_list(exe):
    assert chain(exe, 300, []) == (0, 0, 0, [])


def test_two_candidates_at_one_position(exe):
    # the one that is ok is taken; of two that are ok, the one listed first
    assert chain(exe, 300, [(0, 120, 16, 1, 0), (0, 100, 4096, 1, 1), (100, 300, 4096, 1, 1)]) == (8192, 2, 300, [(1, 0), (2, 4096)])
    assert chain(exe, 300, [(0, 100, 4096, 1, 1), (0, 120, 16, 1, 1), (100, 300, 4096, 1, 1)]) == (8192, 2, 300, [(0, 0), (2, 4096)])


def test_records_that_cannot_be_frames_are_ignored(exe):
    # an end at or before the start, an end past the data, no samples: never links (and never loops)
    assert chain(exe, 300, [(0, 0, 4096, 1, 1)]) == (0, 0, 0, [])
    assert chain(exe, 300, [(0, 400, 4096, 1, 1)]) == (0, 0, 0, [])
    assert chain(exe, 300, [(0, 100, 0, 1, 1)]) == (0, 0, 0, [])


def plan(exe, *args):
    return subprocess.run([exe, "plan"] + [str(a) for a in args], capture_output=True, text=True)


def test_plan_sizes_and_refusals(exe):
    r = plan(exe, 1000, 2, 16, 4096, 0)
    assert r.returncode == 0 and r.stdout.split() == ["201", str(2 * 4096 * 4), str(16 + 201 * 4 + 201 * 20)]
    for args, word in (((1000, 2, 32, 4096, 0), "bits per sample"), ((1000, 3, 16, 4096, 0), "channels"), ((1000, 2, 16, 16385, 0), "block size"),
                       ((1000, 2, 16, 15, 0), "block size"), ((0, 2, 16, 4096, 0), "empty"), ((1000, 2, 7, 4096, 0), "bits per sample")):
        r = plan(exe, *args)
        assert r.returncode == 1 and word in r.stdout, (args, r.stdout)
    for args in ((1000, 1, 8, 16, 0), (1000, 2, 24, 16384, 70000)):
        assert plan(exe, *args).returncode == 0
