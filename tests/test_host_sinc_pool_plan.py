"""The plan of asx_resample_sinc_batch_dev as the library builds it (csrc/sinc_pool_plan.h through tests/host/sinc_pool_plan_host.cpp;
no GPU) against a Python restatement: per job the frames the converter generates -- python-samplerate's int(n_in * ratio), one fewer
for a one-channel call whose n_in * ratio is an integer, never more than n_out -- and the prefix of 256-output workgroups; every
refusal by its message; the C surface (struct, prototype, ABI 7, the Python mirror)."""
import ctypes as C
import math
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH = [2.0 ** (s / 12) for s in (2, -2, 7, -7)]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sincpool") / "sinc_pool_plan_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                    os.path.join(ROOT, "tests", "host", "sinc_pool_plan_host.cpp")], check=True)
    return exe


def run_plan(exe, ratio, mono_calls, jobs):
    args = [exe, float(ratio).hex(), str(int(mono_calls))] + [j if isinstance(j, str) else ":".join(str(v) for v in j) for j in jobs]
    return subprocess.run(args, capture_output=True, text=True)


def expected_plan(ratio, mono_calls, jobs):
    rows, blk0, widest = [], 0, 0
    for n_in, n_out, channels in jobs:
        t = n_in * ratio                                   # one IEEE product, as the library's (double)n_in * ratio
        n_gen = int(t)
        if (mono_calls or channels == 1) and n_gen == t and n_gen > 0:
            n_gen -= 1
        blocks = -(-n_out // 256)
        rows.append((min(n_gen, n_out), blocks, blk0))
        blk0 += blocks
        widest = max(widest, channels)
    return (blk0, widest), rows


def parse_plan(out):
    rows = [line.split() for line in out.splitlines()]
    head = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "plan"]
    assert len(head) == 1
    return head[0], [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "job"]


def ceil_len(n, ratio):
    return int(math.ceil(n * ratio))


def jobs_for(ratio):
    """n_out of 1, 255, 256, 257; n_out below and above ceil(n_in * ratio); one, two and eight channels"""
    jobs = [(1000, n_out, 2) for n_out in (1, 255, 256, 257)]
    for n_in, channels in ((1, 1), (2, 2), (255, 8), (256, 1), (257, 2), (1000, 1), (4999, 8)):
        c = ceil_len(n_in, ratio)
        jobs += [(n_in, c, channels), (n_in, max(1, c - 3), channels), (n_in, c + 300, channels)]
    return jobs


@pytest.mark.parametrize("ratio", PITCH + [0.5, 2.0])
@pytest.mark.parametrize("mono_calls", [False, True])
def test_plan_equals_the_restatement(host_exe, ratio, mono_calls):
    for jobs in (jobs_for(ratio), jobs_for(ratio)[::-1], jobs_for(ratio)[5:6], []):
        r = run_plan(host_exe, ratio, mono_calls, jobs)
        assert r.returncode == 0, (r.stdout, r.stderr)
        got = parse_plan(r.stdout)
        assert got == expected_plan(ratio, mono_calls, jobs), (ratio, mono_calls, jobs)
        totals, rows = got
        assert sum(r[1] for r in rows) == totals[0]        # every workgroup belongs to exactly one job, in job order
        assert all(r[2] == sum(q[1] for q in rows[:j]) for j, r in enumerate(rows))


def test_exact_products_drop_a_frame_only_in_one_channel_calls(host_exe):
    """n_in * ratio an integer (ratio 0.5 and 2.0): the one-channel call -- one channel, or ``mono_calls`` -- generates one frame fewer"""
    for ratio, n_in, whole in ((0.5, 1000, 500), (2.0, 1000, 2000), (2.0, 1, 2)):
        jobs = [(n_in, whole, 1), (n_in, whole, 2), (n_in, whole + 44, 2), (n_in, whole - 1, 2)]
        _, plain = parse_plan(run_plan(host_exe, ratio, False, jobs).stdout)
        _, mono = parse_plan(run_plan(host_exe, ratio, True, jobs).stdout)
        assert [r[0] for r in plain] == [whole - 1, whole, whole, whole - 1]
        assert [r[0] for r in mono] == [whole - 1, whole - 1, whole - 1, whole - 1]
    # an odd n_in at ratio 0.5 is no integer product: int() alone
    _, rows = parse_plan(run_plan(host_exe, 0.5, True, [(1001, 501, 2), (1, 1, 1)]).stdout)
    assert [r[0] for r in rows] == [500, 0]


def test_refusals_name_the_job(host_exe):
    ok = (100, 100, 2)
    cases = [
        ([ok, "100:100:2:nox"], 1.5, "error job 1: null input or output"),
        (["100:100:2:noy", ok], 1.5, "error job 0: null input or output"),
        ([ok, ok, (0, 100, 2)], 1.5, "error job 2: n_in = 0 (1 .. 2^40)"),
        ([(100, 0, 2)], 1.5, "error job 0: n_out = 0 (1 .. 2^40)"),
        ([(100, -5, 2)], 1.5, "error job 0: n_out = -5 (1 .. 2^40)"),
        ([((1 << 40) + 1, 100, 2)], 1.5, f"error job 0: n_in = {(1 << 40) + 1} (1 .. 2^40)"),
        ([ok, (100, 100, 0)], 1.5, "error job 1: 0 channels (1 .. 65535)"),
        ([(100, 100, 65536)], 1.5, "error job 0: 65536 channels (1 .. 65535)"),
        ([ok], 1.0 / 256, "error ratio 0.00390625 outside libsamplerate's (1/256, 256)"),
        ([ok], 256.0, "error ratio 256 outside libsamplerate's (1/256, 256)"),
        ([ok], float("nan"), "error ratio nan outside libsamplerate's (1/256, 256)"),
        (["many=65536"], 1.5, "error 65536 jobs in one call (at most 65535)"),
        (["nolist"], 1.5, "error null job list"),
        ([(100, 1 << 40, 1), (100, 1 << 40, 1)], 1.5, f"error job 0: the jobs up to this one make {1 << 32} workgroups (2^31 - 1 at most)"),
    ]
    for jobs, ratio, text in cases:
        r = run_plan(host_exe, ratio, True, jobs)
        assert r.returncode == 3 and r.stdout.startswith(text), (jobs, r.stdout)
    # the limits themselves pass
    assert run_plan(host_exe, 1.5, True, ["many=65535"]).returncode == 0
    assert run_plan(host_exe, 255.9, True, [(100, 100, 65535)]).returncode == 0
    assert run_plan(host_exe, 1.5, True, [(1 << 40, 1, 1)]).returncode == 0


# ---- surface ----------------------------------------------------------------------------------------------------------------
def test_header_is_plain_c_with_the_sinc_job_struct(tmp_path):
    from audio_separator_amd import engine as E
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed for this check"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "asx.h"\nint main(void) {\n  asx_sinc_job j = {0, 0, 0, 0, 0, 0};\n'
           '  int (*f)(asx_engine *, const asx_sinc_job *, int32_t, double, int32_t, void *) = asx_resample_sinc_batch_dev;\n'
           '  printf("%zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(j), offsetof(asx_sinc_job, x_dev), offsetof(asx_sinc_job, y_dev),\n'
           '         offsetof(asx_sinc_job, n_in), offsetof(asx_sinc_job, n_out), offsetof(asx_sinc_job, channels),\n'
           '         offsetof(asx_sinc_job, reserved), ASX_ABI_VERSION);\n  return f == 0;\n}\n')
    c_file = tmp_path / "probe.c"
    c_file.write_text(src)
    obj = str(tmp_path / "probe.o")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c_file), "-o", obj], check=True)
    # linked against nothing: the sizes come from a second translation unit without the function reference
    c_file.write_text(src.replace("asx_resample_sinc_batch_dev;", "0;").replace("return f == 0;", "(void)f; return 0;"))
    exe = str(tmp_path / "probe")
    subprocess.run([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c_file), "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    J = E._SincJob
    assert got == [C.sizeof(J), J.x_dev.offset, J.y_dev.offset, J.n_in.offset, J.n_out.offset, J.channels.offset, J.reserved.offset, 8]
    assert "asx_resample_sinc_batch_dev" in E.SYMBOLS and callable(E.Engine.resample_sinc_batch_dev)


def test_the_device_path_no_longer_refuses_pitch_shift():
    """``demix_many_dev`` used to raise for ``pitch_shift != 0`` before touching its arguments; an empty list is now an empty result"""
    from audio_separator_amd.mdxc import MDXCDemixer
    dm = MDXCDemixer.__new__(MDXCDemixer)
    dm.pitch_shift, dm.sample_rate = 2, 44100
    assert dm.demix_many_dev([]) == []
    down, back = dm.pitch_ratios()
    target = 44100 * 2 ** (-2 / 12)                          # change_pitch_semitones' own expressions
    assert down == float(target) / 44100 and back == float(target * 2 ** (2 / 12)) / target
    assert dm.pitched_len(1000) == math.ceil(1000 * down)
