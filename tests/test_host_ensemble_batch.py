"""The CPU side of ``EnsembleSeparator.separate_many`` (no GPU):

* the plan of asx_ensemble_batch_dev as the library builds it (csrc/ens_pool_plan.h through tests/host/ens_pool_host.cpp) against a
  few lines of integer arithmetic: live sets, n_max, T, n_out and the prefix tables of the pooled launches, compared for equality;
* the plumbing of ``separate_many`` over member and engine doubles: grouping and names per file, result order, the fail-alone and
  host-decoder routes, the refusal route, the run splitting;
* the surface: ``stems_dev_many`` on all four plugins, the header still plain C with the new struct."""
import ctypes as C
import logging
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGORITHMS = ("avg_wave", "median_wave", "min_wave", "max_wave", "avg_fft", "median_fft", "min_fft", "max_fft", "uvr_max_spec",
              "uvr_min_spec", "ensemble_wav")
SILENT = 1e-6


# ---- the plan ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("enspool") / "ens_pool_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "ens_pool_host.cpp")],
                   check=True)
    return exe


def run_plan(exe, alg, jobs, silent=SILENT):
    args = [exe, str(alg), float(silent).hex()]
    for job in jobs:
        args.append(",".join(f"{n}:{float(np.float32(p)).hex()}" for n, p in job) if job else "none")
    return subprocess.run(args, capture_output=True, text=True)


def expected_plan(alg, jobs, silent=SILENT):
    """-> (totals, rows) by the rules of EnsembleSeparator._separate_on_device + asx_ensemble_dev"""
    rows, wave0, frame0, fold0, picks = [], 0, 0, 0, 0
    for job in jobs:
        who = [c for c, (_, p) in enumerate(job) if not float(np.float32(p)) < silent]
        live = len(who)
        n_max = max((job[c][0] for c in who), default=0)
        T = 1 + n_max // 1024 if live else 0
        wave = frames = fold = n_out = 0
        pick = False
        if live == 1 or (live and (alg <= 3 or alg == 10)):
            n_out = n_max
            wave = -(-2 * n_out // 256)
            pick = live >= 2 and alg == 10
        elif live and not (alg in (8, 9) and T < 2):
            n_out = 1024 * (n_max // 1024) if alg in (8, 9) else n_max
            frames, fold = T, -(-n_out // 256)
        rows.append((live, n_max, T, n_out, wave, wave0, frames, frame0, fold, fold0, int(pick), *who))
        wave0, frame0, fold0, picks = wave0 + wave, frame0 + frames, fold0 + fold, picks + pick
    return (wave0, frame0, fold0, picks), rows


def parse_plan(out):
    rows = [line.split() for line in out.splitlines()]
    head = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "plan"]
    assert len(head) == 1
    return head[0], [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "job"]


# (n, peak after normalisation) per contributor: the job list of the GPU test (K = 1, 2, 3, 8, n_max < 1024, the longest silent, all
# silent, one left), then peaks around the bound and lengths around the frame and workgroup edges
PLAN_JOBS = [
    [(3000, 0.7)],
    [(1024, 0.9), (257, 0.7)],
    [(4099, 0.7), (2048, 0.9), (1025, 0.5)],
    [(1, 0.7), (255, 0.9), (256, 0.5), (1023, 0.7), (2047, 0.9), (2048, 0.5), (3000, 0.7), (1025, 0.9)],
    [(255, 0.7), (1023, 0.9)],
    [(4099, 0.0), (2047, 0.7), (2048, 0.9)],
    [(256, 0.0), (1, 0.0)],
    [(3000, 0.0), (1025, 0.7)],
    [(128, 9.99e-7), (127, 1.0e-6), (129, 1.01e-6)],          # float32(1e-6) is below the float64 bound: silent, as write_audio has it
    [(2048, 0.3), (2047, float("nan"))],                       # a NaN peak is not below the bound
    [(1 << 20, 0.5), ((1 << 20) + 1, 0.5)],
    [(0, 0.5), (1023, 0.5)],
]


@pytest.mark.parametrize("alg", range(11))
def test_plan_equals_the_integer_arithmetic(host_exe, alg):
    for jobs in (PLAN_JOBS, PLAN_JOBS[::-1], PLAN_JOBS[2:3], []):
        r = run_plan(host_exe, alg, jobs)
        assert r.returncode == 0, (r.stdout, r.stderr)
        assert parse_plan(r.stdout) == expected_plan(alg, jobs), (ALGORITHMS[alg], jobs)
    totals, rows = parse_plan(run_plan(host_exe, alg, PLAN_JOBS).stdout)
    assert [r[0] for r in rows[:10]] == [1, 2, 3, 8, 2, 2, 0, 1, 1, 2] and rows[8][11:] == (2,) and rows[5][1] == 2048
    # every workgroup / frame of a stage belongs to exactly one job: the shares tile the grid in job order
    for size, first, total in ((4, 5, totals[0]), (6, 7, totals[1]), (8, 9, totals[2])):
        assert sum(r[size] for r in rows) == total
        assert all(r[first] == sum(q[size] for q in rows[:j]) for j, r in enumerate(rows))
    assert totals[3] == (sum(r[0] >= 2 for r in rows) if alg == 10 else 0)


def test_plan_refusals_name_the_job(host_exe):
    ok = [(100, 0.5)]
    for jobs, text in (([ok, [], ok], "error job 1: 0 contributors"), ([ok, ok, [(10, 0.5)] * 9], "error job 2: 9 contributors"),
                       ([[(-1, 0.5)]], "error job 0: contributor 0 has n = -1")):
        r = run_plan(host_exe, 0, jobs)
        assert r.returncode == 3 and r.stdout.startswith(text), r.stdout
    for alg in (-1, 11):
        r = run_plan(host_exe, alg, [ok])
        assert r.returncode == 3 and r.stdout.startswith(f"error unknown ensemble algorithm {alg}"), r.stdout


# ---- separate_many over doubles ------------------------------------------------------------------------------------------------
class FakeTensor:
    """what separate_many touches of a CUDA tensor"""

    def __init__(self, array, device_index=None):
        self.a = np.ascontiguousarray(array, np.float32)
        self.shape = self.a.shape
        self.device = type("D", (), {"index": device_index})()

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return id(self)

    def __getitem__(self, key):
        return FakeTensor(self.a[key], self.device.index)

    def view(self, *shape):
        return FakeTensor(self.a.reshape(shape), self.device.index)


class FakeEngine:
    device = None

    def __init__(self, registry):
        self.registry, self.calls = registry, []

    def ensemble_batch_dev(self, jobs, algorithm, weights, max_peak, min_peak, silent_below=SILENT, mode="pcm16", stream=0):
        """the result of a job is its first contributor that is not silent (all zeros)"""
        self.calls.append([len(c) for c, _, _ in jobs])
        done = []
        for contributors, out_ptr, capacity in jobs:
            stems = [(self.registry[ptr], n, layout) for ptr, n, layout in contributors]
            peaks = [float(np.abs(t.a).max()) if t.a.size else 0.0 for t, _, _ in stems]
            live = [(t, n, layout) for (t, n, layout), p in zip(stems, peaks) if not p < silent_below]
            assert capacity >= max(n for _, n, _ in stems)
            if live:
                t, n, layout = live[0]
                self.registry[out_ptr].a[: 2 * n] = (t.a if layout == "planar" else t.a.T).reshape(-1)
            done.append((live[0][1] if live else 0, len(live), peaks))
        return done


class FakeMember:
    """a plugin as EnsembleSeparator sees it: stems named ``names``, constant-valued, 10 + len(base name) samples each"""
    sample_rate, normalization_threshold, amplification_threshold = 44100, 0.9, 0.0
    use_soundfile, output_format, output_dir, model_path = False, "WAV", None, None

    def __init__(self, name, names, registry, engine, layout="planar", silent=(), host=(), broken=()):
        self.model_name, self.names, self.registry, self.engine, self.layout = name, names, registry, engine, layout
        self.silent, self.host, self.broken = silent, host, broken
        self.logger = logging.getLogger("fake")
        self.seen, self.written, self.state = [], [], None
        self.audio_file_base = None

    def stems_dev_many(self, paths):
        self.seen.append(list(paths))
        self.batch_errors = {}
        stems, states = [], []
        for i, path in enumerate(paths):
            base = os.path.splitext(os.path.basename(path))[0]
            if base in self.broken:
                self.batch_errors[i] = ValueError(f"{base} is broken")
                stems.append(self.batch_errors[i])
                states.append(None)
            elif base in self.host:
                stems.append(None)
                states.append(None)
            else:
                n = 10 + len(base)
                entry = []
                for s, name in enumerate(self.names):
                    value = 0.0 if (base, name) in self.silent else 0.1 * (s + 1) + 0.01 * len(self.model_name)
                    t = FakeTensor(np.full((2, n) if self.layout == "planar" else (n, 2), value))
                    self.registry[t.data_ptr()] = t
                    entry.append((name, t, self.layout))
                stems.append(entry)
                states.append({"audio_file_base": base, "input_bit_depth": 16})
        return stems, states

    def stems_dev(self, path):
        raise AssertionError("separate_many pools: stems_dev must not run")

    def _restore_file(self, state):
        self.state = dict(state)
        self.audio_file_base = state["audio_file_base"]

    def _reset_file_state(self):
        self.state, self.audio_file_base = None, None

    def get_stem_output_path(self, stem_name, custom_output_names):
        return f"{self.audio_file_base}_({stem_name})_{self.model_name}.wav"

    def _stream(self):
        return 0

    def _writing(self):
        import contextlib
        return contextlib.nullcontext()

    def _host_planar_stems(self, dev):
        return dev.a, [dev.a[i].T for i in range(dev.a.shape[0])]

    def write_audio(self, path, source):
        self.written.append((path, self.state["audio_file_base"], np.array(source)))


@pytest.fixture()
def doubles(monkeypatch):
    from audio_separator_amd import ensemble as ENS
    registry = {}
    engine = FakeEngine(registry)

    def result_buffer(like, numel):
        t = FakeTensor(np.full((numel,), np.nan))
        registry[t.data_ptr()] = t
        return t
    monkeypatch.setattr(ENS.EnsembleSeparator, "_result_buffer", staticmethod(result_buffer))
    return ENS, registry, engine


def test_separate_many_groups_names_and_order(doubles):
    ENS, registry, engine = doubles
    a = FakeMember("model_a", ["Vocals", "Instrumental"], registry, engine, layout="rows", silent={("song_three", "Vocals")})
    b = FakeMember("model_b", ["Drums", "Vocals", "Other"], registry, engine)
    ens = ENS.EnsembleSeparator([a, b], "avg_wave", model_filenames=["a.onnx", "b.ckpt"], pool_files=None)
    ens._free_hbm = lambda: None                       # no device: one run
    paths = ["/x/song_one.wav", "/y/song_three.wav", "/z/s2.wav"]
    got = ens.separate_many(paths, {"Drums": "the_drums"})
    # per file: groups in first-seen order (member a's stems, then b's new ones); a 3-stem model's "Other" stays "Other"
    assert got == [[f"{base}_({g})_custom_ensemble_a_b.wav" for g in ("Vocals", "Instrumental")] + ["the_drums.wav", f"{base}_(Other)_custom_ensemble_a_b.wav"]
                   for base in ("song_one", "song_three", "s2")]
    assert ens.last_paths_taken == ["device"] * 3 and ens.batch_errors == {}
    assert a.seen == [paths] and b.seen == [paths] and a.written == []          # one pooled call per member; the last member writes
    assert engine.calls == [[2, 1, 1, 1] * 3]                                   # ONE combine for all (file, group) jobs
    assert [(p, base) for p, base, _ in b.written] == [(f, base) for fs, base in zip(got, ("song_one", "song_three", "s2")) for f in fs]
    # member a's Vocals of song_three is silent: member b's comes out instead (0.2 + 0.07), at song_three's length
    vocals = b.written[4][2]
    assert vocals.shape == (20, 2) and np.allclose(vocals, 0.27)
    assert np.allclose(b.written[0][2], 0.17) and b.written[0][2].shape == (18, 2)   # song_one: a's (rows layout) first
    assert a.state is None and b.state is None


def test_separate_many_routes(doubles, monkeypatch, caplog):
    ENS, registry, engine = doubles
    a = FakeMember("model_a", ["Vocals", "Instrumental"], registry, engine, broken={"bad"})
    b = FakeMember("model_b", ["Vocals", "Instrumental"], registry, engine, host={"hosted"}, broken={"worse"})
    ens = ENS.EnsembleSeparator([a, b], "max_fft", pool_files=2)
    order = []
    monkeypatch.setattr(ens, "_separate_via_files", lambda path, custom: order.append(path) or [f"files:{os.path.basename(path)}"])
    paths = ["/q/one.wav", "/q/bad.wav", "/q/hosted.wav", "/q/two.wav", "/q/worse.wav"]
    with caplog.at_level(logging.INFO):
        got = ens.separate_many(paths)
    assert ens.last_paths_taken == ["device", "failed", "files", "device", "failed"]
    assert got[1] == [] and got[4] == [] and got[2] == ["files:hosted.wav"] and len(got[0]) == len(got[3]) == 2
    assert sorted(ens.batch_errors) == [1, 4] and "bad is broken" in str(ens.batch_errors[1]) and "worse is broken" in caplog.text
    assert "needs the host decoder" in caplog.text
    # pool_files = 2: runs [0, 1], [2, 3], [4]; every member sees each run once, in order
    assert a.seen == b.seen == [paths[0:2], paths[2:4], paths[4:5]]
    assert engine.calls == [[2, 2], [2, 2]]                                     # (the last run has no file left to combine)
    assert order == ["/q/hosted.wav"]
    # a failing file path fails alone too
    def boom(path, custom):
        raise RuntimeError("no decoder")
    monkeypatch.setattr(ens, "_separate_via_files", boom)
    got = ens.separate_many(paths[2:4])
    assert got[0] == [] and len(got[1]) == 2 and ens.last_paths_taken == ["failed", "device"] and list(ens.batch_errors) == [0]


def test_separate_many_refused_is_the_loop(doubles, monkeypatch):
    ENS, registry, engine = doubles
    a = FakeMember("model_a", ["Vocals"], registry, engine)
    b = FakeMember("model_b", ["Vocals"], registry, engine)
    for kw, patch in (({"via_files": True}, None), ({}, "soundfile"), ({}, "no hook")):
        ens = ENS.EnsembleSeparator([a, b], "avg_wave", **kw)
        if patch == "soundfile":
            monkeypatch.setattr(b, "use_soundfile", True, raising=False)
        if patch == "no hook":
            monkeypatch.setattr(b, "use_soundfile", False, raising=False)
            monkeypatch.delattr(FakeMember, "stems_dev_many")
        calls = []

        def separate(path, custom=None, ens=ens, calls=calls):
            calls.append((path, custom))
            ens.last_path_taken = "files"
            return [f"out:{path}"]
        monkeypatch.setattr(ens, "separate", separate)
        assert ens.separate_many(["p", "q"], {"Vocals": "v"}) == [["out:p"], ["out:q"]]
        assert calls == [("p", {"Vocals": "v"}), ("q", {"Vocals": "v"})] and ens.last_paths_taken == ["files", "files"]
        assert a.seen == [] and engine.calls == []


def test_runs_follow_pool_files_and_the_memory_rule(doubles, tmp_path):
    ENS, registry, engine = doubles
    from audio_separator_amd import audio_io
    members = [FakeMember("model_a", ["Vocals", "Instrumental"], registry, engine), FakeMember("model_b", ["Vocals", "Instrumental"], registry, engine)]
    paths = []
    for i, frames in enumerate((1000, 1000, 3000, 500, 500)):
        paths.append(str(tmp_path / f"f{i}.wav"))
        audio_io.write_wav(paths[-1], np.zeros((frames, 2), np.int16), 44100)
    paths.insert(2, str(tmp_path / "not_a_wav.txt"))                            # costs nothing: no stems are kept for it
    assert ENS.EnsembleSeparator(members, pool_files=4)._runs(paths) == [[0, 1, 2, 3], [4, 5]]
    assert ENS.EnsembleSeparator(members, pool_files=1)._runs(paths) == [[i] for i in range(6)]
    ens = ENS.EnsembleSeparator(members)
    per_frame = 8 * (2 + 2)                                                      # 8 bytes x stems x members
    ens._free_hbm = lambda: 2000.5 * per_frame / ens.HBM_SHARE                   # room for 2000 frames
    assert ens._runs(paths) == [[0, 1, 2], [3], [4, 5]]                          # 1000 + 1000 (+ 0) | 3000 alone, over the budget | 500 + 500
    ens._free_hbm = lambda: None
    assert ens._runs(paths) == [list(range(6))] and ens._runs([]) == []
    assert ens.HBM_SHARE == 0.4
    with pytest.raises(ValueError, match="pool_files"):
        ENS.EnsembleSeparator(members, pool_files=0)


# ---- the surface -----------------------------------------------------------------------------------------------------------------
def test_all_four_plugins_publish_stems_dev_many():
    from audio_separator_amd.architectures.demucs_separator import DemucsSeparator
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from audio_separator_amd.architectures.mdxc_separator import MDXCSeparator
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    from audio_separator_amd.common_separator import CommonSeparator
    for cls in (MDXSeparator, MDXCSeparator, DemucsSeparator, VRSeparator):
        assert cls.stems_dev_many is CommonSeparator._stems_dev_many, cls
        assert "_stems_of" in cls.__dict__ and "stems_dev" in cls.__dict__, cls
    assert not hasattr(CommonSeparator, "stems_dev_many")
    import audio_separator_amd as A
    assert hasattr(A.EnsembleSeparator, "separate_many") and hasattr(A.Engine, "ensemble_batch_dev")


def test_header_is_plain_c_with_the_job_struct(tmp_path):
    from audio_separator_amd import engine as E
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed for this check"
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "asx.h"\nint main(void) {\n  asx_ens_job j;\n'
           '  int (*f)(asx_engine *, asx_ens_job *, int32_t, int32_t, const double *, int32_t, int32_t, float, float, int32_t, double, void *) = '
           'asx_ensemble_batch_dev;\n  j.k = ASX_ENS_MAX_K;\n'
           '  printf("%zu %zu %zu %d %d\\n", sizeof(j), offsetof(asx_ens_job, out_dev), offsetof(asx_ens_job, peak_after), ASX_ABI_VERSION, j.k);\n'
           '  return f == 0;\n}\n')
    c = tmp_path / "job.c"
    c.write_text(src)
    exe = tmp_path / "job"
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(exe) + ".o"],
                   check=True)
    assert C.sizeof(E._EnsJob) == 224 and E._EnsJob.out_dev.offset == 168 and E._EnsJob.peak_after.offset == 192
    assert [n for n, _ in E._EnsJob._fields_] == ["k", "live", "stem_dev", "n_samples", "layout", "out_dev", "out_capacity", "n_out", "peak_after"]
    assert E.ABI_VERSION == 8 and "asx_ensemble_batch_dev" in E.SYMBOLS and E.ENS_MAX_K == 8
    header = open(os.path.join(ROOT, "include", "asx.h")).read()
    assert "#define ASX_ENS_MAX_K 8" in header and "#define ASX_ABI_VERSION 8" in header
