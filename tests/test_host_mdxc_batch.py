"""CPU side of the MDXC batch entry points.  The pool plan as the library builds it (csrc/mdxc_pool_plan.h, no GPU, driven by
tests/host/mdxc_pool_host.cpp) against a restatement of the reference's chunk arithmetic (mdxc_separator.py:298-341 Roformer,
:361-402 TFC) -- all integers, compared for equality; the chunk set the pooled Roformer fold walks per sample against the
definition of "chunk k covers sample i"; ``MDXCSeparator.separate_many`` over the CPU engine double against ``separate`` per path;
and the surface: which plugins publish ``separate_many``, the header is still plain C."""
import ctypes as C
import filecmp
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import fake_engine
from tests import separate_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 16
TFC_DIM_T, TFC_LENGTHS = 16, (1, 100, 239, 240, 241, 480, 3000)               # chunk 240
ROF_DIM_T, ROF_LENGTHS = 21, (320, 321, 520, 640, 777, 1500)                  # chunk 320


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mdxcpool") / "mdxc_pool_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "mdxc_pool_host.cpp")], check=True)
    return exe


def run(exe, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)


def parse(out):
    rows = [line.split() for line in out.splitlines()]
    plan = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "plan"]
    assert len(plan) == 1
    songs = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "song"]          # chunk0, n_chunks, pad, padded_len
    starts = [[int(v) for v in r[1:]] for r in rows if r[0] == "starts"]
    passes = [(int(r[1]), int(r[2])) for r in rows if r[0] == "pass"]
    return plan[0], songs, starts, passes                                           # plan: chunk, step, front, total, per


def even_batches(nk, max_b):
    nbatch = -(-nk // max_b)
    return -(-nk // nbatch)


def ref_tfc(n, chunk, overlap):
    """mdxc_separator.py:361-374 -> hop_size, front zeros, pad_size, padded length, len(chunks)"""
    hop_size = chunk // overlap
    pad_size = hop_size - (n - chunk) % hop_size
    length = (chunk - hop_size) + n + (pad_size + chunk - hop_size)
    return hop_size, chunk - hop_size, pad_size, length, (length - chunk) // hop_size + 1      # Tensor.unfold


def ref_rof_starts(n, chunk, step):
    """mdxc_separator.py:320-341: where each chunk of the loop is added"""
    return [n - chunk if i + chunk > n else i for i in range(0, n, step)]


def check_passes(plan, passes, total, max_batch):
    per = even_batches(total, max_batch if max_batch > 0 else 8)
    assert plan[3] == total and plan[4] == per
    sizes = [per] * (total // per) + ([total % per] if total % per else [])
    assert passes == [(sum(sizes[:i]), b) for i, b in enumerate(sizes)]


@pytest.mark.parametrize("overlap", [4, 8])
@pytest.mark.parametrize("max_batch", [0, 1, 3, 5, 64])
def test_tfc_pool_plan_equals_reference_arithmetic(host_exe, overlap, max_batch):
    chunk = HOP * (TFC_DIM_T - 1)
    assert chunk == 240
    r = run(host_exe, "tfc", HOP, TFC_DIM_T, overlap, max_batch, *TFC_LENGTHS)
    assert r.returncode == 0, (r.stdout, r.stderr)
    plan, songs, _, passes = parse(r.stdout)
    want = [ref_tfc(n, chunk, overlap) for n in TFC_LENGTHS]
    assert plan[:3] == (chunk, want[0][0], want[0][1])
    chunk0 = 0
    for got, (_, _, pad, length, count) in zip(songs, want):
        assert got == (chunk0, count, pad, length)                                 # chunk0[] is the prefix sum of the counts
        chunk0 += count
    assert len(songs) == len(TFC_LENGTHS)
    check_passes(plan, passes, chunk0, max_batch)


@pytest.mark.parametrize("step", [200, 320])
@pytest.mark.parametrize("max_batch", [0, 1, 3, 5, 64])
def test_roformer_pool_plan_equals_reference_arithmetic(host_exe, step, max_batch):
    chunk = HOP * (ROF_DIM_T - 1)
    assert chunk == 320
    r = run(host_exe, "rof", HOP, ROF_DIM_T, step, max_batch, *ROF_LENGTHS)
    assert r.returncode == 0, (r.stdout, r.stderr)
    plan, songs, starts, passes = parse(r.stdout)
    assert plan[:3] == (chunk, step, 0)
    want = [ref_rof_starts(n, chunk, step) for n in ROF_LENGTHS]
    assert starts == want
    assert [s[:2] for s in songs] == [(sum(len(w) for w in want[:i]), len(w)) for i, w in enumerate(want)]
    check_passes(plan, passes, sum(len(w) for w in want), max_batch)
    assert any(w.count(w[-1]) > 1 for w in want) or step == 320                   # step 200: 1500 samples end in TWO re-anchored chunks


def test_a_pool_of_35_songs_crosses_the_group_boundary(host_exe):
    lengths = list(range(320, 355))
    r = run(host_exe, "rof", HOP, ROF_DIM_T, 200, 8, *lengths)
    plan, songs, starts, passes = parse(r.stdout)
    assert starts == [ref_rof_starts(n, 320, 200) for n in lengths]
    assert [s[0] for s in songs] == [2 * i for i in range(35)] and plan[3] == 70   # 320 is one chunk... of step 200: two starts each
    check_passes(plan, passes, 70, 8)
    r = run(host_exe, "tfc", HOP, TFC_DIM_T, 4, 8, *lengths)
    plan, songs, _, passes = parse(r.stdout)
    counts = [ref_tfc(n, 240, 4)[4] for n in lengths]
    assert [s[:2] for s in songs] == [(sum(counts[:i]), c) for i, c in enumerate(counts)]
    check_passes(plan, passes, sum(counts), 8)


def test_invalid_songs_are_reported_by_index(host_exe):
    r = run(host_exe, "rof", HOP, ROF_DIM_T, 200, 3, 320, 640, 319, 777)
    assert r.returncode == 3 and r.stdout.startswith("error song 2: mix (319 samples) shorter than one chunk (320)"), r.stdout
    r = run(host_exe, "rof", HOP, ROF_DIM_T, 200, 3, 320, 0)
    assert r.returncode == 3 and r.stdout.startswith("error song 1: n_samples must be >= 1"), r.stdout
    r = run(host_exe, "rof", HOP, ROF_DIM_T, 321, 3, 320)
    assert r.returncode == 3 and "step must be in [1, chunk_size]" in r.stdout
    r = run(host_exe, "tfc", HOP, TFC_DIM_T, 4, 3, 100, 0)
    assert r.returncode == 3 and r.stdout.startswith("error song 1: n_samples and overlap must be >= 1"), r.stdout
    r = run(host_exe, "tfc", HOP, TFC_DIM_T, 4, 3)                                # an empty pool is a valid, empty plan
    assert r.returncode == 0 and parse(r.stdout)[0][3] == 0


@pytest.mark.parametrize("step", [200, 320, 100])
def test_bounded_fold_visits_exactly_the_covering_chunks(host_exe, step):
    """roformer_finalize_pool_kernel walks rof_fold_range's chunks: the regular ones [k_lo, k_hi], then the re-anchored ones
    [r_lo, r_hi].  For every sample that list must be what the reference loop adds to it -- every chunk k with
    0 <= i - start_k < C, in increasing k -- and its length is bounded by the geometry."""
    chunk = 320
    for n in ROF_LENGTHS:
        starts = np.array(ref_rof_starts(n, chunk, step))
        r = run(host_exe, "fold", HOP, ROF_DIM_T, step, n)
        assert r.returncode == 0, r.stdout
        rng = np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()])
        assert rng.shape == (n, 4)
        i = np.arange(n)[:, None]
        covers = (i - starts[None, :] >= 0) & (i - starts[None, :] < chunk)         # [n, chunks]
        k = np.arange(len(starts))[None, :]
        visited = ((k >= rng[:, 0:1]) & (k <= rng[:, 1:2])) | ((k >= rng[:, 2:3]) & (k <= rng[:, 3:4]))
        assert np.array_equal(visited, covers), (n, step)
        assert (rng[:, 1] < rng[:, 2]).all()                                        # regular before re-anchored: increasing k
        assert covers.sum(1).min() >= 1 and visited.sum(1).max() <= 2 * -(-chunk // step)
        if starts[-1] != (len(starts) - 1) * step:                                  # the re-anchored last chunk is visited
            assert visited[n - 1, len(starts) - 1] and rng[n - 1, 3] == len(starts) - 1


# ---- plugin level, over the engine double -----------------------------------------------------------------------------------
class BatchOracleEngine(fake_engine.OracleEngine):
    """The double plus the four batch methods, as loops of its single-song ones; ``log`` records (segment_size, samples) per demix"""
    log = []
    batch_calls = 0

    def mdxc_demix(self, mix, overlap):
        BatchOracleEngine.log.append((self.cfg.segment_size, mix.shape[1]))
        return super().mdxc_demix(mix, overlap)

    def rof_demix(self, mix, step):
        BatchOracleEngine.log.append((self.cfg.segment_size, mix.shape[1]))
        return super().rof_demix(mix, step)

    def mdxc_demix_batch(self, mixes, overlap):
        BatchOracleEngine.batch_calls += 1
        return [self.mdxc_demix(m, overlap) for m in mixes]

    def rof_demix_batch(self, mixes, step):
        BatchOracleEngine.batch_calls += 1
        return [self.rof_demix(m, step) for m in mixes]

    def mdxc_demix_batch_dev(self, songs, overlap, stream=0):
        raise AssertionError("the double has no device path")

    rof_demix_batch_dev = mdxc_demix_batch_dev


RATE = 100                                                   # the toy rate: a file under 1000 samples is "short"
MODELS = {"two": ("mdxc", 0), "one": ("mdxc", 1), "rof": ("roformer", 0)}


def _install(monkeypatch):
    from audio_separator_amd import mdxc
    fake_engine.install(monkeypatch)
    monkeypatch.setattr(mdxc, "Engine", BatchOracleEngine)
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    BatchOracleEngine.log, BatchOracleEngine.batch_calls = [], 0


def _wav(tmp_path, name, n, seed, scale=0.3):
    from audio_separator_amd import audio_io
    p = str(tmp_path / name)
    x = (scale * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)
    audio_io.write_wav(p, np.clip(x, -0.99, 0.99), RATE, "PCM_16")
    return p


def _maker(tmp_path, model, **arch_over):
    family, idx = MODELS[model]
    _, cls, common, arch, _, _ = SC.cases(family, str(tmp_path))[idx]
    arch = dict(arch, **arch_over)
    if model == "rof":
        arch["segment_size"] = 11                            # the override geometry: chunk 160 against the model's 320
    return lambda out_dir, **over: SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, sample_rate=RATE, **over), arch_config=arch)


def _loop(sep, paths):
    """what the orchestrator does with a list: ``separate`` per path on ONE instance, a failing file skipped"""
    out = []
    for p in paths:
        try:
            out.append(sep.separate(p))
        except Exception:
            out.append([])
        sep.clear_file_specific_paths()
    return out


def _same_files(names, dir_a, dir_b):
    assert names and all(names)
    for per_file in names:
        for name in per_file:
            assert filecmp.cmp(os.path.join(dir_a, name), os.path.join(dir_b, name), shallow=False), name


@pytest.mark.parametrize("model", ["two", "one", "rof"])
def test_separate_many_equals_separate_per_path(tmp_path, monkeypatch, model):
    """[long, short, long]: the first file runs the model's geometry, the short one switches ``override_model_segment_size`` on and
    it stays on for the third -- in ``separate_many`` as in the loop; plus a silent file and (Roformer) one shorter than a chunk of
    the geometry it would run under, which fail alone."""
    _install(monkeypatch)
    make = _maker(tmp_path, model)
    good = [_wav(tmp_path, "a.wav", 1500, 1), _wav(tmp_path, "b.wav", 500, 2), _wav(tmp_path, "c.wav", 1200, 3)]
    silent = _wav(tmp_path, "silent.wav", 700, 4, scale=0.0)
    tiny = _wav(tmp_path, "tiny.wav", 100, 5)                   # under override: one Roformer chunk is 160 samples
    paths = [good[0], silent, good[1], tiny, good[2]]
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    sep = make(one_dir)
    model_seg, over_seg = (21, 11) if model == "rof" else (16, 12)
    want = _loop(sep, paths)
    log_loop = list(BatchOracleEngine.log)
    BatchOracleEngine.log = []
    sep = make(many_dir)
    got = sep.separate_many(paths)
    assert got == want
    bad = [1, 3] if model == "rof" else [1]
    assert sorted(sep.batch_errors) == bad and all(got[i] == [] for i in bad)
    assert all(isinstance(sep.batch_errors[i], ValueError) for i in bad)
    _same_files([got[i] for i in range(5) if i not in bad], one_dir, many_dir)
    # the sticky override: file 0 on the model's geometry, everything from the short file on under the configured one
    log_many = BatchOracleEngine.log
    assert log_many[0] == (model_seg, 1500) and (over_seg, 500) in log_many and (over_seg, 1200) in log_many
    assert sorted(log_many) == sorted(e for e in log_loop if e != (over_seg, 100) or model != "rof")
    if model == "rof":
        assert (over_seg, 100) not in log_many                  # the too-short file never reached the pooled call
    assert BatchOracleEngine.batch_calls == 2                   # two pools: the prefix and the suffix
    assert sep.override_model_segment_size is True
    assert sep.audio_file_path == good[2] and sep.primary_source is not None   # the last good file's state


@pytest.mark.parametrize("model", ["two", "rof"])
def test_pool_split_changes_no_byte(tmp_path, monkeypatch, model):
    _install(monkeypatch)
    paths = [_wav(tmp_path, f"in{i}.wav", n, 10 + i) for i, n in enumerate((1500, 1100, 2000, 1300))]
    whole, split = str(tmp_path / "whole"), str(tmp_path / "split")
    got = _maker(tmp_path, model)(whole).separate_many(paths)
    assert BatchOracleEngine.batch_calls == 1
    assert _maker(tmp_path, model, asx_pool_chunks=12)(split).separate_many(paths) == got
    assert BatchOracleEngine.batch_calls - 1 > 1                # the same files in several pooled calls
    _same_files(got, whole, split)


def test_pitch_shift_takes_the_loop_path(tmp_path, monkeypatch):
    _install(monkeypatch)
    paths = [_wav(tmp_path, "a.wav", 1300, 21), _wav(tmp_path, "b.wav", 1100, 22)]
    make = _maker(tmp_path, "two", pitch_shift=2)
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    want = _loop(make(one_dir), paths)
    got = make(many_dir).separate_many(paths)
    assert got == want and BatchOracleEngine.batch_calls == 0
    _same_files(got, one_dir, many_dir)


# ---- surface ----------------------------------------------------------------------------------------------------------------
def test_all_four_plugins_publish_separate_many(tmp_path, monkeypatch):
    """MDX, Demucs and VR carry the shared shell as a class attribute; MDXCSeparator binds it on every instance"""
    from audio_separator_amd.architectures.demucs_separator import DemucsSeparator
    from audio_separator_amd.architectures.mdx_separator import MDXSeparator
    from audio_separator_amd.architectures.mdxc_separator import MDXCSeparator
    from audio_separator_amd.architectures.vr_separator import VRSeparator
    from audio_separator_amd.common_separator import CommonSeparator
    for cls in (MDXSeparator, DemucsSeparator, VRSeparator):
        assert cls.separate_many is CommonSeparator._separate_many, cls
    _install(monkeypatch)
    for model in MODELS:
        sep = _maker(tmp_path, model)(str(tmp_path / "out"))
        assert isinstance(sep, MDXCSeparator) and sep.separate_many.__func__ is CommonSeparator._separate_many
        assert sep.separate_many.__self__ is sep and sep.separate_many([]) == []
    for hook in ("_prepare_model", "_check_loaded", "_pooled_stems", "_emit_file"):
        assert hook in MDXCSeparator.__dict__, hook
    from audio_separator_amd import sharding
    from audio_separator_amd.mdxc import MDXCDemixer
    assert callable(sharding.mdxc_demix_many) and callable(MDXCDemixer.demix_many) and callable(MDXCDemixer.demix_many_dev)
    with pytest.raises(ValueError):
        sharding.mdxc_demix_many(None)                           # overlap (TFC) or step (Roformer), one of them


def test_header_is_plain_c_with_the_mdxc_song_struct(tmp_path):
    from audio_separator_amd import engine as E
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed for this check"
    src = ('#include <stdio.h>\n#include "asx.h"\nint main(void) {\n  asx_mdxc_song s = {0, 0, 0};\n'
           '  int (*f)(asx_engine *, const asx_mdxc_song *, int32_t, int32_t, void *) = asx_mdxc_demix_batch_dev;\n'
           '  int (*g)(asx_engine *, const asx_mdxc_song *, int32_t, int64_t, void *) = asx_rof_demix_batch_dev;\n'
           '  printf("%zu %d\\n", sizeof(s), ASX_ABI_VERSION);\n  return f == 0 || g == 0;\n}\n')
    c = tmp_path / "song.c"
    c.write_text(src)
    subprocess.run([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o",
                    str(tmp_path / "song.o")], check=True)
    assert C.sizeof(E._MdxcSong) == 24 and [n for n, _ in E._MdxcSong._fields_] == ["mix_dev", "out_dev", "n_samples"]
    assert E.ABI_VERSION == 8 and {"asx_mdxc_demix_batch_dev", "asx_rof_demix_batch_dev"} <= set(E.SYMBOLS)
    for name in ("mdxc_demix_batch", "mdxc_demix_batch_dev", "rof_demix_batch", "rof_demix_batch_dev"):
        assert callable(getattr(E.Engine, name)), name
