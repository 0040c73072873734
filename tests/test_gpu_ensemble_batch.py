"""A batch of songs through an ensemble on the MI355X (EnsembleSeparator.separate_many, asx_ensemble_batch_dev).

1. the pooled combine (``Engine.ensemble_batch_dev``) against the per-job calls it replaces -- ``ensemble_slot_dev`` per
   contributor, the silent ones dropped, ``ensemble_dev`` over the stack -- bit for bit: outputs, lengths, peaks, live counts;
2. its refusals (nothing is written);
3. ``separate_many`` against ``separate`` per path, byte for byte, with three resident 44.1 kHz members and all eleven algorithms,
   and what must (not) run while it does;
4. unequal contributor lengths and lone groups (Demucs + VR at 8 kHz);
5. files that fail alone; 6. ``pool_files``."""
import filecmp
import os
import random
import tempfile

import numpy as np
import pytest

from tests.test_gpu_ensemble_models import ALGORITHMS, MAX_PEAK, _stem
from tests.test_gpu_ensemble_models import members_8k, members_44k  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SILENT = 1e-6
SLACK = 300


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    return A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))


# ---- 1. the pooled combine -------------------------------------------------------------------------------------------------
# job -> [(n, layout, amplitude)]; amplitudes are the peak regimes of test_gpu_ensemble_models.REGIMES under max_peak 0.9:
# 1.7 above max_peak, 0.2 below a min_peak of 0.5, 0.7 between the two, 0.0 all zeros
P, R = "planar", "rows"
JOBS = (
    [(3000, P, 0.7)],                                                               # K = 1
    [(1024, R, 1.7), (257, P, 0.7)],                                                # K = 2; 2 * n_max is a multiple of 256
    [(4099, P, 0.7), (2048, R, 1.7), (1025, P, 0.2)],                               # K = 3; 2 * n_max is not
    [(1, R, 0.7), (255, P, 1.7), (256, R, 0.2), (1023, P, 0.7), (2047, R, 1.7), (2048, P, 0.2), (3000, R, 0.7), (1025, P, 1.7)],   # K = 8
    [(255, R, 0.7), (1023, P, 1.7)],                                                # n_max < 1024: no result under uvr_*
    [(4099, P, 0.0), (2047, R, 0.7), (2048, P, 1.7)],                               # the LONGEST is all zeros: dropped, n_max shrinks
    [(256, P, 0.0), (1, R, 0.0)],                                                   # all zeros: live = 0
    [(3000, R, 0.0), (1025, P, 0.7)],                                               # one left after the drop: its slot image
)
# (min_peak, keep the all-zero stems?): a set min_peak would scale a zero stem by inf, which no file ever meets -- there the zero
# stems become "below" ones, and the zero regime runs under min_peak 0.0 (amplification off, the plugins' default) and None
EDGES = ((0.5, False), (0.0, True), (None, True))


def _device_jobs(min_peak_keeps_zeros, dev):
    import torch
    jobs = []
    for j, spec in enumerate(JOBS):
        contributors = []
        for c, (n, layout, amplitude) in enumerate(spec):
            if amplitude == 0.0 and not min_peak_keeps_zeros:
                amplitude = 0.2
            x = _stem(n, amplitude, 1000 * j + c)
            contributors.append((torch.from_numpy(np.ascontiguousarray(x if layout == P else x.T)).to(dev), n, layout))
        jobs.append(contributors)
    return jobs


def _per_job_reference(eng, contributors, algorithm, weights, min_peak, mode):
    """EnsembleSeparator._separate_on_device for one stem group -> (result bits or None, n_out, peak per contributor, live)"""
    import torch
    live = list(range(len(contributors)))
    peaks_all = [None] * len(contributors)
    stack = None
    while live:
        n_max = max(contributors[c][1] for c in live)
        stack = torch.empty((len(live), 2, n_max), dtype=torch.float32, device=contributors[0][0].device)
        peaks = [eng.ensemble_slot_dev(contributors[c][0].data_ptr(), contributors[c][1], contributors[c][2], MAX_PEAK, min_peak,
                                       stack.data_ptr(), slot, n_max, mode=mode) for slot, c in enumerate(live)]
        for c, p in zip(live, peaks):
            peaks_all[c] = p
        if not any(p < SILENT for p in peaks):
            break
        live = [c for c, p in zip(live, peaks) if not p < SILENT]
    if not live:
        return None, 0, peaks_all, 0
    if len(live) == 1:
        return stack.cpu().numpy().reshape(-1).view(np.uint32), stack.shape[2], peaks_all, 1
    out = torch.full((2 * stack.shape[2],), float("nan"), dtype=torch.float32, device=stack.device)
    n_out = eng.ensemble_dev(stack.data_ptr(), len(live), stack.shape[2], algorithm, weights, out.data_ptr())
    return out[: 2 * n_out].cpu().numpy().view(np.uint32), n_out, peaks_all, len(live)


def _pooled(eng, jobs, algorithm, weights, min_peak, mode):
    import torch
    outs = []
    for contributors in jobs:
        cap = max(n for _, n, _ in contributors) + SLACK
        outs.append(torch.full((2 * cap,), float("nan"), dtype=torch.float32, device=contributors[0][0].device))
    got = eng.ensemble_batch_dev([([(t.data_ptr(), n, layout) for t, n, layout in contributors], out.data_ptr(), out.numel() // 2)
                                  for contributors, out in zip(jobs, outs)], algorithm, weights, MAX_PEAK, min_peak, SILENT, mode=mode)
    torch.cuda.synchronize()
    return got, [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("mode", ["pcm16", "float32"])
@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_pooled_combine_equals_the_per_job_calls(eng, algorithm, mode):
    import torch
    dev = torch.device("cuda", 0)
    weight_lists = ([1.0, 2.0, 0.5], [3.0, 1.0]) if algorithm.startswith("avg_") else (None,)
    for min_peak, zeros in EDGES:
        jobs = _device_jobs(zeros, dev)
        for weights in weight_lists:
            want = [_per_job_reference(eng, c, algorithm, weights, min_peak, mode) for c in jobs]
            got, bufs = _pooled(eng, jobs, algorithm, weights, min_peak, mode)
            for j, ((bits, n_out, peaks, live), (g_n, g_live, g_peaks), buf) in enumerate(zip(want, got, bufs)):
                where = (algorithm, mode, min_peak, weights, j)
                assert (g_n, g_live) == (n_out, live), where
                assert g_peaks == peaks, (where, g_peaks, peaks)
                if bits is not None:
                    assert np.array_equal(buf[: 2 * n_out].view(np.uint32), bits), where
                assert np.isnan(buf[2 * n_out:]).all(), where                   # the slack, and every buffer of a job without a result
            if zeros:
                uvr = algorithm.startswith("uvr_")
                assert [g[1] for g in got] == [1, 2, 3, 8, 2, 2, 0, 1]
                assert got[5][0] == 2048 and got[6][0] == 0 and got[7][0] == 1025 and got[4][0] == (0 if uvr else 1023)
                assert got[2][0] == (1024 * (4099 // 1024) if uvr else 4099) and got[0][0] == 3000
            # the same call again: the same bits
            again, bufs2 = _pooled(eng, jobs, algorithm, weights, min_peak, mode)
            assert again == got
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(bufs, bufs2))
            # one job alone
            for j in (2, 3):
                one, buf1 = _pooled(eng, [jobs[j]], algorithm, weights, min_peak, mode)
                assert one[0][:2] == got[j][:2] and np.array_equal(buf1[0].view(np.uint32), bufs[j].view(np.uint32)), (algorithm, mode, j)


# ---- 2. refusals -------------------------------------------------------------------------------------------------------------
def test_pooled_combine_refuses_bad_arguments(eng):
    import torch
    import audio_separator_amd as A
    dev = torch.device("cuda", 0)
    stem = torch.ones((2, 64), dtype=torch.float32, device=dev)
    outs = [torch.full((2 * 364,), float("nan"), dtype=torch.float32, device=dev) for _ in range(3)]
    good = ([(stem.data_ptr(), 64, P), (stem.data_ptr(), 64, P)], outs[0].data_ptr(), 364)
    nine = [(stem.data_ptr(), 64, P)] * 9
    bad = {"k = 0": ([], outs[1].data_ptr(), 364), "k = 9": (nine, outs[1].data_ptr(), 364),
           "null stem": ([(0, 64, P), (stem.data_ptr(), 64, P)], outs[1].data_ptr(), 364),
           "n < 0": ([(stem.data_ptr(), -1, R)], outs[1].data_ptr(), 364),
           "null out": ([(stem.data_ptr(), 64, P)], 0, 364),
           "short out": ([(stem.data_ptr(), 64, P)], outs[1].data_ptr(), 63)}
    for what, job in bad.items():
        with pytest.raises(A.AsxError, match=r"asx_ensemble_batch_dev: job 1\b") as err:
            eng.ensemble_batch_dev([good, job, (good[0], outs[2].data_ptr(), 364)], "avg_wave", None, MAX_PEAK, 0.0)
        assert err.value is not None, what
    # an unknown algorithm has no offending job: the message names the call and the number
    with pytest.raises(A.AsxError, match="asx_ensemble_batch_dev: unknown ensemble algorithm 11"):
        eng.ensemble_batch_dev([good], 11, None, MAX_PEAK, 0.0)
    with pytest.raises(ValueError, match="Unknown ensemble algorithm"):
        eng.ensemble_batch_dev([good], "avg_wavelet", None, MAX_PEAK, 0.0)
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    assert eng.ensemble_batch_dev([], "avg_wave", None, MAX_PEAK, 0.0) == []
    # and the engine still works
    assert eng.ensemble_batch_dev([good], "avg_wave", None, MAX_PEAK, 0.0)[0][:2] == (64, 2)


# ---- 3. - 6. files -----------------------------------------------------------------------------------------------------------
def _variants(wav, tmp_path, lengths, sample_rate):
    """``wav`` plus copies rolled and cut (or repeated) to ``lengths`` samples, as 16-bit files"""
    from audio_separator_amd import audio_io
    x, sr = audio_io.read_wav(wav)
    assert sr == sample_rate
    paths = [wav]
    for i, n in enumerate(lengths):
        y = np.roll(np.concatenate([x] * (1 + n // x.shape[1]), axis=1), 137 * (i + 1), axis=1)[:, :n]
        path = str(tmp_path / f"variant_{i}_{n}.wav")
        audio_io.write_wav(path, np.ascontiguousarray(y.T), sr, "PCM_16")
        paths.append(path)
    return paths


def _loop(A, members, paths, out_dir, algorithm, weights=None, **kw):
    ens = A.EnsembleSeparator(members, algorithm, weights, **kw)
    ens.output_dir = out_dir
    files = []
    for p in paths:
        files.append(ens.separate(p))
        assert ens.last_path_taken == "device"
    return files


def _same_files(got, want, got_dir, want_dir):
    assert [[os.path.relpath(f, got_dir) for f in fs] for fs in got] == [[os.path.relpath(f, want_dir) for f in fs] for fs in want]
    for fs_got, fs_want in zip(got, want):
        for a, b in zip(fs_got, fs_want):
            assert os.path.isfile(a) and os.path.isfile(b), (a, b)
            assert filecmp.cmp(a, b, shallow=False), os.path.basename(a)


@pytest.fixture(scope="module")
def trio_files(members_44k, tmp_path_factory):  # noqa: F811
    members, wav = members_44k
    chunk = members[2]._demixer(True).chunk_size           # the files are shorter than 10 s: the configured segment size
    lengths = (2817, 4100)
    assert all(n >= chunk for n in lengths + (3000,)), chunk
    return _variants(wav, tmp_path_factory.mktemp("trio"), lengths, 44100)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_separate_many_equals_separate_per_path(members_44k, trio_files, tmp_path, monkeypatch, algorithm):  # noqa: F811
    import audio_separator_amd as A
    members, _ = members_44k
    weights = [1.0, 2.0, 0.5] if algorithm.startswith("avg_") else None
    want = _loop(A, members, trio_files, str(tmp_path / "loop"), algorithm, weights)
    assert all(len(fs) == 2 for fs in want)

    ens = A.EnsembleSeparator(members, algorithm, weights)
    ens.output_dir = str(tmp_path / "batch")
    counts = {}

    def counted(obj, name, key, forbidden=False):
        real = getattr(obj, name)

        def wrapper(*a, **k):
            counts[key] = counts.get(key, 0) + 1
            assert not forbidden, f"{key} must not run during separate_many"
            return real(*a, **k)
        monkeypatch.setattr(obj, name, wrapper)
    with monkeypatch.context():
        counted(tempfile, "mkdtemp", "mkdtemp", forbidden=True)
        for i, m in enumerate(members):
            counted(m, "stems_dev", f"stems_dev {i}", forbidden=True)
            counted(m, "_pooled_stems", f"pooled {i}")
            counted(m, "write_audio", f"write {i}")
        engine = members[-1].engine
        counted(engine, "ensemble_batch_dev", "batch")
        counted(engine, "ensemble_slot_dev", "slot", forbidden=True)
        counted(engine, "ensemble_dev", "combine", forbidden=True)
        got = ens.separate_many(trio_files)
    assert counts == {"pooled 0": 1, "pooled 1": 1, "pooled 2": 1, "batch": 1, "write 2": sum(len(fs) for fs in want)}, counts
    assert ens.last_paths_taken == ["device"] * 3 and ens.batch_errors == {}
    _same_files(got, want, ens.output_dir, str(tmp_path / "loop"))


@pytest.mark.parametrize("algorithm", ["avg_wave", "uvr_max_spec"])
def test_separate_many_unequal_lengths_and_lone_groups(members_8k, tmp_path, monkeypatch, algorithm):  # noqa: F811
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    members, wav = members_8k
    monkeypatch.setattr(random, "randint", lambda a, b: a + (b - a) // 3)      # the Demucs shift draws, as the existing test pins them
    n = audio_io.wav_info(wav)["frames"]
    paths = _variants(wav, tmp_path, (n - 1111,), 8000)
    want = _loop(A, members, paths, str(tmp_path / "loop"), algorithm)
    assert all(len(fs) == 5 for fs in want)                  # Bass, Drums, Other, Vocals (two contributors), Instrumental
    ens = A.EnsembleSeparator(members, algorithm)
    ens.output_dir = str(tmp_path / "batch")
    got = ens.separate_many(paths)
    assert ens.last_paths_taken == ["device", "device"]
    _same_files(got, want, ens.output_dir, str(tmp_path / "loop"))


def test_separate_many_files_fail_alone(members_44k, trio_files, tmp_path):  # noqa: F811
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    members, _ = members_44k
    missing = str(tmp_path / "no_such_file.wav")
    other_rate = str(tmp_path / "at_22050.wav")
    x, _ = audio_io.read_wav(trio_files[0])
    audio_io.write_wav(other_rate, np.ascontiguousarray(x.T), 22050, "PCM_16")
    paths = [trio_files[0], missing, trio_files[1], other_rate]
    want = _loop(A, members, [paths[0], paths[2]], str(tmp_path / "loop"), "max_fft")
    ens = A.EnsembleSeparator(members, "max_fft")
    ens.output_dir = str(tmp_path / "batch")
    got = ens.separate_many(paths)
    _same_files([got[0], got[2]], want, ens.output_dir, str(tmp_path / "loop"))
    assert got[1] == [] and isinstance(ens.batch_errors[1], OSError)
    # a WAV at another rate is the host decoder's: without librosa it cannot resample, so the file fails (with it, the file path)
    if audio_io._optional("librosa") is None:
        assert got[3] == [] and isinstance(ens.batch_errors[3], audio_io.AudioIOError)
        assert ens.last_paths_taken == ["device", "failed", "device", "failed"] and sorted(ens.batch_errors) == [1, 3]
    else:
        assert len(got[3]) == 2 and ens.last_paths_taken == ["device", "failed", "device", "files"] and sorted(ens.batch_errors) == [1]


def test_pool_files_gives_the_same_bytes(members_44k, trio_files, tmp_path, monkeypatch):  # noqa: F811
    import audio_separator_amd as A
    members, _ = members_44k
    whole = A.EnsembleSeparator(members, "median_fft")
    whole.output_dir = str(tmp_path / "whole")
    want = whole.separate_many(trio_files)
    split = A.EnsembleSeparator(members, "median_fft", pool_files=1)
    split.output_dir = str(tmp_path / "split")
    calls = []
    real = members[-1].engine.ensemble_batch_dev
    monkeypatch.setattr(members[-1].engine, "ensemble_batch_dev", lambda jobs, *a, **k: calls.append(len(jobs)) or real(jobs, *a, **k))
    got = split.separate_many(trio_files)
    assert calls == [2, 2, 2]                               # one run per file, two stem groups each
    _same_files(got, want, split.output_dir, whole.output_dir)
    with pytest.raises(ValueError, match="pool_files"):
        A.EnsembleSeparator(members, "median_fft", pool_files=0)
