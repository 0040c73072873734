"""The slot modes of the soundfile writer's formats and the pooled ensemble with a mode per contributor, on the MI355X.

1. asx_ensemble_slot_dev under "PCM_16" / "PCM_24" / "PCM_32" / "FLOAT" against its definition: the float32 array asx_pcm_decode_dev
   returns for the bytes asx_pcm_encode_dev writes for the same stem, layout and thresholds -- bit for bit, with the peak that call
   reports and the zero padding; and against the numpy restatement tests/ensemble_slot_ref.py (which the host tests pin to the files).
2. asx_ensemble_batch_modes_dev against asx_ensemble_slot_dev per contributor (each with its own mode) + asx_ensemble_dev, bit for bit,
   for all eleven algorithms, with mixed modes inside one job; and against asx_ensemble_batch_dev where the modes are uniform.
3. refusals."""
import numpy as np
import pytest

from tests import ensemble_slot_ref as SR

pytestmark = pytest.mark.gpu

ALGORITHMS = ("avg_wave", "median_wave", "min_wave", "max_wave", "avg_fft", "median_fft", "min_fft", "max_fft", "uvr_max_spec",
              "uvr_min_spec", "ensemble_wav")
SILENT = 1e-6
SLACK = 300
P, R = "planar", "rows"


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    return A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))


def _stem(n, amplitude, seed):
    """[2, n] with the peak exactly ``amplitude`` (negative, at one sample) and, from four frames on, +-amplitude / 2, + amplitude and a
    zero: under a scale of exactly 1, 0.5 or 2 they become the exact ties +-0.5 and +-peak of the quantiser."""
    rng = np.random.default_rng(seed)
    x = (np.float32(amplitude) * rng.uniform(-1.0, 1.0, (2, n)).astype(np.float32)).astype(np.float32)
    if n >= 4:
        half = np.float32(amplitude) * np.float32(0.5)
        x[0, :4] = half, -half, np.float32(amplitude), 0.0
        x[1, :4] = -half, half, 0.0, np.float32(amplitude)
    x[n % 2, n // 2] = -np.float32(amplitude)
    return x


# ---- 1. the slot image -----------------------------------------------------------------------------------------------------------
# (amplitude, max_peak, min_peak): above max_peak with an inexact scale; below a set min_peak with an inexact scale; between the two;
# beyond full scale unscaled (clips); then the three whose normalised peak is exactly 1 -- unscaled, above with a scale of exactly 0.5,
# below with a scale of exactly 2 -- so that the peak lands on 2^(b-1) - 1 and the half-amplitude samples on the exact ties +-0.5
REGIMES = ((1.7, 0.9, None), (0.2, 0.9, 0.5), (0.7, 0.9, 0.5), (1.05, 1.1, 0.0), (1.0, 1.0, None), (2.0, 1.0, None), (0.5, 1.0, 1.0))


@pytest.mark.parametrize("layout", [P, R])
@pytest.mark.parametrize("mode", SR.FILE_MODES)
def test_slot_image_is_encode_then_decode(eng, mode, layout):
    import torch
    dev = torch.device("cuda", 0)
    frame_bytes = {"PCM_16": 4, "PCM_24": 6, "PCM_32": 8, "FLOAT": 8}[mode]
    for n in (1, 255, 256, 257, 1000):
        for r, (amplitude, max_peak, min_peak) in enumerate(REGIMES):
            x = _stem(n, amplitude, 100 * n + r)
            stem = torch.from_numpy(np.ascontiguousarray(x if layout == P else x.T)).to(dev)
            body = torch.zeros(n * frame_bytes + 16, dtype=torch.uint8, device=dev)
            peak_ref = eng.pcm_encode_dev(stem.data_ptr(), n, layout, max_peak, min_peak, mode, body.data_ptr())
            back = torch.empty((2, n), dtype=torch.float32, device=dev)
            eng.pcm_decode_dev(body.data_ptr(), n, 2, mode, back.data_ptr())
            torch.cuda.synchronize()
            back = back.cpu().numpy()
            where = (mode, layout, n, amplitude)
            ref, ref_peak = SR.round_trip(x, mode, max_peak, min_peak)
            assert np.array_equal(back.view(np.uint32), ref.view(np.uint32)), where        # the restatement is this pair of calls
            assert np.float32(peak_ref) == ref_peak, where
            for n_max in (n, n + 37):
                want = np.zeros((2, n_max), np.float32)
                want[:, :n] = back
                stack = torch.full((3, 2, n_max), float("nan"), dtype=torch.float32, device=dev)
                peak = eng.ensemble_slot_dev(stem.data_ptr(), n, layout, max_peak, min_peak, stack.data_ptr(), 1, n_max, mode=mode)
                got = stack.cpu().numpy()
                assert np.array_equal(got[1].view(np.uint32), want.view(np.uint32)), (where, n_max)
                assert np.isnan(got[0]).all() and np.isnan(got[2]).all(), (where, n_max)   # the neighbours are not touched
                assert peak == peak_ref, (where, peak, peak_ref)
            if n >= 4 and max_peak == 1.0 and mode != "FLOAT":
                # the ties and the peak did reach the quantiser as such: +-0.5 -> +-2^(b-2) (half to even), 1 -> 2^(b-1) - 1
                bits = SR.FILE_BITS[mode]
                top = np.float32(np.float64((1 << (bits - 1)) - 1) / (1 << (bits - 1)))
                assert peak_ref == 1.0 and back[0, 0] == 0.5 and back[0, 1] == -0.5 and back[0, 2] == top and back.min() == -top, where


def test_file_pcm16_rounds_where_pcm16_truncates(eng):
    import torch
    dev = torch.device("cuda", 0)
    x = np.full((2, 8), 0.7, np.float32)                         # 0.7 * 32767 = 22936.9
    stem = torch.from_numpy(x).to(dev)
    stack = torch.empty((2, 2, 8), dtype=torch.float32, device=dev)
    eng.ensemble_slot_dev(stem.data_ptr(), 8, P, 0.9, None, stack.data_ptr(), 0, 8, mode="pcm16")
    eng.ensemble_slot_dev(stem.data_ptr(), 8, P, 0.9, None, stack.data_ptr(), 1, 8, mode="PCM_16")
    got = stack.cpu().numpy()
    assert (got[0] == np.float32(22936 / 32768)).all() and (got[1] == np.float32(22937 / 32768)).all()


# ---- 2. the pooled call with a mode per contributor ------------------------------------------------------------------------------------
# job -> [(n, layout, amplitude, mode)]; amplitudes under max_peak 0.9: 1.7 above, 0.2 below a min_peak of 0.5, 0.7 between, 0.0 all
# zeros, 5e-7 not zero but silent (below 1e-6 unless a set min_peak amplifies it)
MAX_PEAK = 0.9
JOBS = (
    [(1023, P, 0.7, "pcm16"), (1023, R, 1.7, "PCM_24")],                              # K = 2, below one hop: no result under uvr_*
    [(1024, R, 1.7, "PCM_24"), (1024, P, 0.7, "FLOAT")],                              # K = 2, one hop exactly
    [(2049, P, 0.7, "pcm16"), (1024, R, 1.7, "PCM_24"), (1023, P, 0.2, "FLOAT")],     # K = 3, the three modes, unequal lengths
    [(2049, R, 1.7, "FLOAT"), (2049, P, 0.2, "PCM_32"), (2049, R, 0.7, "PCM_16")],    # K = 3, equal lengths, the other formats
    [(2049, P, 0.0, "PCM_24"), (1023, R, 0.7, "pcm16"), (1024, P, 1.7, "FLOAT")],     # the LONGEST is silent: dropped, n_max shrinks
    [(1000, R, 0.7, "PCM_24")],                                                       # a lone contributor: its slot image
    [(256, P, 0.0, "FLOAT"), (1, R, 0.0, "PCM_16")],                                  # none left
    [(3000, R, 0.0, "pcm16"), (1025, P, 0.7, "PCM_32")],                              # one left after the drop
    [(257, P, 0.7, "float32"), (257, R, 1.7, "PCM_16")],                              # the unquantised mode beside a file mode
    [(500, P, 5e-7, "FLOAT"), (700, R, 0.7, "PCM_24"), (600, P, 5e-7, "pcm16")],      # silent by the rule, not by being zero
)
EDGES = ((0.5, False), (0.0, True), (None, True))              # (min_peak, keep the all-zero stems?) as in tests/test_gpu_ensemble_batch.py


def _device_jobs(keep_zeros, dev):
    import torch
    jobs = []
    for j, spec in enumerate(JOBS):
        contributors = []
        for c, (n, layout, amplitude, mode) in enumerate(spec):
            if amplitude == 0.0 and not keep_zeros:
                amplitude = 0.2                                  # (a set min_peak would scale a zero stem by inf, which no file meets)
            x = _stem(n, amplitude, 1000 * j + c)
            contributors.append((torch.from_numpy(np.ascontiguousarray(x if layout == P else x.T)).to(dev), n, layout, mode))
        jobs.append(contributors)
    return jobs


def _per_job_reference(eng, contributors, algorithm, weights, min_peak):
    """EnsembleSeparator._separate_on_device for one stem group -> (result bits or None, n_out, peak per contributor, live)"""
    import torch
    live = list(range(len(contributors)))
    peaks_all = [None] * len(contributors)
    stack = None
    while live:
        n_max = max(contributors[c][1] for c in live)
        stack = torch.empty((len(live), 2, n_max), dtype=torch.float32, device=contributors[0][0].device)
        peaks = [eng.ensemble_slot_dev(contributors[c][0].data_ptr(), contributors[c][1], contributors[c][2], MAX_PEAK, min_peak,
                                       stack.data_ptr(), slot, n_max, mode=contributors[c][3]) for slot, c in enumerate(live)]
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


def _pooled(eng, jobs, algorithm, weights, min_peak, **how):
    """``how``: nothing (the modes of the jobs' contributors, the new call) or ``mode=`` (the old call)"""
    import torch
    outs = []
    for contributors in jobs:
        cap = max(c[1] for c in contributors) + SLACK
        outs.append(torch.full((2 * cap,), float("nan"), dtype=torch.float32, device=contributors[0][0].device))
    if not how:
        how = {"modes": [[c[3] for c in contributors] for contributors in jobs]}
    got = eng.ensemble_batch_dev([([(c[0].data_ptr(), c[1], c[2]) for c in contributors], out.data_ptr(), out.numel() // 2)
                                  for contributors, out in zip(jobs, outs)], algorithm, weights, MAX_PEAK, min_peak, SILENT, **how)
    torch.cuda.synchronize()
    return got, [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_pooled_modes_equal_the_per_job_calls(eng, algorithm):
    import torch
    dev = torch.device("cuda", 0)
    weight_lists = ([1.0, 2.0, 0.5], [3.0, 1.0]) if algorithm.startswith("avg_") else (None,)
    uvr = algorithm.startswith("uvr_")
    for min_peak, zeros in EDGES:
        jobs = _device_jobs(zeros, dev)
        for weights in weight_lists:
            want = [_per_job_reference(eng, c, algorithm, weights, min_peak) for c in jobs]
            got, bufs = _pooled(eng, jobs, algorithm, weights, min_peak)
            for j, ((bits, n_out, peaks, live), (g_n, g_live, g_peaks), buf) in enumerate(zip(want, got, bufs)):
                where = (algorithm, min_peak, weights, j)
                assert (g_n, g_live) == (n_out, live), where
                assert g_peaks == peaks, (where, g_peaks, peaks)
                if bits is not None:
                    assert np.array_equal(buf[: 2 * n_out].view(np.uint32), bits), where
                assert np.isnan(buf[2 * n_out:]).all(), where                   # the slack, and every buffer of a job without a result
            if zeros:
                assert [g[1] for g in got] == [2, 2, 3, 3, 2, 1, 0, 1, 2, 1]
                assert [g[0] for g in got] == ([0, 1024, 2048, 2048, 1024, 1000, 0, 1025, 0, 700] if uvr else
                                               [1023, 1024, 2049, 2049, 1024, 1000, 0, 1025, 257, 700])
            else:
                assert [g[1] for g in got] == [len(spec) for spec in JOBS]      # a set min_peak amplifies every quiet stem: all take part
            # one job alone gives the bits it gives in the pool
            one, buf1 = _pooled(eng, [jobs[2]], algorithm, weights, min_peak)
            assert one[0] == got[2] and np.array_equal(buf1[0].view(np.uint32), bufs[2].view(np.uint32)), (algorithm, min_peak)


@pytest.mark.parametrize("algorithm", ALGORITHMS)
def test_uniform_modes_equal_the_old_call(eng, algorithm):
    import torch
    dev = torch.device("cuda", 0)
    weights = [1.0, 2.0, 0.5] if algorithm.startswith("avg_") else None
    for min_peak, zeros in EDGES[:2]:
        base = _device_jobs(zeros, dev)
        for mode in ("pcm16", "float32") + SR.FILE_MODES:
            jobs = [[(t, n, layout, mode) for t, n, layout, _ in contributors] for contributors in base]
            new, bufs_new = _pooled(eng, jobs, algorithm, weights, min_peak)
            old, bufs_old = _pooled(eng, jobs, algorithm, weights, min_peak, mode=mode)
            assert new == old, (algorithm, mode, min_peak)
            assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(bufs_new, bufs_old)), (algorithm, mode, min_peak)
            assert any(g[0] > 0 for g in new)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_unknown_modes_are_refused_before_anything_runs(eng, monkeypatch):
    import torch
    import audio_separator_amd as A
    dev = torch.device("cuda", 0)
    stem = torch.ones((2, 64), dtype=torch.float32, device=dev)
    outs = [torch.full((2 * 364,), float("nan"), dtype=torch.float32, device=dev) for _ in range(2)]
    jobs = [([(stem.data_ptr(), 64, P), (stem.data_ptr(), 64, P)], o.data_ptr(), 364) for o in outs]
    for call in (lambda: eng.ensemble_batch_dev(jobs, "avg_wave", None, 0.9, 0.0, modes=[["pcm16", "PCM_24"], ["pcm16", "DOUBLE"]]),
                 lambda: eng.ensemble_batch_dev(jobs, "avg_wave", None, 0.9, 0.0, mode="DOUBLE"),
                 lambda: eng.ensemble_slot_dev(stem.data_ptr(), 64, P, 0.9, 0.0, outs[0].data_ptr(), 0, 64, mode="PCM_U8")):
        with pytest.raises(ValueError, match="unknown slot mode"):
            call()
    # a number the library does not know (the wrapper would not let it through): refused there, naming the job and the contributor
    monkeypatch.setitem(A.Engine.SLOT_MODES, "bogus", 7)
    with pytest.raises(A.AsxError, match=r"asx_ensemble_batch_modes_dev: job 1: contributor 1 has mode 7\b"):
        eng.ensemble_batch_dev(jobs, "avg_wave", None, 0.9, 0.0, modes=[["pcm16", "PCM_24"], ["FLOAT", "bogus"]])
    with pytest.raises(A.AsxError, match=r"asx_ensemble_batch_dev: mode 7\b"):
        eng.ensemble_batch_dev(jobs, "avg_wave", None, 0.9, 0.0, mode="bogus")
    with pytest.raises(A.AsxError, match=r"asx_ensemble_slot_dev: mode 7\b"):
        eng.ensemble_slot_dev(stem.data_ptr(), 64, P, 0.9, 0.0, outs[0].data_ptr(), 0, 64, mode="bogus")
    # the other argument checks of the old call hold for the new one, under its own name
    with pytest.raises(A.AsxError, match=r"asx_ensemble_batch_modes_dev: job 1\b"):
        eng.ensemble_batch_dev([jobs[0], ([(stem.data_ptr(), 64, P)], outs[1].data_ptr(), 63)], "avg_wave", None, 0.9, 0.0,
                               modes=[["pcm16", "PCM_24"], ["FLOAT"]])
    torch.cuda.synchronize()
    assert all(torch.isnan(o).all() for o in outs)
    assert eng.ensemble_batch_dev([], "avg_wave", None, 0.9, 0.0, modes=[]) == []
    assert eng.ensemble_batch_dev(jobs, "avg_wave", None, 0.9, 0.0, modes=[["pcm16", "PCM_24"], ["FLOAT", "PCM_32"]])[1][:2] == (64, 2)
