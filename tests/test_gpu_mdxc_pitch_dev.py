"""MDXC ``pitch_shift`` with every array in HBM: asx_resample_sinc_batch_dev, ``MDXCDemixer.demix_many_dev`` and the plugin's device file
path, pooled and in ensembles.

Nothing here is held to a tolerance.  The pooled converter runs the single call's per-frame code with the single call's arguments, the
pooled demix is bit-identical to the single-song call (tests/test_gpu_mdxc_batch.py), the ratios are formed by
``change_pitch_semitones``' own expressions, and ``mix - primary`` is one IEEE subtraction: every output must EQUAL the host-array path's,
compared on the uint32 view, and every written file its bytes."""
import filecmp
import math
import os

import numpy as np
import pytest

from tests import separate_cases as SC
from tests import test_gpu_mdxc as TM
from tests import test_gpu_roformer as TR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def passes(nk, max_b):
    nbatch = -(-nk // max_b)
    return -(-nk // -(-nk // nbatch))


# ---- 1. the pooled converter against the single call -------------------------------------------------------------------------------
N_IN = (1, 2, 255, 256, 257, 1000, 4999)
CHANNELS = (1, 2, 8)
RATIOS = [2.0 ** (2 / 12), 2.0 ** (-2 / 12), 2.0 ** (7 / 12), 2.0 ** (-7 / 12), 0.5, 2.0]


def sinc_jobs(ratio):
    """(n_in, channels, n_out): every n_in x channels at n_out = ceil, ceil - 3 and ceil + 300, plus the workgroup edges 1, 255, 256, 257
    as n_out -- 67 jobs, more than one group of the table launch"""
    jobs = []
    for n_in in N_IN:
        for ch in CHANNELS:
            c = int(math.ceil(n_in * ratio))
            jobs += [(n_in, ch, c), (n_in, ch, max(1, c - 3)), (n_in, ch, c + 300)]
    return jobs + [(1000, 2, n_out) for n_out in (1, 255, 256, 257)]


@pytest.fixture(scope="module")
def plain_engine(A):
    eng = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def sinc_inputs():
    import torch
    rng = np.random.default_rng(1234)
    return {(n, ch): torch.from_numpy(rng.standard_normal((ch, n)).astype(np.float32)).cuda() for n in N_IN for ch in CHANNELS}


@pytest.mark.parametrize("ratio", RATIOS)
def test_batch_converter_equals_the_single_call(plain_engine, sinc_inputs, ratio):
    import torch
    eng, st = plain_engine, torch.cuda.current_stream().cuda_stream
    jobs = sinc_jobs(ratio)
    assert len(jobs) == 67

    def nan_outputs():
        return [torch.full((ch, n_out), float("nan"), dtype=torch.float32, device="cuda") for _, ch, n_out in jobs]

    for mono in (False, True):
        want = nan_outputs()
        for (n_in, ch, n_out), y in zip(jobs, want):
            eng.resample_sinc_dev(sinc_inputs[n_in, ch].data_ptr(), ch, n_in, ratio, mono, y.data_ptr(), n_out, stream=st)
        runs = []
        for _ in range(2):
            got = nan_outputs()
            eng.resample_sinc_batch_dev([(sinc_inputs[n_in, ch].data_ptr(), y.data_ptr(), n_in, n_out, ch) for (n_in, ch, n_out), y in zip(jobs, got)],
                                        ratio, mono, stream=st)
            runs.append(got)
        torch.cuda.synchronize()
        moved = 0
        for job, w, g, g2 in zip(jobs, want, *runs):
            w, g, g2 = w.cpu().numpy(), g.cpu().numpy(), g2.cpu().numpy()
            assert np.isfinite(w).all(), job
            assert same_bits(g, w), (ratio, mono, job)
            assert same_bits(g2, g), (ratio, mono, job)                       # a second run: the same bits
            n_in, ch, n_out = job
            t = n_in * ratio
            n_gen = int(t) - (1 if (mono or ch == 1) and int(t) == t and int(t) > 0 else 0)
            assert not g[:, n_gen:].any()                                       # frames the library does not generate are zero
            moved += int(np.count_nonzero(g))
        assert moved > 0


def test_batch_converter_checks_every_job_before_it_runs(A, plain_engine, sinc_inputs):
    import torch
    eng = plain_engine
    x = sinc_inputs[1000, 2]
    outs = [torch.full((2, 1200), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    good = [(x.data_ptr(), o.data_ptr(), 1000, 1200, 2) for o in outs]
    xp, yp = good[1][0], good[1][1]
    for bad, ratio, text in (((0, yp, 1000, 1200, 2), 1.1, "job 1: null input or output"), ((xp, 0, 1000, 1200, 2), 1.1, "job 1: null input or output"),
                             ((xp, yp, 0, 1200, 2), 1.1, r"job 1: n_in = 0 "), ((xp, yp, 1000, 0, 2), 1.1, r"job 1: n_out = 0 "),
                             ((xp, yp, 1000, 1200, 0), 1.1, "job 1: 0 channels"), ((xp, yp, 1000, 1200, 65536), 1.1, "job 1: 65536 channels"),
                             (good[1], 1.0 / 256, "ratio 0.00390625 outside"), (good[1], 256.0, "ratio 256 outside"),
                             (good[1], float("nan"), "ratio nan outside")):
        with pytest.raises(A.AsxError, match="asx_resample_sinc_batch_dev: " + text):
            eng.resample_sinc_batch_dev([good[0], bad, good[2]], ratio, True)
    with pytest.raises(A.AsxError, match="65536 jobs in one call"):
        eng.resample_sinc_batch_dev([good[0]] * 65536, 1.1, True)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(o).all()) for o in outs)                        # nothing was enqueued
    eng.resample_sinc_batch_dev([], 1.1, True)                                  # an empty list is valid
    lib = A.engine.load_library()
    assert lib.asx_resample_sinc_batch_dev(None, None, 0, 1.1, 1, None) != 0     # a null engine is an error
    assert lib.asx_resample_sinc_batch_dev(eng._h, None, 1, 1.1, 1, None) != 0 and b"null job list" in lib.asx_last_error()


# ---- 2. demix_many_dev against demix ------------------------------------------------------------------------------------------------
def down_ratio(sr, pitch_shift):
    target = sr * 2 ** (-pitch_shift / 12)            # spec_utils.change_pitch_semitones(mix, sr, -pitch_shift)
    return float(target) / sr


def pitched_len(n, ratio):
    return int(np.ceil(n * ratio))


def shortest_with(ratio, want):
    """the shortest song whose pitched length is at least ``want``"""
    n = max(1, int(want / ratio) - 3)
    while pitched_len(n, ratio) < want:
        n += 1
    return n


def song_lengths(ratio, chunk, under):
    """songs whose PITCHED lengths fall under one chunk (``under``), on exactly one chunk, just over it, and across several"""
    exact, over, several = shortest_with(ratio, chunk), shortest_with(ratio, chunk + 1), shortest_with(ratio, 4 * chunk + 17)
    assert pitched_len(exact, ratio) == chunk and chunk < pitched_len(over, ratio) <= chunk + 2
    lengths = [exact, over, several]
    if under:
        lengths.insert(0, exact - 1)
        assert pitched_len(exact - 1, ratio) < chunk
    return lengths


def make_demixer(A, net, single_target, pitch_shift):
    if net == "tfc":
        return TM.demixer(A, TM.CFG1 if single_target else TM.CFG2, 6 if single_target else 5, 4, max_batch=5, pitch_shift=pitch_shift)
    cfg, seed = (TR.CFG, 7) if single_target else (TR.CFG2, 8)
    return A.MDXCDemixer({"model_data": cfg.as_model_data(), "torch_device": 0, "secondary_stem_name": cfg.instruments[1]},
                         {"overlap": 2, "pitch_shift": pitch_shift}, state_dict=TR.R.make_roformer_state(cfg, seed), max_batch=3)


@pytest.mark.parametrize("pitch_shift", [2, -3])
@pytest.mark.parametrize("single_target", [True, False])
@pytest.mark.parametrize("net", ["tfc", "rof"])
def test_demix_many_dev_equals_demix(A, net, single_target, pitch_shift):
    import torch
    dm = make_demixer(A, net, single_target, pitch_shift)
    try:
        chunk, max_b = (240, 5) if net == "tfc" else (320, 3)
        assert dm.chunk_size == chunk and dm.is_primary_stem_main_target == single_target
        ratio = down_ratio(dm.sample_rate, pitch_shift)
        assert dm.pitch_ratios()[0] == ratio
        lengths = song_lengths(ratio, chunk, under=net == "tfc")
        pitched = [pitched_len(n, ratio) for n in lengths]
        assert [dm.pitched_len(n) for n in lengths] == pitched
        mixes = [(0.4 * np.random.default_rng(900 + i).standard_normal((2, n))).astype(np.float32) for i, n in enumerate(lengths)]
        counter = "v3_net_passes" if net == "tfc" else "rof_net_passes"
        n0 = dm.engine.counter(counter)
        want = [dm.demix(m) for m in mixes]
        n1 = dm.engine.counter(counter)
        res = dm.demix_many_dev([torch.from_numpy(m).cuda() for m in mixes])
        torch.cuda.synchronize()
        n2 = dm.engine.counter(counter)
        assert len(res) == len(mixes)
        for i, (w, (names, stems_d)) in enumerate(zip(want, res)):
            assert list(w) == names and len(names) == 2 and tuple(stems_d.shape) == (2, 2, lengths[i])
            for r, k in enumerate(names):
                got = stems_d[r].cpu().numpy()
                assert np.isfinite(got).all() and same_bits(got, w[k]), (i, lengths[i], pitched[i], k)
            assert float(np.abs(w[names[0]]).max()) > 0
        if net == "tfc":
            counts = [dm.engine.mdxc_plan(n, 4)["n_chunks"] for n in pitched]
        else:
            counts = [-(-n // dm.roformer_step()) for n in pitched]
        print(net, "single" if single_target else "multi", pitch_shift, "songs", lengths, "pitched", pitched, "chunks", counts,
              "passes pooled / single", n2 - n1, n1 - n0)
        assert n1 - n0 == sum(passes(c, max_b) for c in counts) and n2 - n1 == passes(sum(counts), max_b)
        assert n2 - n1 < n1 - n0
        one = dm.demix_dev(torch.from_numpy(mixes[1]).cuda())                   # demix_dev is the pool of one
        torch.cuda.synchronize()
        assert one[0] == res[1][0] and same_bits(one[1].cpu().numpy(), res[1][1].cpu().numpy())
    finally:
        dm.engine.close()


@pytest.mark.parametrize("pitch_shift", [2, -3])
def test_roformer_song_one_sample_short_of_a_chunk_is_refused_by_index(A, pitch_shift):
    import torch
    dm = make_demixer(A, "rof", True, pitch_shift)
    try:
        ratio = down_ratio(dm.sample_rate, pitch_shift)
        exact = shortest_with(ratio, 320)
        assert pitched_len(exact, ratio) == 320 and pitched_len(exact - 1, ratio) == 319
        lengths = [exact + 100, exact, exact - 1, exact + 7]
        mixes_d = [torch.from_numpy((0.4 * np.random.default_rng(950 + i).standard_normal((2, n))).astype(np.float32)).cuda()
                   for i, n in enumerate(lengths)]
        n0 = dm.engine.counter("rof_net_passes")
        with pytest.raises(ValueError, match=r"song 2: pitched mix \(319 samples\) shorter than one chunk \(320\)"):
            dm.demix_many_dev(mixes_d)
        torch.cuda.synchronize()
        assert dm.engine.counter("rof_net_passes") == n0                         # before anything ran
        assert len(dm.demix_many_dev(mixes_d[:2] + mixes_d[3:])) == 3
        torch.cuda.synchronize()
    finally:
        dm.engine.close()


# ---- 3. files -----------------------------------------------------------------------------------------------------------------------
FILE_CASES = [("mdxc", 0), ("mdxc", 1), ("roformer", 0)]      # two stems, single target with its residual, BS-Roformer


def _plugin(tmp, family, idx, out_dir, arch_over=None, **common_over):
    _, cls, common, arch, wav, _ = SC.cases(family, str(tmp))[idx]
    arch = dict(arch, pitch_shift=2, **(arch_over or {}))
    return SC.plugin_class(cls)(common_config=dict(common, output_dir=str(out_dir), **common_over), arch_config=arch), wav


def _blobs(out_dir, names):
    assert names
    return [open(os.path.join(str(out_dir), n), "rb").read() for n in names]


def _cut(tmp_path, wav, n, subtype="PCM_16"):
    """the first ``n`` frames of the 16-bit ``wav``; "DOUBLE": the same samples as 64-bit floats, a file only the host decoder takes"""
    from audio_separator_amd import audio_io
    x, sr = audio_io.read_wav(wav)
    p = str(tmp_path / f"song_{n}_{subtype}.wav")
    if subtype == "DOUBLE":
        audio_io.write_wav(p, np.ascontiguousarray(x[:, :n].T.astype(np.float64)), sr, "DOUBLE")
    else:
        audio_io.write_wav(p, np.ascontiguousarray(np.rint(x[:, :n].T.astype(np.float64) * 32768.0), np.int16), sr, subtype)
    return p


def _chunk_counts(dm, lengths):
    if dm.is_roformer:
        return [-(-n // dm.roformer_step()) for n in lengths]
    return [dm.engine.mdxc_plan(n, int(dm.overlap))["n_chunks"] for n in lengths]


def _greedy_runs(costs, budget):
    """consecutive runs, in order, within ``budget``; a file that alone exceeds it is a run of its own"""
    runs, used = [[]], 0
    for i, c in enumerate(costs):
        if runs[-1] and used + c > budget:
            runs.append([])
            used = 0
        runs[-1].append(i)
        used += c
    return runs


@pytest.mark.parametrize("family,idx", FILE_CASES)
def test_separate_equals_the_host_path(tmp_path, monkeypatch, family, idx):
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")

    def run(fast):
        monkeypatch.setenv("ASX_FILE_FASTPATH", "1" if fast else "0")
        out = tmp_path / ("dev" if fast else "host")
        inst, wav = _plugin(tmp_path, family, idx, out, asx_profile_file=True)
        names = inst.separate(wav, None)
        got = names, _blobs(out, names), dict(inst.file_timings)
        inst.clear_gpu_cache()
        return got
    names_d, blobs_d, t_d = run(True)
    assert "h2d_decode" in t_d and "demix" in t_d and "stems_d2h" in t_d, t_d      # the device path took the file
    names_h, blobs_h, t_h = run(False)
    assert "h2d_decode" not in t_h and "stems_d2h" not in t_h, t_h
    assert names_d == names_h and len(names_d) == 2 and blobs_d == blobs_h


@pytest.mark.parametrize("family,idx", FILE_CASES)
def test_separate_many_equals_the_per_file_loop(tmp_path, monkeypatch, family, idx):
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    from audio_separator_amd import audio_io
    from audio_separator_amd.mdxc import MDXCDemixer
    loop, wav = _plugin(tmp_path, family, idx, tmp_path / "loop", arch_over={"asx_max_batch": 5})
    full = audio_io.wav_info(wav)["frames"]
    lengths = [full, full - 123, full - 300]
    # the last file is one only the host decoder takes: it joins the pool after upload
    paths = [wav, _cut(tmp_path, wav, lengths[1]), _cut(tmp_path, wav, lengths[2], "DOUBLE")]
    want = []
    for p in paths:
        want.append(loop.separate(p, None))
        loop.clear_file_specific_paths()
    loop.clear_gpu_cache()
    calls = []
    pooled_call = MDXCDemixer.demix_many_dev
    monkeypatch.setattr(MDXCDemixer, "demix_many_dev", lambda self, mixes_d: calls.append(len(mixes_d)) or pooled_call(self, mixes_d))
    pooled, _ = _plugin(tmp_path, family, idx, tmp_path / "pooled", arch_over={"asx_max_batch": 5})
    got = pooled.separate_many(paths)
    assert pooled.batch_errors == {} and got == want and calls == [3]              # one pooled call for the three files
    for names in got:
        assert _blobs(tmp_path / "pooled", names) == _blobs(tmp_path / "loop", names)
    # asx_pool_chunks splits the pool by the chunks of the PITCHED mixes: a budget that holds the first two files' pitched chunks exactly,
    # which their unpitched chunks would exceed
    dm = pooled._demixer()
    ratio = down_ratio(dm.sample_rate, 2)
    pitched_counts = _chunk_counts(dm, [pitched_len(n, ratio) for n in lengths])
    budget = pitched_counts[0] + pitched_counts[1]
    assert sum(_chunk_counts(dm, lengths)[:2]) > budget
    del calls[:]
    split, _ = _plugin(tmp_path, family, idx, tmp_path / "split", arch_over={"asx_max_batch": 5, "asx_pool_chunks": budget})
    assert split.separate_many(paths) == want and calls == [2, 1] == [len(r) for r in _greedy_runs(pitched_counts, budget)]
    for names in got:
        assert _blobs(tmp_path / "split", names) == _blobs(tmp_path / "loop", names)
    # and the same batch without the device file path: the loop of demix on host arrays
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    del calls[:]
    host, _ = _plugin(tmp_path, family, idx, tmp_path / "host", arch_over={"asx_max_batch": 5})
    assert host.separate_many(paths) == want and calls == []
    for names in got:
        assert _blobs(tmp_path / "host", names) == _blobs(tmp_path / "loop", names)
    for inst in (pooled, split, host):
        inst.clear_gpu_cache()


@pytest.mark.parametrize("family,idx", FILE_CASES)
def test_sub_pools_charge_the_pitched_temporaries(tmp_path, monkeypatch, family, idx):
    """Under the free-HBM budget a song costs its pitched chunks plus, in chunks of the pooled chunk buffer, the temporaries of the round
    trip: the pitched mix [2, n'] and the stems at the pitched rate [R, 2, n'].  The runs are those of that cost, and the charge covers what
    ``demix_many_dev`` really allocates beside its results (the torch allocator's peak, each tensor rounded up to its 512-byte block)."""
    import torch
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    inst, _ = _plugin(tmp_path, family, idx, tmp_path / "out")
    dm = inst._demixer()
    lengths = [1000, 877, 700]
    ratio = down_ratio(dm.sample_rate, 2)
    pitched = [pitched_len(n, ratio) for n in lengths]
    rows = int(dm.rof.num_stems) if dm.is_roformer else int(dm.v3.num_targets)          # stems per chunk of the chunk buffer
    net_rows = int(dm.engine.rof_cfg.n_out) if dm.is_roformer else rows                   # rows of a song's demix result
    per_chunk = rows * 2 * dm.chunk_size * 4
    extra = [-(-(net_rows + 1) * n // (rows * dm.chunk_size)) for n in pitched]
    temporaries = [(net_rows + 1) * 2 * n * 4 for n in pitched]
    assert all(x * per_chunk >= t for x, t in zip(extra, temporaries))
    costs = [c + x for c, x in zip(_chunk_counts(dm, pitched), extra)]
    budget = costs[0] + costs[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda device=None: (int(budget * per_chunk / 0.6) + per_chunk // 4 + 1, 1 << 40))
    assert inst._sub_pools(dm, lengths) == _greedy_runs(costs, budget) == [[0, 1], [2]]
    monkeypatch.undo()
    mixes_d = [torch.from_numpy((0.4 * np.random.default_rng(970 + i).standard_normal((2, n))).astype(np.float32)).cuda()
               for i, n in enumerate(lengths)]
    dm.demix_many_dev(mixes_d)                                                            # the engine's own workspaces exist from here on
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = dm.demix_many_dev(mixes_d)
    torch.cuda.synchronize()
    beside_results = torch.cuda.max_memory_allocated() - base - sum(-(-(net_rows + 1) * 2 * n * 4 // 512) * 512 for n in lengths)
    print(family, idx, "temporaries", sum(temporaries), "allocator peak beside the results", beside_results, "charged", sum(extra) * per_chunk)
    assert len(res) == 3 and 0 < beside_results <= sum(extra) * per_chunk + 2 * 512 * len(lengths)
    inst.clear_gpu_cache()


def test_a_roformer_file_whose_pitched_mix_is_short_fails_alone(tmp_path, monkeypatch):
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    inst, wav = _plugin(tmp_path, "roformer", 0, tmp_path / "out")
    ratio = down_ratio(inst._demixer().sample_rate, 2)
    n_short = shortest_with(ratio, 320) - 1                                       # 320 samples or more itself, 319 once pitched
    # decoded on the device, and as a file only the host decoder takes: it too would reach the pooled device call
    shorts = [_cut(tmp_path, wav, n_short), _cut(tmp_path, wav, n_short, "DOUBLE")]
    got = inst.separate_many([wav, shorts[0], shorts[1], _cut(tmp_path, wav, n_short + 1)])
    assert len(got[0]) == 2 and got[1] == got[2] == [] and len(got[3]) == 2 and sorted(inst.batch_errors) == [1, 2]
    for i in (1, 2):
        assert isinstance(inst.batch_errors[i], ValueError) and "pitched mix (319 samples" in str(inst.batch_errors[i])
    inst.clear_gpu_cache()
    # without the device file path the loop of demix refuses them, alone as well
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    host, _ = _plugin(tmp_path, "roformer", 0, tmp_path / "host")
    got = host.separate_many([wav, shorts[0], shorts[1]])
    assert len(got[0]) == 2 and got[1] == got[2] == [] and sorted(host.batch_errors) == [1, 2]
    host.clear_gpu_cache()


@pytest.mark.parametrize("family,idx", [("mdxc", 0), ("roformer", 0)])
def test_a_flac_input_separates_like_the_wav(tmp_path, monkeypatch, plain_engine, family, idx):
    from audio_separator_amd import audio_io
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    by_wav, wav = _plugin(tmp_path, family, idx, tmp_path / "w")
    x, sr = audio_io.read_wav(wav)
    pcm = np.ascontiguousarray(np.rint(x.T.astype(np.float64) * 32768.0), np.int16)
    frames, sizes = plain_engine.flac_encode(pcm, sr, 16, 4096)
    os.makedirs(str(tmp_path / "in"))
    flac = str(tmp_path / "in" / (os.path.splitext(os.path.basename(wav))[0] + ".flac"))
    audio_io.write_flac(flac, frames, sizes, sr, 16, pcm.shape[0])
    names_w = by_wav.separate(wav, None)
    by_wav.clear_gpu_cache()
    by_flac, _ = _plugin(tmp_path, family, idx, tmp_path / "f", asx_profile_file=True)
    names_f = by_flac.separate(flac, None)
    assert "flac_decode" in by_flac.file_timings, by_flac.file_timings            # decoded on the device
    assert names_f == names_w and _blobs(tmp_path / "f", names_f) == _blobs(tmp_path / "w", names_w)
    by_flac.clear_gpu_cache()


@pytest.mark.parametrize("family,idx", FILE_CASES)
def test_stems_dev_keeps_the_stems_on_the_device(tmp_path, monkeypatch, family, idx):
    from audio_separator_amd import audio_io
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    inst, wav = _plugin(tmp_path, family, idx, tmp_path / "out")
    stems = inst.stems_dev(wav)
    assert isinstance(stems, list) and [name for name, _, _ in stems] == [inst.secondary_stem_name, inst.primary_stem_name]
    n = audio_io.wav_info(wav)["frames"]
    assert all(t.is_cuda and tuple(t.shape) == (2, n) and layout == "planar" for _, t, layout in stems)
    inst.clear_file_specific_paths()
    many, states = inst.stems_dev_many([wav, wav])
    assert all(isinstance(s, list) and len(s) == 2 for s in many) and None not in states
    for (_, a, _), (_, b, _) in zip(many[0], stems):
        assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    inst.clear_gpu_cache()


def test_ensemble_of_two_pitched_members_takes_the_device_path(A, tmp_path, monkeypatch):
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    # the same net at two overlaps, the second under a name of its own: the intermediate files carry the model's name
    first, wav = _plugin(tmp_path, "mdxc", 0, tmp_path / "m")
    second, _ = _plugin(tmp_path, "mdxc", 0, tmp_path / "m", arch_over={"overlap": 2}, model_name="mdxc_v3two_ov2")
    members = [first, second]
    assert all(m.pitch_shift == 2 for m in members)
    by_files = A.EnsembleSeparator(members, "avg_wave", None, via_files=True)
    by_files.output_dir = str(tmp_path / "files")
    want = by_files.separate(wav, None)
    assert by_files.last_path_taken == "files" and len(want) == 2
    on_device = A.EnsembleSeparator(members, "avg_wave", None)
    on_device.output_dir = str(tmp_path / "device")
    got = on_device.separate(wav, None)
    assert on_device.last_path_taken == "device"
    assert [os.path.basename(f) for f in got] == [os.path.basename(f) for f in want]
    for a, b in zip(got, want):
        assert os.path.isfile(a) and filecmp.cmp(a, b, shallow=False), os.path.basename(a)
    many = A.EnsembleSeparator(members, "avg_wave", None)
    many.output_dir = str(tmp_path / "many")
    got_many = many.separate_many([wav])
    assert many.last_paths_taken == ["device"]
    for a, b in zip(got_many[0], want):
        assert filecmp.cmp(a, b, shallow=False), os.path.basename(a)
    for m in members:
        m.clear_gpu_cache()
