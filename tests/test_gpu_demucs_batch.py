"""A batch of songs through the Demucs path in one call (asx_ht_demix_batch_dev / asx_hd_demix_batch_dev): the segments of all
songs share the forwards, every song keeps its own standardisation statistics, one segmented fold per shift writes all outputs.
The claim is bit identity with the single-song call, so every comparison is np.array_equal / torch.equal / filecmp."""
import filecmp
import os
import random

import numpy as np
import pytest

from oracle import demucs_oracle as D
from oracle import hdemucs_oracle as H
from tests.test_gpu_demucs import hcfg as ht_hcfg, ocfg_a
from tests.test_gpu_hdemucs import hcfg as hd_hcfg, ocfg as hd_ocfg

pytestmark = pytest.mark.gpu
SR = 8000                          # both small nets; max_shift = 4000
MAXB = {"ht": 3, "hd": 2}


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


def _engine(A, gen, max_batch, seed=None):
    eng = A.Engine(A.MDXConfig(n_fft=1024, hop_length=256, dim_f=512, segment_size=8), device=0)
    if gen == "ht":
        oc = ocfg_a()                                             # segment 8000 samples
        eng.load_ht(ht_hcfg(A, oc, max_batch), D.make_ht_state(oc, seed or 11))
    else:
        oc = hd_ocfg()                                            # segment 16000 samples
        eng.load_hd(hd_hcfg(A, oc, max_batch), H.make_hd_state(oc, seed or 21))
    return eng


def _mixes(lengths, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((2, n)) * (0.1 + 0.05 * i) + 0.01 * i).astype(np.float32) for i, n in enumerate(lengths)]


def _offsets(i, shifts):
    return [(i * 997 + 13 + 1741 * k) % (SR // 2 + 1) for k in range(shifts)] if shifts else None


def _pool_lengths(eng, gen):
    """one song shorter than a segment, two of equal N, one with >= 3 * max_batch segments, ragged tails"""
    plan = eng.ht_plan if gen == "ht" else eng.hd_plan
    seg = plan(1000)["chunk_size"]
    stride = int(0.75 * seg)
    long_n = (3 * MAXB[gen]) * stride - stride // 2 + 11
    lens = [seg // 3 + 1, 2 * stride + 923, 2 * stride + 923, long_n, stride + 1777]
    assert lens[0] < seg and plan(lens[0])["n_chunks"] == 1
    assert plan(long_n)["n_chunks"] >= 3 * MAXB[gen]
    assert all(0 < (n - 1) % stride + 1 < seg for n in lens[1:])                 # the last chunk of every longer song is a ragged tail
    return lens


@pytest.mark.parametrize("flags", [0, 3])
@pytest.mark.parametrize("shifts", [0, 2])
@pytest.mark.parametrize("gen", ["ht", "hd"])
def test_pool_equals_singles(A, gen, shifts, flags):
    import torch
    eng = _engine(A, gen, MAXB[gen])
    single = eng.ht_demix_dev if gen == "ht" else eng.hd_demix_dev
    batch = eng.ht_demix_batch_dev if gen == "ht" else eng.hd_demix_batch_dev
    lens = _pool_lengths(eng, gen)
    mixes = [torch.from_numpy(m).cuda() for m in _mixes(lens, seed=4)]
    offs = [_offsets(i, shifts) for i in range(len(lens))]
    want = []
    for m, n, o in zip(mixes, lens, offs):
        out = torch.empty((4, 2, n), dtype=torch.float32, device="cuda")
        single(m.data_ptr(), n, out.data_ptr(), shifts=shifts, offsets=o, overlap=0.25, flags=flags)
        torch.cuda.synchronize()
        want.append(out)
    for order in (list(range(len(lens))), list(reversed(range(len(lens))))):
        outs = [torch.full((4, 2, n), float("nan"), dtype=torch.float32, device="cuda") for n in lens]
        batch([(mixes[i].data_ptr(), outs[i].data_ptr(), lens[i], offs[i]) for i in order], shifts=shifts, overlap=0.25, flags=flags)
        torch.cuda.synchronize()
        for i in range(len(lens)):
            assert torch.equal(outs[i], want[i]), (gen, shifts, flags, order, i)
    # the host-array convenience returns the same arrays
    run = eng.ht_demix_batch if gen == "ht" else eng.hd_demix_batch
    got = run([m.cpu().numpy() for m in mixes[:3]], shifts=shifts, offsets=offs[:3] if shifts else None, overlap=0.25,
              standardize=bool(flags & 1), swap01=bool(flags & 2))
    for i in range(3):
        assert np.array_equal(got[i], want[i].cpu().numpy())
    eng.close()


@pytest.mark.parametrize("gen", ["ht", "hd"])
def test_more_songs_than_one_fold_launch_holds(A, gen):
    """35 short songs of different lengths, shifts 2, flags 3: the fold's arguments travel by value, 32 songs per launch, so songs
    33 .. 35 take a second launch per shift index (its own block numbering, the global statistics slots and slab rows).  Every song
    equals its single-song call in both pool orders; the fold launches are shifts x ceil(35 / 32) = 4."""
    import torch
    eng = _engine(A, gen, MAXB[gen])
    single = eng.ht_demix_dev if gen == "ht" else eng.hd_demix_dev
    batch = eng.ht_demix_batch_dev if gen == "ht" else eng.hd_demix_batch_dev
    lens = [1500 + 137 * i for i in range(35)]
    mixes = [torch.from_numpy(m).cuda() for m in _mixes(lens, seed=14)]
    offs = [_offsets(i, 2) for i in range(35)]
    want = []
    for m, n, o in zip(mixes, lens, offs):
        out = torch.empty((4, 2, n), dtype=torch.float32, device="cuda")
        single(m.data_ptr(), n, out.data_ptr(), shifts=2, offsets=o, overlap=0.25, flags=3)
        torch.cuda.synchronize()
        want.append(out)
    for order in (list(range(35)), list(reversed(range(35)))):
        outs = [torch.full((4, 2, n), float("nan"), dtype=torch.float32, device="cuda") for n in lens]
        batch([(mixes[i].data_ptr(), outs[i].data_ptr(), lens[i], offs[i]) for i in order], shifts=2, overlap=0.25, flags=3)
        torch.cuda.synchronize()
        for i in range(35):
            assert torch.equal(outs[i], want[i]), (gen, order[0], i)
    outs = [torch.empty((4, 2, n), device="cuda") for n in lens]
    count = _classes(eng, lambda: batch([(m.data_ptr(), o.data_ptr(), n, f) for m, o, n, f in zip(mixes, outs, lens, offs)], shifts=2, flags=3))
    assert count["finalize"] == 4
    eng.close()


def _bag(A, **arch):
    oc = ocfg_a()
    models = [(ht_hcfg(A, oc, 3), D.make_ht_state(oc, 11)), (ht_hcfg(A, oc, 3), D.make_ht_state(oc, 21))]
    return A.DemucsDemixer({"torch_device": 0}, arch, models=models, weights=[[1.0, 0.5, 2.0, 1.0], [0.5, 1.5, 1.0, 1.0]])


def test_bag_many_equals_per_song(A):
    dm = _bag(A, shifts=2, overlap=0.25)
    mixes = _mixes([5000, 20923, 20923, 13001], seed=8)
    offs = [[_offsets(2 * s, 2), _offsets(2 * s + 1, 2)] for s in range(len(mixes))]          # per song: one list per member
    many = dm.demix_many(mixes, offsets=offs)
    for s, m in enumerate(mixes):
        assert np.array_equal(many[s], dm.demix(m, offsets=offs[s])), s
    dm.close()


@pytest.mark.parametrize("gen", ["ht", "hd"])
def test_seeded_draws(A, gen):
    if gen == "ht":
        oc = ocfg_a()
        models = [(ht_hcfg(A, oc, 3), D.make_ht_state(oc, 11))]
    else:
        oc = hd_ocfg()
        models = [(hd_hcfg(A, oc, 2), H.make_hd_state(oc, 21))]
    dm = A.DemucsDemixer({"torch_device": 0}, {"shifts": 2, "overlap": 0.25}, models=models)
    mixes = _mixes([9000, 30011, 4000], seed=9)
    random.seed(5)
    many = dm.demix_many(mixes)
    random.seed(5)
    loop = [dm.demix(m) for m in mixes]
    assert all(np.array_equal(a, b) for a, b in zip(many, loop))
    dm.close()


def _classes(eng, run):
    import torch
    run()                                                       # workspace sized, weight images built
    torch.cuda.synchronize()
    eng.profile_enable(True)
    run()
    torch.cuda.synchronize()
    recs = eng.profile_launches()
    eng.profile_enable(False)
    count = {}
    for r in recs:
        count[r[0]] = count.get(r[0], 0) + 1
    return count


def test_v4_launch_count_depends_on_segments_only(A):
    """8 songs x 2 segments against 1 song x 16 segments (shifts = 2: one against eight per shift): the same launches in every
    class of the forwards; one fold per shift index, not per song and shift; the per-song extra is one statistics launch each."""
    import torch
    eng = _engine(A, "ht", 5)
    n2, n16, offs = 1900, 42000, [0, 0]
    assert eng.ht_plan(n2, 2, offs)["n_chunks"] == 2 and eng.ht_plan(n16, 2, offs)["n_chunks"] == 16
    small = [torch.from_numpy(m).cuda() for m in _mixes([n2] * 8, seed=4)]
    big = torch.from_numpy(_mixes([n16], seed=5)[0]).cuda()
    outs = [torch.empty((4, 2, n2), device="cuda") for _ in small]
    out = torch.empty((4, 2, n16), device="cuda")
    for flags in (0, 3):
        pool = _classes(eng, lambda: eng.ht_demix_batch_dev([(m.data_ptr(), o.data_ptr(), n2, offs) for m, o in zip(small, outs)],
                                                            shifts=2, flags=flags))
        one = _classes(eng, lambda: eng.ht_demix_batch_dev([(big.data_ptr(), out.data_ptr(), n16, offs)], shifts=2, flags=flags))
        keys = sorted(k for k in set(pool) | set(one) if k != "misc")
        assert "stft" in keys and "istft" in keys and "finalize" in keys and len(keys) >= 4, keys
        assert {k: pool.get(k, 0) for k in keys} == {k: one.get(k, 0) for k in keys}
        assert pool["finalize"] == 2                              # shifts, not songs x shifts
        assert pool["misc"] - one["misc"] == (7 if flags & 1 else 0)     # the statistics reduction of songs 2 .. 8
    eng.close()


def _hd_rounds(lengths, max_batch, segment, budget, max_groups=6):
    """The rounds of hd_forward_groups for chunks of these lengths, restated from the engine's rule: sort descending, equal lengths
    form groups of up to max_batch, up to max_groups (HD_MAX_GROUPS, knobs.h) groups advance in one round, and (pool only) the
    groups of a round hold at most `budget` samples together."""
    order = sorted(lengths, reverse=True)
    groups, i = [], 0
    while i < len(order):
        j = i
        while j < len(order) and order[j] == order[i] and j - i < max_batch:
            j += 1
        groups.append((j - i) * order[i])
        i = j
    rounds, held, n = 0, 0, 0
    for g in groups:
        if n == 0 or n == max_groups or (budget and held + g > budget):
            rounds, held, n = rounds + 1, 0, 0
        held, n = held + g, n + 1
    return len(groups), rounds


def test_v3_equal_songs_fill_groups_across_songs(A):
    """4 songs of equal length, max_batch = 2, 3 chunks each (two full, one tail).  The pool forms the groups that ONE song with
    these 12 chunks would form, ceil(8 / 2) + ceil(4 / 2) = 6, where four single calls form 4 x 2 = 8 (a group launches its STFT and
    its iSTFT once, so those classes count the groups).  Rounds of hd_forward_groups (the engine's "hd_rounds" counter): the six
    groups advance in 3 rounds -- a round of the pool holds at most 2 x max_batch segments' worth of samples, which two full groups
    reach -- against one round per song, 4, for the loop."""
    import torch
    eng = _engine(A, "hd", 2)
    seg, n = 16000, 16000 + 12000 + 100
    assert eng.hd_plan(n)["n_chunks"] == 3
    chunks = [16000, 16000, 4100]
    assert _hd_rounds(chunks * 4, 2, seg, 2 * 2 * seg) == (6, 3) and _hd_rounds(chunks, 2, seg, 0) == (2, 1)
    mixes = [torch.from_numpy(m).cuda() for m in _mixes([n] * 4, seed=6)]
    outs = [torch.empty((4, 2, n), device="cuda") for _ in mixes]

    def rounds(run):
        r0 = eng.counter("hd_rounds")
        count = _classes(eng, run)
        return count, (eng.counter("hd_rounds") - r0) // 2          # _classes runs twice
    pool, pool_rounds = rounds(lambda: eng.hd_demix_batch_dev([(m.data_ptr(), o.data_ptr(), n, None) for m, o in zip(mixes, outs)]))
    one, one_rounds = rounds(lambda: eng.hd_demix_dev(mixes[0].data_ptr(), n, outs[0].data_ptr()))
    assert one["stft"] == one["istft"] == 2 and one_rounds == 1
    assert pool["stft"] == pool["istft"] == 6
    assert pool_rounds == 3 < 4 * one_rounds
    assert pool["finalize"] == 1
    eng.close()


def test_pooled_call_is_capturable_into_a_hip_graph(A):
    """After one warm call the v4 pooled call only enqueues work on its stream: captured on one side stream and replayed it gives the
    direct result, also for new contents"""
    import torch
    eng = _engine(A, "ht", 3)
    lens = [3001, 20923, 13001]
    offs = [_offsets(i, 2) for i in range(3)]
    mixes = [torch.from_numpy(m).cuda() for m in _mixes(lens, seed=7)]
    direct = [torch.empty((4, 2, n), device="cuda") for n in lens]
    replayed = [torch.zeros((4, 2, n), device="cuda") for n in lens]
    songs = lambda outs: [(m.data_ptr(), o.data_ptr(), n, f) for m, o, n, f in zip(mixes, outs, lens, offs)]  # noqa: E731
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        eng.ht_demix_batch_dev(songs(direct), shifts=2, flags=3, stream=side.cuda_stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        eng.ht_demix_batch_dev(songs(replayed), shifts=2, flags=3, stream=torch.cuda.current_stream().cuda_stream)
    assert all(float(o.abs().sum()) == 0.0 for o in replayed)          # nothing ran during capture
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(direct, replayed))
    for m in mixes:
        m.mul_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    for m, o, n, f in zip(mixes, replayed, lens, offs):
        again = torch.empty_like(o)
        eng.ht_demix_dev(m.data_ptr(), n, again.data_ptr(), shifts=2, offsets=f, flags=3)
        torch.cuda.synchronize()
        assert torch.equal(again, o)
    eng.close()


@pytest.mark.parametrize("gen", ["ht", "hd"])
def test_arguments(A, gen):
    """A null pointer, n_samples < 1 (and 1, which the single-song calls refuse too), a bad offset or a missing offsets list (shifts > 0) in any slot raises and leaves every output
    untouched; an empty pool returns at once"""
    import torch
    eng = _engine(A, gen, 2)
    batch = eng.ht_demix_batch_dev if gen == "ht" else eng.hd_demix_batch_dev
    lens = [700, 1200, 900]
    mixes = [torch.from_numpy(m).cuda() for m in _mixes(lens, seed=6)]
    outs = [torch.full((4, 2, n), -7.0, dtype=torch.float32, device="cuda") for n in lens]
    good = [(m.data_ptr(), o.data_ptr(), n, [5, 4000]) for m, o, n in zip(mixes, outs, lens)]
    for slot in range(3):
        m, o, n, f = good[slot]
        for bad in ((0, o, n, f), (m, 0, n, f), (m, o, 0, f), (m, o, -5, f), (m, o, 1, f), (m, o, n, [5, 4001]), (m, o, n, [-1, 5]), (m, o, n, None)):
            songs = list(good)
            songs[slot] = bad
            with pytest.raises(A.AsxError):
                batch(songs, shifts=2, flags=3)
            torch.cuda.synchronize()
            assert all(bool((t == -7.0).all()) for t in outs), (slot, bad)
        with pytest.raises(ValueError):                              # one offset per shift
            batch(good[:slot] + [(m, o, n, [5])] + good[slot + 1:], shifts=2)
    for overlap in (1.0, -0.1):
        with pytest.raises(A.AsxError):
            batch(good, shifts=2, overlap=overlap)
    assert all(bool((t == -7.0).all()) for t in outs)
    batch([], shifts=2)
    assert (eng.ht_demix_batch if gen == "ht" else eng.hd_demix_batch)([], shifts=0) == []
    batch(good, shifts=2, flags=3)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) and not bool((t == -7.0).any()) for t in outs)
    eng.close()


def test_separate_many_files_equal_separate(A, tmp_path):
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.demucs_separator import DemucsSeparator
    from tests import separate_cases as SC
    repo = SC.write_demucs_repo(str(tmp_path / "demucs_repo"))
    wavs = []
    for i, n in enumerate((21000, 9500, 30011)):
        p = str(tmp_path / f"song{i}.wav")
        audio_io.write_wav(p, np.clip(_mixes([n], seed=30 + i)[0].T * 2.0, -0.99, 0.99), SR, "PCM_16" if i != 1 else "PCM_24")
        wavs.append(p)
    bad = str(tmp_path / "broken.wav")
    with open(bad, "w") as f:
        f.write("not audio")
    for yml, arch in (("htd_single", {"shifts": 2, "overlap": 0.25, "segments_enabled": True}),
                      ("htd_bag", {"shifts": 1, "overlap": 0.5, "segments_enabled": True})):
        def make(out_dir):
            common = SC.common_config(yml, os.path.join(repo, yml + ".yaml"), {}, out_dir, sample_rate=SR)
            return DemucsSeparator(common_config=common, arch_config=dict(arch, segment_size="Default"))
        one_dir, many_dir = str(tmp_path / f"{yml}_one"), str(tmp_path / f"{yml}_many")
        sep = make(one_dir)
        random.seed(3)
        want = [sep.separate(p) for p in wavs]
        sep.clear_gpu_cache()
        sep = make(many_dir)
        random.seed(3)
        got = sep.separate_many([wavs[0], bad, wavs[1], wavs[2]])
        assert got[1] == [] and list(sep.batch_errors) == [1] and isinstance(sep.batch_errors[1], Exception)
        assert [got[0], got[2], got[3]] == want and all(len(names) == 4 for names in want)
        for names in want:
            for name in names:
                assert filecmp.cmp(os.path.join(one_dir, name), os.path.join(many_dir, name), shallow=False), (yml, name)


def test_config5_rank_share_on_one_gpu(A):
    """BASELINE config 5's per-rank workload on the Demucs path: 8 songs through FilesPipeline(world=1, demix_many=...); every stem
    equals the single-song demix_dev result."""
    import torch
    from audio_separator_amd.sharding import FilesPipeline, demucs_demix_many
    eng = _engine(A, "ht", 0)
    n = 20923
    mixes = [torch.from_numpy(m).cuda() for m in _mixes([n] * 8, seed=12)]
    offs = [_offsets(i, 2) for i in range(8)]
    want = []
    for m, f in zip(mixes, offs):
        o = torch.empty((4, 2, n), device="cuda")
        eng.ht_demix_dev(m.data_ptr(), n, o.data_ptr(), shifts=2, offsets=f, flags=3, stream=torch.cuda.current_stream().cuda_stream)
        want.append(o)

    def never(mix, out):
        raise AssertionError("the per-song loop ran")
    pipe = FilesPipeline(never, mixes, 1, 0, False, demix_many=demucs_demix_many(eng, "ht", shifts=2, offsets=offs), stem_shape=(4, 2, n))
    pipe.step(0)
    pipe.step(1)
    pipe.drain()
    torch.cuda.synchronize()
    for b in (0, 1):
        assert tuple(pipe.outs[b].shape) == (8, 4, 2, n)
        for s in range(8):
            assert torch.equal(pipe.outs[b][s], want[s]), (b, s)
    eng.close()
