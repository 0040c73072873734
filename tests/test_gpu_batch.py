"""A batch of songs in one engine call (asx_demix_batch_dev / asx_separate_batch_dev): the chunks of all songs are pooled per
launch, each song's result must equal the single-song path's BIT FOR BIT -- np.array_equal / filecmp everywhere, no tolerance.
The single-song path is the yardstick: it is pinned to the reference by tests/test_gpu_parity.py and tests/test_gpu_fullsong.py,
and tests/test_gpu_sharding.py already demands that results do not depend on how the chunk list is cut into batches."""
import filecmp
import os

import numpy as np
import pytest

from oracle import mdx_oracle as O
from tests import separate_cases as SC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


def _engine(A, geometry, max_batch=3, **cfg):
    """fast: n_fft 6144 / hop 1024 (the three-pass FFT kernels) with a short segment and a narrow net; generic: n_fft 2048"""
    if geometry == "fast":
        mc = A.MDXConfig(segment_size=40, dim_f=3072, max_batch=max_batch, **cfg)
        d = O.NetDims(dim_c=4, dim_f=3072, dim_t=40, g=8, l=1, num_blocks=3, k=3, bn=8)
    else:
        mc = A.MDXConfig(n_fft=2048, hop_length=512, dim_f=256, segment_size=16, max_batch=max_batch, **cfg)
        d = O.NetDims(dim_c=4, dim_f=256, dim_t=16, g=8, l=2, num_blocks=5, k=3, bn=4)
    eng = A.Engine(mc)
    eng.load_net(A.NetConfig(dim_f=d.dim_f, dim_t=d.dim_t, g=d.g, l=d.l, num_blocks=d.num_blocks, bn=d.bn),
                 A.fold_convtdf_state(O.make_convtdf_state(d, seed=5), d.num_blocks, d.l))
    return eng


def _pool_lengths(eng):
    """>= 7 songs: N = 1, N < gen_size, an exact multiple of gen_size (maximal pad), N % 4 != 0 beside N % 4 == 0 (both fold
    paths), two of equal N, one of at least 3 x max_batch chunks"""
    p = eng.plan(1000)
    gen, step = p["gen_size"], p["step"]
    lens = [1, gen // 2 + 1, 2 * gen, gen + 6, gen + 8, 2 * gen, 10 * step]
    assert eng.plan(lens[-1])["n_chunks"] >= 3 * eng.cfg.max_batch
    assert lens[3] % 4 != 0 and lens[4] % 4 == 0 and lens[2] % gen == 0
    return lens


def _mixes(lens, seed=0):
    rng = np.random.default_rng(seed)
    return [(0.4 * rng.standard_normal((2, n))).astype(np.float32) for n in lens]


def _check_pool(eng, mixes, match=False):
    want = [eng.demix(m, is_match_mix=match) for m in mixes]
    got = eng.demix_batch(mixes, is_match_mix=match)
    assert len(got) == len(mixes)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (i, mixes[i].shape, int(np.sum(g != w)))
    back = eng.demix_batch(mixes[::-1], is_match_mix=match)[::-1]       # a song's result does not depend on its position
    for i, (g, w) in enumerate(zip(back, want)):
        assert np.array_equal(g, w), ("reversed", i, int(np.sum(g != w)))
    assert all(np.isfinite(w).all() for w in want) and any(np.abs(w).max() > 0 for w in want)


@pytest.mark.parametrize("geometry", ["fast", "generic"])
def test_pool_equals_singles(A, geometry):
    eng = _engine(A, geometry)
    _check_pool(eng, _mixes(_pool_lengths(eng), seed=1))
    eng.close()


@pytest.mark.parametrize("geometry", ["fast", "generic"])
@pytest.mark.parametrize("mode", ["denoise", "match_mix", "overlap0"])
def test_pool_modes(A, geometry, mode):
    cfg = {"denoise": dict(enable_denoise=True), "match_mix": {}, "overlap0": dict(overlap=0.0)}[mode]
    eng = _engine(A, geometry, **cfg)
    _check_pool(eng, _mixes(_pool_lengths(eng), seed=2), match=(mode == "match_mix"))
    eng.close()


def test_stem_algebra(A):
    """separate_batch against separate per song: peaks above and below max_peak (scaled / untouched), the caller's arrays
    normalised in place"""
    eng = _engine(A, "generic")
    lens = _pool_lengths(eng)[1:]
    base = _mixes(lens, seed=3)
    scale = [2.5, 0.2, 1.7, 0.05, 3.0, 0.4]
    mixes = [np.ascontiguousarray(m * (s / np.abs(m).max())) for m, s in zip(base, scale)]
    max_peak, min_peak, comp = 0.9, 0.3, 1.035
    assert any(np.abs(m).max() > max_peak for m in mixes) and any(min_peak < np.abs(m).max() < max_peak for m in mixes)
    singles, normed = [], []
    for m in mixes:
        c = m.copy()
        singles.append(eng.separate(c, max_peak, min_peak, comp))
        normed.append(c)
    pooled_in = [m.copy() for m in mixes]
    pooled = eng.separate_batch(pooled_in, max_peak, min_peak, comp)
    for i in range(len(mixes)):
        assert np.array_equal(pooled_in[i], normed[i]), i                 # in-place normalisation of the caller's array
        assert np.array_equal(pooled[i][0], singles[i][0]) and np.array_equal(pooled[i][1], singles[i][1]), i
    assert not np.array_equal(normed[0], mixes[0]) and np.array_equal(normed[5], mixes[5])   # one scaled, one left alone
    none_min = eng.separate_batch([m.copy() for m in mixes[:2]], max_peak, None, comp)
    for i in range(2):
        p, s = eng.separate(mixes[i].copy(), max_peak, None, comp)
        assert np.array_equal(none_min[i][0], p) and np.array_equal(none_min[i][1], s)
    eng.close()


def test_launch_count_depends_on_chunks_only(A):
    """8 songs x 2 chunks against 1 song x 16 chunks: the same number of STFT, net-class and iSTFT launches"""
    import torch
    eng = _engine(A, "fast", max_batch=5)
    p = eng.plan(1000)
    n2 = p["step"] + 10
    n16 = 15 * p["step"] + 10
    assert eng.plan(n2)["n_chunks"] == 2 and eng.plan(n16)["n_chunks"] == 16
    small = [torch.from_numpy(m).cuda() for m in _mixes([n2] * 8, seed=4)]
    big = torch.from_numpy(_mixes([n16], seed=5)[0]).cuda()

    def classes(run):
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
    outs = [torch.empty_like(m) for m in small]
    pool = classes(lambda: eng.demix_batch_dev([(m.data_ptr(), o.data_ptr(), n2) for m, o in zip(small, outs)]))
    out = torch.empty_like(big)
    one = classes(lambda: eng.demix_dev(big.data_ptr(), n16, out.data_ptr()))
    per_song = ("misc", "finalize")                                 # fold, divider build: O(1) per song is allowed
    keys = sorted(k for k in set(pool) | set(one) if k not in per_song)
    assert "stft" in keys and "istft" in keys and len(keys) >= 4, keys
    assert {k: pool.get(k, 0) for k in keys} == {k: one.get(k, 0) for k in keys}
    assert pool["finalize"] == 1                                    # one segmented fold for the pool
    eng.close()


def test_batch_call_is_capturable_into_a_hip_graph(A):
    """Once the workspace has its size the batch call only enqueues work (tables come from launch arguments, no host copy, no
    synchronisation): captured into a hipGraph and replayed it gives the directly launched result, also for new contents"""
    import torch
    for geometry, match in (("generic", False), ("fast", True)):
        eng = _engine(A, geometry)
        lens = _pool_lengths(eng)[1:5]
        mixes = [torch.from_numpy(m).cuda() for m in _mixes(lens, seed=7)]
        direct = [torch.empty_like(m) for m in mixes]
        replayed = [torch.zeros_like(m) for m in mixes]
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            eng.demix_batch_dev([(m.data_ptr(), o.data_ptr(), n) for m, o, n in zip(mixes, direct, lens)], match, side.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.demix_batch_dev([(m.data_ptr(), o.data_ptr(), n) for m, o, n in zip(mixes, replayed, lens)], match,
                                torch.cuda.current_stream().cuda_stream)
        assert all(float(o.abs().sum()) == 0.0 for o in replayed)          # nothing ran during capture
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(direct, replayed))
        for m in mixes:
            m.mul_(0.5)
        graph.replay()
        torch.cuda.synchronize()
        for m, o, n in zip(mixes, replayed, lens):
            again = torch.empty_like(m)
            eng.demix_dev(m.data_ptr(), n, again.data_ptr(), is_match_mix=match, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert torch.equal(again, o)
        eng.close()


def test_arguments(A):
    """A null pointer or n_samples < 1 in any slot raises and leaves every output untouched; an empty pool returns at once"""
    import torch
    eng = _engine(A, "generic")
    lens = [700, 1200, 900]
    mixes = [torch.from_numpy(m).cuda() for m in _mixes(lens, seed=6)]
    outs = [torch.full((2, n), -7.0, dtype=torch.float32, device="cuda") for n in lens]
    good = [(m.data_ptr(), o.data_ptr(), n) for m, o, n in zip(mixes, outs, lens)]
    for slot in range(3):
        for bad in ((0, good[slot][1], good[slot][2]), (good[slot][0], 0, good[slot][2]), (good[slot][0], good[slot][1], 0),
                    (good[slot][0], good[slot][1], -5)):
            songs = list(good)
            songs[slot] = bad
            with pytest.raises(A.AsxError):
                eng.demix_batch_dev(songs)
            torch.cuda.synchronize()
            assert all(bool((o == -7.0).all()) for o in outs), (slot, bad)
    prim = [torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda") for n in lens]
    sec = [torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda") for n in lens]
    before = [m.clone() for m in mixes]
    sg = [(m.data_ptr(), p.data_ptr(), s.data_ptr(), n) for m, p, s, n in zip(mixes, prim, sec, lens)]
    for slot in range(3):
        for col in range(4):
            songs = list(sg)
            songs[slot] = tuple(0 if c == col else v for c, v in enumerate(sg[slot]))
            with pytest.raises(A.AsxError):
                eng.separate_batch_dev(songs, 0.9, None, 1.0)
            torch.cuda.synchronize()
            assert all(bool((t == -7.0).all()) for t in prim + sec), (slot, col)
            assert all(torch.equal(m, b) for m, b in zip(mixes, before)), (slot, col)     # not even the in-place normalise ran
    eng.demix_batch_dev([])
    eng.separate_batch_dev([], 0.9, None, 1.0)
    assert eng.demix_batch([]) == [] and eng.separate_batch([], 0.9, None, 1.0) == []
    with pytest.raises(ValueError):
        eng.demix_batch([np.zeros((3, 100), np.float32)])
    with pytest.raises(ValueError):
        eng.separate_batch([np.zeros((2, 100), np.float64)], 0.9, None, 1.0)
    eng.demix_batch_dev(good)                                       # the engine is still usable
    torch.cuda.synchronize()
    assert all(bool((o != -7.0).any()) for o in outs)
    eng.close()


def test_separate_many_files(tmp_path):
    """MDXSeparator.separate_many on three WAVs of different length (one PCM_24) against separate() per file into another
    directory: the same names, the same bytes; a silent file fails alone"""
    from audio_separator_amd import audio_io
    tag, cls, common, arch, wav, _ = SC.cases("mdx", str(tmp_path))[0]
    x, sr = audio_io.read_wav(wav)
    srcs = []
    for i, (n, subtype) in enumerate([(x.shape[1], "PCM_16"), (x.shape[1] * 2 // 3 + 1, "PCM_24"), (x.shape[1] // 3, "PCM_16")]):
        path = str(tmp_path / f"song{i}.wav")
        audio_io.write_wav(path, np.ascontiguousarray(x[:, :n].T), sr, subtype)
        srcs.append(path)
    silent = str(tmp_path / "silent.wav")
    audio_io.write_wav(silent, np.zeros((4000, 2), np.int16), sr, "PCM_16")
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=one_dir), arch_config=arch)
    want = []
    for path in srcs:
        want.append(inst.separate(path, None))
        inst.clear_gpu_cache()
        inst.clear_file_specific_paths()
    inst = SC.plugin_class(cls)(common_config=dict(common, output_dir=many_dir), arch_config=arch)
    got = inst.separate_many(srcs[:2] + [silent] + srcs[2:])
    assert got[2] == [] and isinstance(inst.batch_errors[2], ValueError) and "empty or not valid" in str(inst.batch_errors[2])
    got = got[:2] + got[3:]
    assert got == want and all(len(names) == 2 for names in got)
    for names in want:
        for name in names:
            assert filecmp.cmp(os.path.join(one_dir, name), os.path.join(many_dir, name), shallow=False), name
    assert audio_io.info(os.path.join(many_dir, want[1][0]))["subtype"] == "PCM_24"


@pytest.mark.parametrize("family", ["mdx", "demucs"])
def test_separate_many_mixed_decode(family, tmp_path, monkeypatch):
    """One batch in which the first and the last file are decoded on the device and the middle one (PCM_24) on the host, so both
    branches of the plugin's emit step run between the same pooled call and the same per-file state: the same names and the same
    bytes as separate() per file under the same decoders (and, for Demucs, the same seed)."""
    import random
    from audio_separator_amd import audio_io
    tag, cls, common, arch, wav, _ = SC.cases(family, str(tmp_path))[0]
    x, sr = audio_io.read_wav(wav)
    assert sr == common["sample_rate"] and x.shape[0] == 2
    srcs = []
    for i, (n, subtype) in enumerate([(x.shape[1], "PCM_16"), (x.shape[1] * 2 // 3 + 1, "PCM_24"), (x.shape[1] // 3, "PCM_16")]):
        path = str(tmp_path / f"song{i}.wav")
        audio_io.write_wav(path, np.ascontiguousarray(x[:, :n].T), sr, subtype)
        srcs.append(path)
    klass = SC.plugin_class(cls)
    real, decoded = klass._device_mix, []

    def device_mix(self, path, check_silent=True):
        mix = None if path == srcs[1] else real(self, path, check_silent)
        decoded.append((path, mix is not None))
        return mix
    monkeypatch.setattr(klass, "_device_mix", device_mix)
    mixed = [(srcs[0], True), (srcs[1], False), (srcs[2], True)]
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    inst = klass(common_config=dict(common, output_dir=one_dir), arch_config=arch)
    random.seed(5)
    want = []
    for path in srcs:
        want.append(inst.separate(path, None))
        inst.clear_gpu_cache()
        inst.clear_file_specific_paths()
    assert decoded == mixed                                          # one decode attempt per file, the middle one refused
    del decoded[:]
    inst = klass(common_config=dict(common, output_dir=many_dir), arch_config=arch)
    random.seed(5)
    got = inst.separate_many(srcs)
    assert decoded == mixed and inst.batch_errors == {}
    assert got == want and all(len(names) == (4 if family == "demucs" else 2) for names in got)
    for names in want:
        for name in names:
            assert filecmp.cmp(os.path.join(one_dir, name), os.path.join(many_dir, name), shallow=False), name
    assert audio_io.info(os.path.join(many_dir, want[1][0]))["subtype"] == "PCM_24"
    assert audio_io.info(os.path.join(many_dir, want[2][0]))["subtype"] == "PCM_16"


def test_config5_rank_share_on_one_gpu(A):
    """BASELINE config 5's per-rank workload on the HIP engine: 8 distinct seeded songs at the HQ_3 geometry and weights
    through FilesPipeline(world=1, demix_many=...); every stem bit-identical to the single-song demix_dev result."""
    import torch
    from audio_separator_amd.sharding import FilesPipeline, batch_demix_many
    d = O.NetDims()
    eng = A.Engine(A.MDXConfig())
    eng.load_net(A.NetConfig(), A.fold_convtdf_state(O.make_convtdf_state(d, seed=0), d.num_blocks, d.l))
    n = 44100 * 30
    mixes = [torch.from_numpy(O.synth_mix(n, seed=s)).cuda() for s in range(8)]
    want = []
    for m in mixes:
        o = torch.empty_like(m)
        eng.demix_dev(m.data_ptr(), n, o.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
        want.append(o)

    def never(mix, out):
        raise AssertionError("the per-song loop ran")
    pipe = FilesPipeline(never, mixes, 1, 0, False, demix_many=batch_demix_many(eng))
    pipe.step(0)
    pipe.step(1)
    pipe.drain()
    torch.cuda.synchronize()
    for b in (0, 1):
        for s in range(8):
            assert torch.equal(pipe.outs[b][s], want[s]), (b, s)
    assert bool(torch.isfinite(pipe.outs[0]).all()) and float(pipe.outs[0].abs().max()) > 0
    eng.close()
