"""asx_mdxc_demix_batch_dev / asx_rof_demix_batch_dev: a pool of songs whose chunks share the net passes, on the toy nets of
test_gpu_mdxc.py and test_gpu_roformer.py.

Both nets give the same floats whatever the number of chunks in a pass (``test_batching_is_invisible`` in those two files), and a
single-song call is a pool of one song through the same loop and fold, so every pooled output is held to np.array_equal on the
uint32 view against the single-song call on the same engine; the library's pass counters prove that the chunks really were
pooled.  The two folds alone are held to their definition on chunk buffers the tests make up."""
import filecmp
import os

import numpy as np
import pytest

from tests import separate_cases as SC
from tests import test_gpu_mdxc as TM
from tests import test_gpu_roformer as TR

pytestmark = pytest.mark.gpu
TFC_SONGS = (100, 241, 3000, 240, 1)         # chunk 240: under a chunk, one over, many chunks, exactly one, the minimum
ROF_SONGS = (320, 321, 1500, 777, 640)       # chunk 320: exactly one, one over (re-anchored tail), two re-anchored chunks at step 200, ...


@pytest.fixture(scope="module")
def A():
    import audio_separator_amd as A
    return A


def even_batches(nk, max_b):
    nbatch = -(-nk // max_b)
    return -(-nk // nbatch)


def passes(nk, max_b):
    return -(-nk // even_batches(nk, max_b))


def mixes_for(lengths, seed):
    return [(0.4 * np.random.default_rng(seed + i).standard_normal((2, n))).astype(np.float32) for i, n in enumerate(lengths)]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def run_pool(eng, kind, mixes, arg, rows):
    """the pooled call on NaN-filled outputs -> (outs as numpy, pass-counter delta)"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    d_mix = [torch.from_numpy(m).cuda() for m in mixes]
    d_out = [torch.full((rows, 2, m.shape[1]), float("nan"), dtype=torch.float32, device="cuda") for m in mixes]
    name = "v3_net_passes" if kind == "tfc" else "rof_net_passes"
    call = eng.mdxc_demix_batch_dev if kind == "tfc" else eng.rof_demix_batch_dev
    n0 = eng.counter(name)
    call([(m.data_ptr(), o.data_ptr(), m.shape[1]) for m, o in zip(d_mix, d_out)], arg, stream=st)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in d_out], eng.counter(name) - n0


def run_singles(eng, kind, mixes, arg):
    name = "v3_net_passes" if kind == "tfc" else "rof_net_passes"
    n0 = eng.counter(name)
    outs = [eng.mdxc_demix(m, arg) if kind == "tfc" else eng.rof_demix(m, arg) for m in mixes]
    return outs, eng.counter(name) - n0


@pytest.mark.parametrize("cfg_name,seed,overlap,seg", [("CFG2", 5, 4, None), ("CFG1", 6, 4, None), ("CFG2", 5, 8, 12)])
def test_tfc_pool_equals_the_single_song_call(A, cfg_name, seed, overlap, seg):
    cfg = getattr(TM, cfg_name)
    eng = TM.demixer(A, cfg, seed, overlap, seg=seg, max_batch=5).engine
    mixes = mixes_for(TFC_SONGS, 300)
    rows = eng.v3_cfg.num_targets
    want, single_passes = run_singles(eng, "tfc", mixes, overlap)
    got, pool_passes = run_pool(eng, "tfc", mixes, overlap, rows)
    counts = [eng.mdxc_plan(n, overlap)["n_chunks"] for n in TFC_SONGS]
    print("tfc chunks", counts, "passes pooled / single", pool_passes, single_passes)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all() and same_bits(g, w), (i, TFC_SONGS[i])
    assert pool_passes == passes(sum(counts), 5) and single_passes == sum(passes(c, 5) for c in counts)
    assert pool_passes < single_passes
    assert float(np.abs(want[2]).max()) > 0
    again, _ = run_pool(eng, "tfc", mixes, overlap, rows)                      # determinism
    assert all(same_bits(a, b) for a, b in zip(again, got))
    eng.close()


@pytest.mark.parametrize("cfg_name,seed", [("CFG", 7), ("CFG2", 8)])
@pytest.mark.parametrize("max_batch", [3, 64])
def test_roformer_pool_equals_the_single_song_call(A, cfg_name, seed, max_batch):
    cfg = getattr(TR, cfg_name)
    eng = TR.demixer(A, cfg, seed, 2, max_batch=max_batch).engine
    mixes = mixes_for(ROF_SONGS, 400)
    rows = eng.rof_cfg.n_out
    try:
        for f16x3 in (1, 0):
            eng.set_option("gemm_f16x3", f16x3)
            for step in (200, 320):
                want, single_passes = run_singles(eng, "rof", mixes, step)
                got, pool_passes = run_pool(eng, "rof", mixes, step, rows)
                counts = [-(-n // step) for n in ROF_SONGS]
                print("rof step", step, "f16x3", f16x3, "chunks", counts, "passes pooled / single", pool_passes, single_passes)
                for i, (g, w) in enumerate(zip(got, want)):
                    assert np.isfinite(g).all() and same_bits(g, w), (step, f16x3, i, ROF_SONGS[i])
                assert pool_passes == passes(sum(counts), max_batch) and single_passes == sum(passes(c, max_batch) for c in counts)
                assert pool_passes < single_passes
                assert float(np.abs(want[2]).max()) > 0
        again, _ = run_pool(eng, "rof", mixes, 320, rows)                      # determinism
        assert all(same_bits(a, b) for a, b in zip(again, got))
    finally:
        eng.set_option("gemm_f16x3", 1)
    eng.close()


def test_pool_of_35_songs_crosses_the_table_group(A):
    """more songs than one launch of the table kernel carries by value (POOL_GROUP = 32)"""
    eng = TR.demixer(A, TR.CFG, 7, 2, max_batch=8).engine
    lengths = tuple(range(320, 355))
    mixes = mixes_for(lengths, 500)
    want, _ = run_singles(eng, "rof", mixes, 200)
    got, pool_passes = run_pool(eng, "rof", mixes, 200, eng.rof_cfg.n_out)
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all() and same_bits(g, w), (i, lengths[i])
    assert pool_passes == passes(70, 8)
    eng.close()


def test_argument_errors_leave_the_outputs_untouched(A):
    """every argument is checked on the host before anything is enqueued"""
    import torch
    eng = TR.demixer(A, TR.CFG, 7, 2, max_batch=3).engine
    lengths = (640, 320, 100, 777)
    d_mix = [torch.from_numpy(m).cuda() for m in mixes_for(lengths, 600)]
    d_out = [torch.full((eng.rof_cfg.n_out, 2, n), float("nan"), dtype=torch.float32, device="cuda") for n in lengths]
    songs = [(m.data_ptr(), o.data_ptr(), m.shape[1]) for m, o in zip(d_mix, d_out)]
    n0 = eng.counter("rof_net_passes")
    with pytest.raises(A.engine.AsxError, match=r"song 2: mix \(100 samples\) shorter than one chunk"):
        eng.rof_demix_batch_dev(songs, 200)
    with pytest.raises(A.engine.AsxError, match="null pointer in song 1"):
        eng.rof_demix_batch_dev([songs[0], (0, songs[1][1], 320)], 200)
    with pytest.raises(A.engine.AsxError, match="song 0: n_samples must be >= 1"):
        eng.rof_demix_batch_dev([(songs[0][0], songs[0][1], 0)], 200)
    torch.cuda.synchronize()
    assert eng.counter("rof_net_passes") == n0
    assert all(bool(torch.isnan(o).all()) for o in d_out)
    eng.rof_demix_batch_dev([], 200)                                           # an empty pool is valid
    eng.close()
    v3 = TM.demixer(A, TM.CFG1, 6, 4).engine
    with pytest.raises(A.engine.AsxError, match="song 0: n_samples must be >= 1"):
        v3.mdxc_demix_batch_dev([(songs[0][0], songs[0][1], 0)], 4)
    with pytest.raises(A.engine.AsxError, match="asx_rof_demix_batch_dev: weights not committed"):
        v3.rof_demix_batch_dev(songs[:1], 200)
    assert v3.mdxc_demix_batch([], 4) == []
    v3.close()


def test_demixer_demix_many_equals_demix(A):
    """MDXCDemixer.demix_many / demix_many_dev: the stem dictionaries of ``demix``, the residual stem made per song"""
    import torch
    for dm, lengths in ((TM.demixer(A, TM.CFG1, 6, 4, max_batch=5), (100, 700, 241)), (TR.demixer(A, TR.CFG, 7, 2, max_batch=3), (320, 900, 321))):
        mixes = mixes_for(lengths, 700)
        want = [dm.demix(m) for m in mixes]
        got = dm.demix_many(mixes)
        res = dm.demix_many_dev([torch.from_numpy(m).cuda() for m in mixes])
        torch.cuda.synchronize()
        for w, g, (names, stems_d) in zip(want, got, res):
            assert list(w) == list(g) == names and len(names) == 2
            for r, k in enumerate(names):
                assert same_bits(w[k], g[k]) and same_bits(w[k], stems_d[r].cpu().numpy()), k
        dm.engine.close()


def test_sharding_adaptor_runs_the_pooled_call(A):
    import torch
    from audio_separator_amd.sharding import FilesPipeline, mdxc_demix_many
    eng = TM.demixer(A, TM.CFG2, 5, 4, max_batch=5).engine
    n = 700
    host = mixes_for([n] * 3, 800)
    want = [eng.mdxc_demix(m, 4) for m in host]

    def never(mix, out):
        raise AssertionError("the per-song loop ran")
    pipe = FilesPipeline(never, [torch.from_numpy(m).cuda() for m in host], 1, 0, False, demix_many=mdxc_demix_many(eng, overlap=4),
                         stem_shape=(2, 2, n))
    n0 = eng.counter("v3_net_passes")
    pipe.step(0)
    pipe.drain()
    torch.cuda.synchronize()
    assert eng.counter("v3_net_passes") - n0 == passes(3 * eng.mdxc_plan(n, 4)["n_chunks"], 5)
    for s in range(3):
        assert same_bits(pipe.outs[0][s].cpu().numpy(), want[s]), s
    eng.close()


# ---- the folds alone, against their definition ------------------------------------------------------------------------------
def run_fold(eng, kind, chunks, n, arg, rows):
    """*_finalize_dev on a chunk buffer of the test's own -> out [rows, 2, n] (NaN where the fold wrote nothing)"""
    import torch
    d_chunks = torch.from_numpy(chunks).cuda()
    d_out = torch.full((rows, 2, n), float("nan"), dtype=torch.float32, device="cuda")
    call = eng.mdxc_finalize_dev if kind == "tfc" else eng.rof_finalize_dev
    call(d_chunks.data_ptr(), n, arg, d_out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_tfc_fold_equals_the_reference_loop(A):
    """mdxc_separator.py:394-404 on chunks the test makes up: ``accumulated[k*step : k*step+C] += chunk_k``, the front zeros cropped,
    ``/ overlap``.  Integer-valued chunks in [-8, 8] and overlap a power of two: every partial sum and the division are exact in
    float32, so the fold must EQUAL the loop whatever order it adds in."""
    eng = TM.demixer(A, TM.CFG2, 5, 4).engine
    S, C = eng.v3_cfg.num_targets, 240
    rng = np.random.default_rng(900)
    for overlap in (1, 2, 4, 8):
        for n in (1, 100, 240, 241, 3000):
            step = C // overlap                                             # mdxc_separator.py:364-374
            pad = step - (n - C) % step
            front = C - step
            length = front + n + pad + C - step
            nk = (length - C) // step + 1
            plan = eng.mdxc_plan(n, overlap)
            assert (plan["n_chunks"], plan["step"], plan["trim"], plan["padded_len"]) == (nk, step, front, length)
            chunks = rng.integers(-8, 9, (nk, S, 2, C)).astype(np.float32)
            acc = np.zeros((S, 2, length), np.float32)
            for k in range(nk):
                acc[..., k * step:k * step + C] += chunks[k]
            want = acc[..., front:front + n] / np.float32(overlap)
            got = run_fold(eng, "tfc", chunks, n, overlap, S)
            assert same_bits(got, want), (overlap, n)
    eng.close()


def test_roformer_fold_against_float64(A):
    """mdxc_separator.py:310-343 on standard-normal chunks: every chunk k with 0 <= i - start_k < C, in increasing k, adds
    ``x_k * w`` to the result and ``w`` to the counter; out = result / clamp(counter, 1e-10), w = float32(float64 Hamming) as the
    engine builds it.  Reference in float64.  For a sample covered by n chunks the bound is (2n + 6) * 2^-24 * sum|x_k w| / sum w:
    float32 rounding of n products and n additions in the numerator, n additions in the denominator and one division (each a
    relative 2^-24 of a term bounded by sum|x_k w| / sum w); the rest covers the window table's own rounding."""
    eng = TR.demixer(A, TR.CFG, 7, 2).engine
    S, rows, C = eng.rof_cfg.num_stems, eng.rof_cfg.n_out, 320
    assert rows > S == 1                                                    # out row o reads chunk stem o % S
    w = (0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(C) / (C - 1))).astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(901)
    for step in (200, 320):
        for n in (320, 321, 640, 777, 1500):
            starts = [n - C if i + C > n else i for i in range(0, n, step)]  # mdxc_separator.py:320-341
            assert eng.rof_plan(n, step) == {"n_chunks": len(starts), "chunk_size": C}
            chunks = rng.standard_normal((len(starts), S, 2, C)).astype(np.float32)
            num, mag, den, cover = (np.zeros((S, 2, n)) for _ in range(4))
            for k, st in enumerate(starts):
                num[..., st:st + C] += chunks[k].astype(np.float64) * w
                mag[..., st:st + C] += np.abs(chunks[k].astype(np.float64)) * w
                den[..., st:st + C] += w
                cover[..., st:st + C] += 1
            assert cover.min() >= 1
            want = num / np.maximum(den, 1e-10)
            tol = (2 * cover + 6) * 2.0 ** -24 * mag / den
            got = run_fold(eng, "rof", chunks, n, step, rows)
            for o in range(rows):
                err = np.abs(got[o].astype(np.float64) - want[o % S])
                print("rof fold step", step, "n", n, "row", o, "max err / tol", float((err / tol[o % S]).max()))
                assert np.isfinite(got[o]).all() and (err <= tol[o % S]).all(), (step, n, o)
    eng.close()


# ---- files ------------------------------------------------------------------------------------------------------------------
RATE = 100                                   # the toy rate: a file under 1000 samples is "short"


def _wav(tmp_path, name, n, seed, subtype="PCM_16"):
    from audio_separator_amd import audio_io
    p = str(tmp_path / name)
    x = (0.3 * np.random.default_rng(seed).standard_normal((n, 2))).astype(np.float32)
    audio_io.write_wav(p, np.clip(x, -0.99, 0.99), RATE, subtype)
    return p


@pytest.mark.parametrize("family", ["mdxc", "roformer"])
def test_separate_many_writes_the_files_of_separate(tmp_path, monkeypatch, family):
    """[long, short, long] on the device file path: the short file switches the configured segment size on for itself and the
    third; a 24-bit file and one only the host decoder takes (64-bit float) share the pools with the 16-bit ones; a silent file and
    (Roformer) one shorter than a chunk fail alone."""
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    _, cls, common, arch, _, _ = SC.cases(family, str(tmp_path))[0]
    if family == "roformer":
        arch = dict(arch, segment_size=11)       # the override geometry: chunk 160 against the model's 320
    arch = dict(arch, asx_max_batch=5)
    good = [_wav(tmp_path, "a.wav", 1500, 1), _wav(tmp_path, "a24.wav", 1100, 2, "PCM_24"), _wav(tmp_path, "b.wav", 500, 3),
            _wav(tmp_path, "c.wav", 1200, 4), _wav(tmp_path, "d64.wav", 1300, 5, "DOUBLE")]
    silent = _wav(tmp_path, "silent.wav", 700, 6)
    with open(silent, "r+b") as f:
        f.seek(44)
        f.write(bytes(700 * 4))
    tiny = _wav(tmp_path, "tiny.wav", 100, 7)
    paths = [good[0], good[1], silent, good[2], tiny, good[3], good[4]]
    bad = [2, 4] if family == "roformer" else [2]

    def make(out_dir):
        return SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, sample_rate=RATE), arch_config=arch)
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    sep = make(one_dir)
    want = []
    for p in paths:
        try:
            want.append(sep.separate(p))
        except Exception:
            want.append([])
        sep.clear_file_specific_paths()
    assert [i for i, w in enumerate(want) if not w] == bad
    sep.clear_gpu_cache()
    from audio_separator_amd.mdxc import MDXCDemixer
    calls = []
    pooled_call = MDXCDemixer.demix_many_dev
    monkeypatch.setattr(MDXCDemixer, "demix_many_dev", lambda self, mixes_d: calls.append(len(mixes_d)) or pooled_call(self, mixes_d))
    sep = make(many_dir)
    name = "rof_net_passes" if family == "roformer" else "v3_net_passes"
    n0 = sep.engine.counter(name)
    got = sep.separate_many(paths)
    pooled = sep.engine.counter(name) - n0
    assert got == want and sorted(sep.batch_errors) == bad
    assert calls == [2, len(paths) - len(bad) - 2]                      # two pools: the files before the short one, the rest
    assert all(isinstance(sep.batch_errors[i], ValueError) for i in bad)
    for names in got:
        for nm in names:
            assert filecmp.cmp(os.path.join(one_dir, nm), os.path.join(many_dir, nm), shallow=False), nm
    assert sep.override_model_segment_size is True and sorted(sep._demixers) == [False, True]
    assert sep.audio_file_path == good[4] and sep.audio_file_base == "d64" and sep.primary_source is not None
    # two pools (the files before the short one, the rest), each in as few passes as its chunks need
    dm0, dm1 = sep._demixers[False], sep._demixers[True]
    if family == "roformer":
        count = lambda dm, n: -(-n // dm.roformer_step())  # noqa: E731
    else:
        count = lambda dm, n: dm.engine.mdxc_plan(n, int(dm.overlap))["n_chunks"]  # noqa: E731
    tail = [500, 1200, 1300] + ([100] if family == "mdxc" else [])
    assert pooled == passes(count(dm0, 1500) + count(dm0, 1100), 5) + passes(sum(count(dm1, n) for n in tail), 5)
    # a small asx_pool_chunks splits the pools; no byte changes
    split_dir = str(tmp_path / "split")
    sep2 = SC.plugin_class(cls)(common_config=dict(common, output_dir=split_dir, sample_rate=RATE), arch_config=dict(arch, asx_pool_chunks=9))
    del calls[:]
    assert sep2.separate_many(paths) == want
    assert len(calls) > 2 and sum(calls) == len(paths) - len(bad)
    for names in got:
        for nm in names:
            assert filecmp.cmp(os.path.join(one_dir, nm), os.path.join(split_dir, nm), shallow=False), nm
    sep.clear_gpu_cache()
    sep2.clear_gpu_cache()
