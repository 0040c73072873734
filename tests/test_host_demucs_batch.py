"""The Demucs batch path above and below the GPU, without one.

* The pool plan of csrc/apply_plan.h (apply_pool_build, compiled with g++ through tests/host/apply_pool_host.cpp) against the
  concatenation, song by song, of the oracles' plans -- oracle.demucs_oracle.segment_plan for v4, oracle.hdemucs_oracle.
  hd_segment_plan for v3 -- with every number compared for equality, and a rejected song rejecting the whole pool.
* DemucsDemixer.demix_many / DemucsSeparator.separate_many over an engine double defined here: the order of the random draws,
  the order in which a bag accumulates, the segments_enabled=False fallback, and a bad file failing alone."""
import os
import random
import subprocess

import numpy as np
import pytest

from tests.test_host_apply_plan import reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the pool plan ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("applypool") / "apply_pool_host")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "host", "apply_pool_host.cpp")], check=True)
    return exe


def run_pool(exe, seg, sr, overlap, centered, shifts, songs):
    """songs: [(N, [offsets])]"""
    args = [exe, str(seg), str(sr), repr(float(overlap)), str(int(centered)), str(shifts), str(len(songs))]
    for n, offs in songs:
        args += [str(n)] + [str(o) for o in offs]
    return subprocess.run(args, capture_output=True, text=True)


def parse_pool(out):
    rows = [line.split() for line in out.splitlines()]
    head = [r for r in rows if r[0] == "pool"]
    assert len(head) == 1 and all(r[0] in ("pool", "shift", "seg") for r in rows)
    stride, max_shift, segment, nsh = (int(v) for v in head[0][1:])
    shifts = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "shift"]     # song, offset, VL, first, nk
    segs = [tuple(int(v) for v in r[1:]) for r in rows if r[0] == "seg"]         # song, start, clen
    return stride, max_shift, segment, nsh, shifts, segs


@pytest.mark.parametrize("centered", [True, False], ids=["v4_centred", "v3_own_length"])
@pytest.mark.parametrize("overlap", (0.0, 0.25, 0.75))
@pytest.mark.parametrize("sr,seconds", ((200, 3), (601, 1)))
def test_pool_plan_is_the_concatenation_of_the_oracle_plans(pool_exe, sr, seconds, overlap, centered):
    seg = sr * seconds
    stride = int((1 - overlap) * seg)
    ms = sr // 2
    lengths = [seg // 2 - 7, 3 * stride + 1, 3 * stride + 1, 7 * stride - 1, seg]     # below a segment, two equal, long, exactly one
    for shifts, draw in ((0, lambda i: []), (1, lambda i: [(i * 37) % (ms + 1)]), (3, lambda i: [0, ms, (i * 53 + 1) % (ms + 1)])):
        songs = [(n, draw(i)) for i, n in enumerate(lengths)]
        r = run_pool(pool_exe, seg, sr, overlap, centered, shifts, songs)
        assert r.returncode == 0, (r.stdout, r.stderr)
        g_stride, g_ms, g_seg, nsh, got_shifts, got_segs = parse_pool(r.stdout)
        want_shifts, want_segs = [], []
        for i, (n, offs) in enumerate(songs):
            w_stride, w_ms, w_seg, per_shift, chunks = reference(n, sr, seconds, overlap, centered, shifts, offs)
            assert (g_stride, g_ms, g_seg) == (w_stride, w_ms, w_seg)
            base = len(want_segs)
            want_shifts += [(i, off, vl, base + first, nk) for (off, vl, first, nk) in per_shift]      # shift 0's chunks, shift 1's, ...
            want_segs += [(i, start, clen) for (start, clen) in chunks]
        assert nsh == max(shifts, 1)
        assert got_shifts == want_shifts
        assert got_segs == want_segs and len(got_segs) > len(songs)


@pytest.mark.parametrize("centered", [True, False], ids=["v4_centred", "v3_own_length"])
def test_one_rejected_song_rejects_the_pool(pool_exe, centered):
    sr, seg = 200, 600
    good = (1000, [3, 100])
    assert run_pool(pool_exe, seg, sr, 0.25, centered, 2, [good, good]).returncode == 0
    for slot, bad in ((0, (1000, [0, 101])), (1, (1000, [-1, 0])), (2, (0, [0, 0])), (1, (-5, [0, 0])), (0, (1, [0, 0]))):
        songs = [good, good, good]
        songs[slot] = bad
        r = run_pool(pool_exe, seg, sr, 0.25, centered, 2, songs)
        assert r.returncode == 3 and r.stdout.startswith(f"error song {slot}:"), r.stdout
        assert "seg" not in r.stdout
    r = run_pool(pool_exe, seg, sr, 1.0, centered, 0, [(1000, [])])
    assert r.returncode == 3 and "bad stride" in r.stdout
    r = run_pool(pool_exe, seg, sr, 0.25, centered, 0, [])                        # an empty pool is a valid, empty plan
    assert r.returncode == 0 and parse_pool(r.stdout)[4:] == ([], [])


# ---- demix_many / separate_many over an engine double -----------------------------------------------------------------------
class FakeEngine:
    """Records what the host layer asks for.  A "model" is {"gain": g}: source s of a demix is mix * g * (s + 1) + the sum of the
    offsets / 1000 (so the result depends on the member, the song and its draws); the demix_demucs framing adds 0.5."""
    log = []

    def __init__(self, cfg=None, device=0):
        self.device = device
        self.gain = None

    def close(self):
        pass

    def load_ht(self, hc, sd, pos_tables=True):
        self.gain = np.float32(sd["gain"])
        FakeEngine.log.append(("load", float(self.gain)))

    def _one(self, mix, offsets, standardize):
        S = 4
        out = np.stack([mix * self.gain * np.float32(s + 1) for s in range(S)]).astype(np.float32)
        out += np.float32(sum(offsets or []) / 1000.0)
        return out + np.float32(0.5) if standardize else out

    def pcm16(self, stem, max_peak=1.0, min_peak=None):               # the writer's int16 pass, as tests/fake_engine.py does it
        from oracle import mdx_oracle as O
        a = O.normalize(np.array(stem, np.float32, copy=True), max_peak, min_peak)
        return (a * 32767).astype(np.int16), float(np.abs(a).max())

    def ht_demix(self, mix, shifts=0, offsets=None, overlap=0.25, standardize=False, swap01=False):
        FakeEngine.log.append(("single", float(self.gain), list(offsets) if offsets is not None else None))
        return self._one(mix, offsets, standardize)

    def ht_demix_batch(self, mixes, shifts=0, offsets=None, overlap=0.25, standardize=False, swap01=False):
        FakeEngine.log.append(("batch", float(self.gain), [list(o) for o in offsets] if offsets is not None else None))
        return [self._one(m, offsets[i] if offsets is not None else None, standardize) for i, m in enumerate(mixes)]


@pytest.fixture()
def A(monkeypatch):
    import audio_separator_amd as A
    from audio_separator_amd import demucs
    monkeypatch.setattr(demucs, "Engine", FakeEngine)
    monkeypatch.setattr(demucs, "_cuda_ready", lambda: False)      # the double has no device path, wherever this test runs
    FakeEngine.log = []
    return A


def _demixer(A, gains, weights=None, **arch):
    hc = A.HTConfig(samplerate=8000)
    return A.DemucsDemixer({"torch_device": 0}, arch, models=[(hc, {"gain": g}) for g in gains], weights=weights)


def _mixes(lengths, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal((2, n)) * 0.3).astype(np.float32) for n in lengths]


def test_draws_come_in_song_order_then_model_order(A, monkeypatch):
    counter = iter(range(1000))
    monkeypatch.setattr(random, "randint", lambda a, b: next(counter))
    dm = _demixer(A, [1.0, 2.0], shifts=2, overlap=0.25)
    dm.demix_many(_mixes([500, 700, 900]))
    batches = [r for r in FakeEngine.log if r[0] == "batch"]
    # song 0 draws 0..3 (model 0: 0, 1; model 1: 2, 3), song 1 draws 4..7, song 2 draws 8..11 -- what a loop of demix() consumes
    assert batches == [("batch", 1.0, [[0, 1], [4, 5], [8, 9]]), ("batch", 2.0, [[2, 3], [6, 7], [10, 11]])]


@pytest.mark.parametrize("gains,weights", [([1.5], None), ([1.0, 2.0, 0.5], [[1.0, 0.5, 2.0, 1.0], [0.5, 1.5, 1.0, 1.0], [2.0, 1.0, 1.0, 3.0]])])
def test_seeded_batch_equals_seeded_loop(A, gains, weights):
    mixes = _mixes([300, 1201, 1201, 77])
    dm = _demixer(A, gains, weights, shifts=2, overlap=0.25)
    random.seed(7)
    many = dm.demix_many(mixes)
    random.seed(7)
    loop = [dm.demix(m) for m in mixes]
    assert len(many) == len(loop) == 4
    for a, b in zip(many, loop):
        assert a.shape == b.shape and a.dtype == np.float32 and np.array_equal(a, b)
    fixed = [[[s, 1 + i] for i in range(len(gains))] for s in range(4)]
    for a, m, o in zip(dm.demix_many(mixes, offsets=fixed), mixes, fixed):
        assert np.array_equal(a, dm.demix(m, offsets=o))
    with pytest.raises(ValueError):
        dm.demix_many(mixes, offsets=fixed[:2])
    with pytest.raises(ValueError):
        dm.demix_many([mixes[0], mixes[1][:1]])
    assert dm.demix_many([]) == []


def test_bag_accumulates_member_by_member(A):
    mixes = _mixes([640, 333])
    weights = [[1.0, 0.5, 2.0, 1.0], [0.5, 1.5, 1.0, 1.0]]
    dm = _demixer(A, [1.0, 3.0], weights, shifts=0)
    got = dm.demix_many(mixes)
    assert [r[:2] for r in FakeEngine.log] == [("load", 1.0), ("batch", 1.0), ("load", 3.0), ("batch", 3.0)]    # one pooled call per member
    import torch
    for mix, out in zip(mixes, got):
        t = torch.from_numpy(mix)
        ref = t.mean(0)
        std = ((t - ref.mean()) / ref.std()).numpy()
        est = None
        for g, w in zip((1.0, 3.0), weights):
            o = np.stack([std * np.float32(g) * np.float32(s + 1) for s in range(4)]).astype(np.float32) * np.asarray(w, np.float32)[:, None, None]
            est = o if est is None else est + o
        est /= (np.asarray(weights[0], np.float32) + np.asarray(weights[1], np.float32))[:, None, None]
        est = est * float(ref.std()) + float(ref.mean())
        est[[0, 1]] = est[[1, 0]]
        assert np.array_equal(out, est)


def test_segments_disabled_runs_the_per_song_loop(A, monkeypatch):
    dm = _demixer(A, [1.0], shifts=1, segments_enabled=False)
    calls = []
    monkeypatch.setattr(dm, "demix", lambda mix, offsets=None: calls.append((mix.shape, offsets)) or np.zeros((4,) + mix.shape, np.float32))
    outs = dm.demix_many(_mixes([100, 200]), offsets=[[[5]], [[9]]])
    assert calls == [((2, 100), [[5]]), ((2, 200), [[9]])] and [o.shape for o in outs] == [(4, 2, 100), (4, 2, 200)]
    assert not any(r[0] == "batch" for r in FakeEngine.log)
    assert dm.demix_many_dev([]) is None


def test_separate_many_isolates_a_bad_file(A, tmp_path, monkeypatch):
    import filecmp
    from audio_separator_amd import audio_io
    from audio_separator_amd.architectures.demucs_separator import DemucsSeparator
    from tests.separate_cases import common_config
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    wavs = []
    for i, n in enumerate((4000, 6100, 2500)):
        p = str(tmp_path / f"in{i}.wav")
        audio_io.write_wav(p, np.clip(_mixes([n], seed=20 + i)[0].T, -0.99, 0.99), 8000, "PCM_16")
        wavs.append(p)
    bad = str(tmp_path / "broken.wav")
    with open(bad, "w") as f:
        f.write("not audio")
    paths = [wavs[0], bad, wavs[1], str(tmp_path / "missing.wav"), wavs[2]]

    def make(out_dir):
        common = common_config("fake", "fake.yaml", {}, out_dir, sample_rate=8000, asx_models=[(A.HTConfig(samplerate=8000), {"gain": 0.25})])
        return DemucsSeparator(common_config=common, arch_config={"shifts": 2, "overlap": 0.25, "segments_enabled": True})
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    sep = make(one_dir)
    random.seed(11)
    want = [sep.separate(p) for p in (wavs[0], wavs[1], wavs[2])]
    sep = make(many_dir)
    random.seed(11)
    got = sep.separate_many(paths)
    assert got[1] == [] and got[3] == [] and sorted(sep.batch_errors) == [1, 3]
    assert all(isinstance(e, Exception) for e in sep.batch_errors.values())
    assert [got[0], got[2], got[4]] == want and all(len(names) == 4 for names in want)
    for names in want:
        for name in names:
            assert filecmp.cmp(os.path.join(one_dir, name), os.path.join(many_dir, name), shallow=False), name
    assert sep.separate_many([bad]) == [[]] and list(sep.batch_errors) == [0]
