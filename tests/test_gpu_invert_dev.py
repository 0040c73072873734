"""invert_stem with every array in HBM (asx_invert_stem_dev, asx_invert_stem_batch_dev; csrc/kernels_ens.h, csrc/engine_ens.h) and the
MDX plugin's ``invert_using_spec`` on the device-resident file path.

Kernel level: the device forms against ``Engine.invert_stem`` -- the host-array call -- bit for bit, for a planar and for a rows stem
and with the stem scaled on the way in (``stem_scale`` = one float32 multiplication = numpy's ``stem * np.float32(scale)``); against
the float64 statement of tests/ensemble_ref.py at the bar of tests/test_gpu_ensemble_kernels.py (5e-6 in ``scaled_err``, not fitted
to the kernel; measured on an MI355X: 3.1e-7 / 3.3e-7 plain / weighted peak on uniform noise, 1.7e-6 / 1.8e-6 where the stem is louder
than the mix); the pooled form against the single one, bit for bit, with its refusals.

Plugin level: the tiny MDX case with ``invert_using_spec=True`` -- ``separate``, ``stems_dev``, ``separate_many`` and an
``EnsembleSeparator`` of two such members -- against the host path (``ASX_FILE_FASTPATH=0``, ``via_files=True``), byte for byte."""
import filecmp
import functools
import os

import numpy as np
import pytest

from tests import ensemble_ref as R
from tests import separate_cases as SC

pytestmark = pytest.mark.gpu

BAR = 5e-6                                     # tests/test_gpu_ensemble_kernels.py
SIZES = (700, 1023, 1024, 1025, 2047, 2048, 3071, 5000)
SCALES = (1.0, 1.035)
POOL = ((3000, "rows"), (1024, "planar"), (700, "rows"), (6100, "planar"), (2048, "rows"))
POOL_SCALE = 1.035
SENTINEL = -7.5


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))
    yield e
    e.close()


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


@functools.lru_cache(maxsize=None)
def pair(n, seed=0):
    """(mix, stem), float32 [2, n], uniform in [-1, 1]"""
    rng = np.random.default_rng(1000 * seed + n)
    out = tuple(rng.uniform(-1.0, 1.0, (2, n)).astype(np.float32) for _ in range(2))
    for x in out:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def host_result(eng, n, scale, seed=0):
    """Engine.invert_stem -- the host-array call -- on the stem multiplied by numpy: [n_out, 2]"""
    mix, stem = pair(n, seed)
    r = eng.invert_stem(mix, stem * np.float32(scale))
    r.setflags(write=False)
    return r


def upload(x):
    import torch
    return torch.from_numpy(np.array(x, dtype=np.float32, order="C", copy=True)).to(torch.device("cuda", 0))


def stem_as(stem, layout):
    return upload(stem if layout == "planar" else stem.T)


def run_single(eng, mix, stem, layout, scale, capacity=None):
    """invert_stem_dev over uploaded arrays -> (n_out, the whole output buffer [capacity + 8, 2] on the host)"""
    import torch
    n = mix.shape[1]
    capacity = 1024 * (n // 1024) if capacity is None else capacity
    d_mix, d_stem = upload(mix), stem_as(stem, layout)
    out = torch.full((capacity + 8, 2), SENTINEL, dtype=torch.float32, device=d_mix.device)
    n_out = eng.invert_stem_dev(d_mix.data_ptr(), d_stem.data_ptr(), n, layout, scale, out.data_ptr(), capacity)
    torch.cuda.synchronize()
    return n_out, out.cpu().numpy()


# ---- the single form ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("n", SIZES)
def test_single_equals_the_host_call(eng, n, scale):
    mix, stem = pair(n)
    want = host_result(eng, n, scale)
    assert want.shape == (1024 * (n // 1024), 2)
    for layout in ("planar", "rows"):
        n_out, buf = run_single(eng, mix, stem, layout, scale)
        assert n_out == want.shape[0] == (0 if n < 1024 else n_out), (layout, n_out)
        assert np.array_equal(bits(buf[:n_out]), bits(want)), (layout, n, scale)
        assert (buf[n_out:] == SENTINEL).all(), layout            # nothing beyond [n_out, 2]


def louder_stem(n):
    """tests/test_gpu_ensemble_kernels.py's case: the stem louder than the mix, the result a small difference of two large terms"""
    mix = R.members(60, n, 1)[0]
    noise = (np.random.default_rng(61).standard_normal(mix.shape) * 0.3).astype(np.float32)
    return mix, (np.float32(2.0) * mix + np.float32(0.2) * noise).astype(np.float32)


@pytest.mark.parametrize("what", ("uniform 5000", "stem louder than mix 5121"))
def test_single_against_float64(eng, what):
    if what.startswith("uniform"):
        mix, stem = pair(5000)
    else:
        mix, stem = louder_stem(5121)
    n = mix.shape[1]
    for layout, scale in (("rows", 1.035), ("planar", 1.0)):
        n_out, buf = run_single(eng, mix, stem, layout, scale)
        ref = R.invert_stem(mix, (stem * np.float32(scale)).astype(np.float32))
        got = buf[:n_out]
        assert got.shape == ref.shape and np.isfinite(got).all()
        e1, e2 = R.scaled_err(got.T, ref.T, n), R.scaled_err(got.T, ref.T, n, peak="weighted")
        print(f"INVERT_DEV {what} {layout} scale={scale} scaled_err {e1:.3e} weighted-peak {e2:.3e}")
        assert e1 <= BAR and e2 <= BAR, (what, layout, e1, e2)


def test_single_refusals(eng):
    import torch
    import audio_separator_amd as A
    mix, stem = pair(3071)
    d_mix, d_stem = upload(mix), upload(stem)
    out = torch.full((2048, 2), SENTINEL, dtype=torch.float32, device=d_mix.device)
    m, s, o = d_mix.data_ptr(), d_stem.data_ptr(), out.data_ptr()
    for args in ((0, s, 3071, "planar", 1.0, o, 2048), (m, 0, 3071, "planar", 1.0, o, 2048), (m, s, 3071, "planar", 1.0, 0, 2048),
                 (m, s, 3071, "rows", 1.0, o, 2047), (m, s, 0, "rows", 1.0, o, 2048)):
        with pytest.raises(A.AsxError, match="asx_invert_stem_dev"):
            eng.invert_stem_dev(*args)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    assert eng.invert_stem_dev(m, s, 700, "planar", 1.0, 0, 0) == 0           # no result: no output needed


# ---- the pooled form ----------------------------------------------------------------------------------------------------------------
def pool_buffers():
    """uploaded (mix, stem in its layout, sentinel-filled output with 8 spare rows) per song of POOL"""
    import torch
    bufs = []
    for i, (n, layout) in enumerate(POOL):
        mix, stem = pair(n, seed=i + 1)
        d_mix = upload(mix)
        out = torch.full((1024 * (n // 1024) + 8, 2), SENTINEL, dtype=torch.float32, device=d_mix.device)
        bufs.append((d_mix, stem_as(stem, layout), out))
    return bufs


def pool_songs(bufs):
    return [(m.data_ptr(), s.data_ptr(), n, layout, o.data_ptr(), o.shape[0] - 8) for (n, layout), (m, s, o) in zip(POOL, bufs)]


def test_pool_equals_the_single_calls(eng):
    import torch
    bufs = pool_buffers()
    n_outs = eng.invert_stem_batch_dev(pool_songs(bufs), POOL_SCALE)
    torch.cuda.synchronize()
    first = [o.cpu().numpy() for _, _, o in bufs]
    assert n_outs == [1024 * (n // 1024) for n, _ in POOL] and n_outs[2] == 0
    for i, (n, layout) in enumerate(POOL):
        mix, stem = pair(n, seed=i + 1)
        n_out, want = run_single(eng, mix, stem, layout, POOL_SCALE)
        assert n_out == n_outs[i]
        assert np.array_equal(bits(first[i]), bits(want)), (i, n, layout)       # the result and the sentinels behind it
        assert np.array_equal(bits(want[:n_out]), bits(host_result(eng, n, POOL_SCALE, seed=i + 1)))
    # a second run into fresh buffers: the same bits
    again = pool_buffers()
    assert eng.invert_stem_batch_dev(pool_songs(again), POOL_SCALE) == n_outs
    torch.cuda.synchronize()
    for a, (_, _, o) in zip(first, again):
        assert np.array_equal(bits(a), bits(o.cpu().numpy()))
    assert eng.invert_stem_batch_dev([], POOL_SCALE) == []


@pytest.mark.parametrize("bad", ("capacity", "null mix", "null stem", "null out", "layout", "empty"))
def test_pool_checks_every_song_before_it_runs(eng, bad):
    import torch
    import audio_separator_amd as A
    bufs = pool_buffers()
    songs = pool_songs(bufs)
    m, s, n, layout, o, cap = songs[3]
    songs[3] = {"capacity": (m, s, n, layout, o, cap - 1), "null mix": (0, s, n, layout, o, cap), "null stem": (m, 0, n, layout, o, cap),
                "null out": (m, s, n, layout, 0, cap), "layout": (m, s, n, layout, o, cap), "empty": (m, s, 0, layout, o, cap)}[bad]
    if bad == "layout":
        import ctypes as C
        from audio_separator_amd import engine as E
        arr = (E._InvertSong * len(songs))()
        for i, (mp, sp, nn, lay, op, cp) in enumerate(songs):
            arr[i] = E._InvertSong(mp, sp, op, nn, cp, -1, 7 if i == 3 else eng.SLOT_LAYOUTS[lay])
        assert eng._lib.asx_invert_stem_batch_dev(eng._h, arr, len(songs), C.c_float(POOL_SCALE), None) != 0
        assert b"song 3" in eng._lib.asx_last_error()
        assert [arr[i].n_out for i in range(len(songs))] == [-1] * len(songs)   # no n_out written either
    else:
        with pytest.raises(A.AsxError, match="song 3"):
            eng.invert_stem_batch_dev(songs, POOL_SCALE)
    torch.cuda.synchronize()
    for _, _, out in bufs:
        assert (out == SENTINEL).all()


# ---- the MDX plugin ---------------------------------------------------------------------------------------------------------------------
def _case(tmp, idx=0):
    tag, cls, common, arch, wav, custom = SC.cases("mdx", str(tmp))[idx]
    return cls, dict(common, invert_using_spec=True), arch, wav


def _plugin(tmp, out_dir=None, idx=0, **over):
    cls, common, arch, _ = _case(tmp, idx)
    if out_dir is not None:
        common = dict(common, output_dir=str(out_dir))
    return SC.plugin_class(cls)(common_config=dict(common, **over), arch_config=arch)


def _blobs(out_dir, names):
    blobs = []
    for n in names:
        full = os.path.join(str(out_dir), n)
        blobs.append(open(full, "rb").read() if os.path.isfile(full) else None)
    return blobs


def test_separate_equals_the_host_path(tmp_path, monkeypatch):
    wav = _case(tmp_path)[3]

    def run(fast):
        monkeypatch.setenv("ASX_FILE_FASTPATH", "1" if fast else "0")
        out = tmp_path / ("dev" if fast else "host")
        inst = _plugin(tmp_path, out, asx_profile_file=True)
        names = inst.separate(wav, None)
        srcs = (np.array(inst.secondary_source, copy=True), np.array(inst.primary_source, copy=True))
        return names, srcs, _blobs(out, names), dict(inst.file_timings)
    names_d, srcs_d, blobs_d, t_d = run(True)
    assert "h2d_decode" in t_d and "demix" in t_d and "invert" in t_d, t_d          # the device path ran, invert_stem included
    names_h, srcs_h, blobs_h, t_h = run(False)
    assert "h2d_decode" not in t_h and "invert" not in t_h
    assert names_d == names_h and len(names_d) == 2
    assert srcs_d[0].shape == (2048, 2) and srcs_d[1].shape == (3000, 2)
    for a, b in zip(srcs_d, srcs_h):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    assert None not in blobs_d and blobs_d == blobs_h


def test_stems_dev_keeps_both_stems_on_the_device(tmp_path, monkeypatch):
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    wav = _case(tmp_path)[3]
    inst = _plugin(tmp_path)
    stems = inst.stems_dev(wav)
    assert isinstance(stems, list) and [name for name, _, _ in stems] == [inst.secondary_stem_name, inst.primary_stem_name]
    (_, sec, lay_s), (_, prim, lay_p) = stems
    assert sec.is_cuda and prim.is_cuda and lay_s == lay_p == "rows"
    assert tuple(prim.shape) == (3000, 2) and tuple(sec.shape) == (1024 * (3000 // 1024), 2)
    host = _plugin(tmp_path, tmp_path / "h")
    monkeypatch.setenv("ASX_FILE_FASTPATH", "0")
    host.separate(wav, None)
    assert np.array_equal(bits(sec.cpu().numpy()), bits(np.array(host.secondary_source)))
    assert np.array_equal(bits(prim.cpu().numpy()), bits(np.array(host.primary_source)))


def test_separate_many_equals_the_per_file_loop(tmp_path, monkeypatch):
    from audio_separator_amd import audio_io
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    wav = _case(tmp_path)[3]
    x, sr = audio_io.read_wav(wav)
    paths = []
    for n in (x.shape[1], 2500, 700):                       # 700: fewer than 1024 samples, no secondary stem
        p = str(tmp_path / f"song_{n}.wav")
        audio_io.write_wav(p, np.ascontiguousarray(x[:, :n].T), sr, "PCM_16")
        paths.append(p)
    pooled = _plugin(tmp_path, tmp_path / "pooled")
    got = pooled.separate_many(paths)
    assert pooled.batch_errors == {} and all(len(g) == 2 for g in got)
    loop = _plugin(tmp_path, tmp_path / "loop")
    want = []
    for p in paths:
        want.append(loop.separate(p, None))
        loop.clear_gpu_cache()
        loop.clear_file_specific_paths()
    assert got == want
    for names in got:
        a, b = _blobs(tmp_path / "pooled", names), _blobs(tmp_path / "loop", names)
        assert a == b and a[1] is not None
    assert _blobs(tmp_path / "pooled", got[2])[0] is None and None not in _blobs(tmp_path / "pooled", got[0] + got[1])


def test_ensemble_of_two_members_takes_the_device_path(tmp_path, monkeypatch):
    import audio_separator_amd as A
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    wav = _case(tmp_path)[3]
    # the plain net and the denoise / overlap 0.1 variant, under a name of its own: the intermediate files carry the model's name
    members = [_plugin(tmp_path, idx=0), _plugin(tmp_path, idx=2, model_name="net_small_denoise")]
    assert all(m.invert_using_spec for m in members)
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


def test_ensemble_with_a_file_under_one_hop(tmp_path, monkeypatch):
    """A file of fewer than 1024 samples has no secondary stem: the members leave it out of ``stems_dev`` / ``stems_dev_many`` as their
    writers leave its file out, the primary group is ensembled on the device path, and the other files of a batch are unaffected."""
    import torch
    import audio_separator_amd as A
    from audio_separator_amd import audio_io
    monkeypatch.setenv("ASX_FILE_FASTPATH", "1")
    wav = _case(tmp_path)[3]
    x, sr = audio_io.read_wav(wav)
    paths = [wav]
    for n in (700, 2500):
        p = str(tmp_path / f"song_{n}.wav")
        audio_io.write_wav(p, np.ascontiguousarray(x[:, :n].T), sr, "PCM_16")
        paths.append(p)
    short = paths[1]
    members = [_plugin(tmp_path, idx=0), _plugin(tmp_path, idx=2, model_name="net_small_denoise")]
    stems = members[0].stems_dev(short)
    members[0].clear_file_specific_paths()
    assert [name for name, _, _ in stems] == [members[0].primary_stem_name] and tuple(stems[0][1].shape) == (700, 2)
    many, _ = members[0].stems_dev_many(paths)
    assert [len(s) for s in many] == [2, 1, 2] and all(isinstance(t, torch.Tensor) and t.shape[0] > 0 for s in many for _, t, _ in s)
    by_files = A.EnsembleSeparator(members, "avg_wave", None, via_files=True)
    by_files.output_dir = str(tmp_path / "files")
    want = [by_files.separate(p, None) for p in paths]
    assert [len(w) for w in want] == [2, 1, 2]                     # the short file: the primary group only
    one = A.EnsembleSeparator(members, "avg_wave", None)
    one.output_dir = str(tmp_path / "one")
    got = one.separate(short, None)
    assert one.last_path_taken == "device"
    assert [os.path.basename(f) for f in got] == [os.path.basename(f) for f in want[1]]
    assert filecmp.cmp(got[0], want[1][0], shallow=False)
    pooled = A.EnsembleSeparator(members, "avg_wave", None)
    pooled.output_dir = str(tmp_path / "pooled")
    got_many = pooled.separate_many(paths)
    assert pooled.last_paths_taken == ["device"] * 3 and pooled.batch_errors == {}
    for g, w in zip(got_many, want):
        assert [os.path.basename(f) for f in g] == [os.path.basename(f) for f in w]
        for a, b in zip(g, w):
            assert filecmp.cmp(a, b, shallow=False), os.path.basename(a)
