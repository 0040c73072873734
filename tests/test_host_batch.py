"""CPU side of the batch entry points: FilesPipeline's ``demix_many`` hook over the CPU test double of the engine (world 1 and
gloo world 2), the Python-level shape / dtype refusals of the batch methods, and the C boundary -- include/asx.h declares
asx_demix_batch_dev / asx_separate_batch_dev and engine.py binds them with matching argument counts and struct layouts -- and
``MDXSeparator.separate_many`` over the same double (the batch shell of CommonSeparator on host arrays)."""
import ctypes as C
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import mdx_oracle as O
from tests.fake_engine import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = O.NetDims(dim_c=4, dim_f=32, dim_t=16, g=8, l=2, num_blocks=5, k=3, bn=4)
N, SONGS, STEPS = 1500, 3, 3


def _fake_engine():
    import audio_separator_amd as A
    eng = OracleEngine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16, overlap=0.25))
    eng.load_net(A.NetConfig(dim_f=32, dim_t=16, g=8, l=2, num_blocks=5, bn=4),
                 A.fold_convtdf_state(O.make_convtdf_state(DIMS, seed=3), DIMS.num_blocks, DIMS.l))
    return eng


def _mixes(rank):
    return [torch.from_numpy((0.4 * np.random.default_rng(10 * rank + s).standard_normal((2, N))).astype(np.float32)) for s in range(SONGS)]


def _run_pipeline(world, rank, use_dist, many):
    """STEPS steps of FilesPipeline over the fake engine; returns ({step: [slab per rank]} on rank 0, calls made)"""
    from audio_separator_amd.sharding import FilesPipeline
    eng = _fake_engine()
    calls = {"one": 0, "many": 0}

    def demix(mix, out):
        calls["one"] += 1
        out.copy_(torch.from_numpy(np.ascontiguousarray(eng.demix(mix.numpy()))))

    def demix_many(mixes, outs):
        calls["many"] += 1
        assert tuple(outs.shape) == (len(mixes), 2, N)
        for s, mix in enumerate(mixes):
            outs[s].copy_(torch.from_numpy(np.ascontiguousarray(eng.demix(mix.numpy()))))

    got = {}
    pipe = FilesPipeline(demix, _mixes(rank), world, rank, use_dist, on_gathered=lambda k, slabs: got.__setitem__(k, [s.clone() for s in slabs]),
                         demix_many=demix_many if many else None)
    local = {}
    for k in range(STEPS):
        pipe.step(k)
        local[k] = pipe.outs[k & 1].clone()
    pipe.drain()
    return (got if use_dist else {k: [v] for k, v in local.items()}), calls


def test_files_pipeline_demix_many_world_1():
    loop, c0 = _run_pipeline(1, 0, False, many=False)
    pooled, c1 = _run_pipeline(1, 0, False, many=True)
    assert c0 == {"one": SONGS * STEPS, "many": 0} and c1 == {"one": 0, "many": STEPS}      # one call per step in place of the loop
    assert sorted(loop) == sorted(pooled) == list(range(STEPS))
    for k in loop:
        assert torch.equal(loop[k][0], pooled[k][0])
    assert float(loop[0][0].abs().max()) > 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, many, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    got, calls = _run_pipeline(world, rank, True, many)
    if rank == 0:
        q.put(({k: [s.numpy() for s in v] for k, v in got.items()}, calls))
    dist.barrier()
    dist.destroy_process_group()


def _gloo(many):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, many, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    return res


def test_files_pipeline_demix_many_gloo_world_2():
    loop, c0 = _gloo(False)
    pooled, c1 = _gloo(True)
    assert c0 == {"one": SONGS * STEPS, "many": 0} and c1 == {"one": 0, "many": STEPS}
    assert sorted(loop) == sorted(pooled) == list(range(STEPS))
    for k in loop:
        assert len(loop[k]) == len(pooled[k]) == 2
        for a, b in zip(loop[k], pooled[k]):
            assert a.shape == (SONGS, 2, N) and np.array_equal(a, b)
    assert not np.array_equal(loop[0][0], loop[0][1])                  # the two ranks hold different songs


def test_demixer_batch_refusals(monkeypatch):
    """MDXDemixer.demix_many / separate_stems_many refuse what demix / separate_stems refuse, before the engine is called"""
    from tests import fake_engine
    fake_engine.install(monkeypatch)
    import audio_separator_amd as A
    dm = A.MDXDemixer({"model_data": {"compensate": 1.035, "mdx_dim_f_set": 32, "mdx_dim_t_set": 4, "mdx_n_fft_scale_set": 96}},
                      {"hop_length": 16, "segment_size": 16, "overlap": 0.25, "enable_denoise": False},
                      state_dict=O.make_convtdf_state(DIMS, seed=3), net_config=A.NetConfig(dim_f=32, dim_t=16, g=8, l=2, num_blocks=5, bn=4))
    ok = np.zeros((2, 100), np.float32)
    for fn in (dm.demix_many, dm.separate_stems_many):
        with pytest.raises(ValueError, match="2-channel"):
            fn([ok, np.zeros((3, 100), np.float32)])
        with pytest.raises(ValueError, match="2-channel"):
            fn([np.zeros(100, np.float32)])
        with pytest.raises(ValueError, match="empty or not valid"):
            fn([ok, np.zeros((2, 0), np.float32)])


def test_engine_batch_refusals_come_before_the_device():
    """Engine.demix_batch / separate_batch make the shape / dtype checks of demix / separate; they need no engine handle"""
    from audio_separator_amd.engine import Engine
    eng = Engine.__new__(Engine)                                       # no library, no GPU: the checks run first
    with pytest.raises(ValueError, match="2-channel"):
        eng.demix_batch([np.zeros((2, 10), np.float32), np.zeros((1, 10), np.float32)])
    for bad in (np.zeros((2, 10), np.float64), np.zeros((10, 2), np.float32), np.zeros((2, 20), np.float32)[:, ::2], [[0.0] * 4] * 2):
        with pytest.raises(ValueError, match="C-contiguous float32"):
            eng.separate_batch([np.zeros((2, 10), np.float32), bad], 0.9, None, 1.0)
    assert eng.demix_batch([]) == [] and eng.separate_batch([], 0.9, None, 1.0) == []


def test_header_declares_and_binding_matches():
    import __graft_entry__ as entry
    from audio_separator_amd import engine as E
    entry.build()
    lib = E.load_library()
    hdr = open(os.path.join(ROOT, "include", "asx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("asx_demix_batch_dev", "asx_separate_batch_dev"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/asx.h"
        assert len(m.group(1).split(",")) == len(getattr(lib, name).argtypes), name
        assert name in E.SYMBOLS and getattr(lib, name).restype is C.c_int
    for struct, mirror in (("asx_song", E._Song), ("asx_song_stems", E._SongStems)):
        m = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{([^}]*)\}\s*" + struct + r"\s*;", hdr)
        assert m, struct
        fields = [re.sub(r"[\s\*]", " ", f).split()[-1] for f in m.group(1).split(";") if f.strip()]
        assert fields == [n for n, _ in mirror._fields_], (struct, fields)
        assert C.sizeof(mirror) == 8 * len(fields)
    assert lib.asx_abi_version() == 8
    # the entry points validate before they touch the engine
    assert lib.asx_demix_batch_dev(None, None, 0, 0, None) != 0 and lib.asx_separate_batch_dev(None, None, 0, 0.9, 0.0, 0, 1.0, None) != 0


def test_separate_many_through_the_mdx_plugin(tmp_path, monkeypatch):
    """The batch shell of CommonSeparator through MDXSeparator over the engine double (tests/test_host_demucs_batch.py drives it
    through DemucsSeparator): ``invert_using_spec`` keeps every array on the host.  A bad file fails alone, the files equal
    those of ``separate`` per path byte for byte, and an exception out of the pooled call leaves no write pending."""
    import filecmp
    import threading
    from tests import fake_engine
    from tests import separate_cases as SC
    from audio_separator_amd import audio_io
    fake_engine.install(monkeypatch)
    monkeypatch.setenv("ASX_ASYNC_WRITES", "0")
    _, cls, common, arch, _, _ = SC.cases("mdx", str(tmp_path))[0]
    wavs = []
    for i, n in enumerate((4000, 6100, 2500)):
        p = str(tmp_path / f"in{i}.wav")
        x = (0.3 * np.random.default_rng(40 + i).standard_normal((n, 2))).astype(np.float32)
        audio_io.write_wav(p, np.clip(x, -0.99, 0.99), common["sample_rate"], "PCM_16")
        wavs.append(p)
    bad = str(tmp_path / "broken.wav")
    with open(bad, "w") as f:
        f.write("not audio")
    paths = [wavs[0], bad, wavs[1], str(tmp_path / "missing.wav"), wavs[2]]

    def make(out_dir):
        return SC.plugin_class(cls)(common_config=dict(common, output_dir=out_dir, invert_using_spec=True), arch_config=arch)
    one_dir, many_dir = str(tmp_path / "one"), str(tmp_path / "many")
    sep = make(one_dir)
    want = []
    for p in wavs:
        want.append(sep.separate(p))
        sep.clear_file_specific_paths()
    sep = make(many_dir)
    got = sep.separate_many(paths)
    assert got[1] == [] and got[3] == [] and sorted(sep.batch_errors) == [1, 3]
    assert all(isinstance(e, Exception) for e in sep.batch_errors.values())
    assert [got[0], got[2], got[4]] == want and all(len(names) == 2 for names in want)
    for names in want:
        for name in names:
            assert filecmp.cmp(os.path.join(one_dir, name), os.path.join(many_dir, name), shallow=False), name
    assert sep.separate_many([bad]) == [[]] and list(sep.batch_errors) == [0]
    assert sep.audio_file_path is None and sep.primary_source is None          # nothing loaded: the file state is reset

    # an exception out of the pooled call is the caller's; a write that was in flight is joined and its own error only logged
    def boom(mixes):
        raise RuntimeError("pooled call failed")
    monkeypatch.setattr(sep, "_pooled_stems", boom)
    writer = threading.Thread(target=lambda: None)
    writer.start()
    sep._pending_writes.append((writer, [OSError("disk full")]))
    with pytest.raises(RuntimeError, match="pooled call failed"):
        sep.separate_many(wavs[:2])
    assert sep._pending_writes == [] and not writer.is_alive() and sep._in_separate is False
    assert sep.batch_errors == {}
