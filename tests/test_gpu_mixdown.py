"""asx_mixdown_batch_dev / asx_mixdown (csrc/kernels_mix.h) against tests/mixdown_ref.py, bit for bit: every length at which the kernel
takes another path (a head or tail group, a single whole group, more than one workgroup), K = 1, 2 and 8, rows and planar sources mixed
in one job, both output layouts, sources shorter than the output (one of length 0, one longer than it), weights 0 and negative, and
pointers one float off the 16-byte grid -- the scalar path.  Every output buffer carries guard floats in front and behind."""
import numpy as np
import pytest

from tests.mixdown_ref import mixdown_ref

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 63, 64, 65, 4099]
GUARD = 8


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=64, hop_length=16, dim_f=32, segment_size=8))
    yield e
    e.close()


def sources_for(rng, k, n_out):
    """[(array, layout, weight)]: lengths n_out, n_out - 1, 0, n_out // 2, n_out + 3, ...; weights with a zero and negatives"""
    lengths = [n_out, max(n_out - 1, 0), 0, n_out // 2, n_out + 3, n_out, 1, max(n_out - 2, 0)]
    weights = [1.0, -0.75, 0.0, 1.5, -2.0, 0.3333, 0.0, -1.0]
    out = []
    for i in range(k):
        n = lengths[i] if k > 1 else n_out
        layout = "rows" if i % 2 else "planar"
        a = rng.standard_normal((n, 2) if layout == "rows" else (2, n)).astype(np.float32)
        out.append((a, layout, np.float32(weights[i] if k > 1 else -0.6)))
    return out


class Placed:
    """arrays on the device at a chosen offset (in floats) from a 16-byte boundary, outputs between guards"""

    def __init__(self):
        import torch
        self.torch, self.keep = torch, []

    def put(self, a, offset):
        t = self.torch.zeros(a.size + 4 + offset, dtype=self.torch.float32, device="cuda")
        assert t.data_ptr() % 16 == 0
        view = t[offset: offset + a.size]
        if a.size:
            view.copy_(self.torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
        self.keep.append(t)
        return view.data_ptr() if a.size else 0

    def out(self, n_out, offset):
        t = self.torch.full((GUARD + offset + 2 * n_out + GUARD,), float("nan"), dtype=self.torch.float32, device="cuda")
        assert t.data_ptr() % 16 == 0
        self.keep.append(t)
        return t, GUARD + offset

    @staticmethod
    def result(t, start, n_out, layout):
        h = t.cpu().numpy()
        assert np.isnan(h[:start]).all() and np.isnan(h[start + 2 * n_out:]).all(), "the kernel wrote outside its output"
        body = h[start: start + 2 * n_out]
        return body.reshape(2, n_out) if layout == "planar" else body.reshape(n_out, 2)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n_out", LENGTHS)
def test_kernel_equals_the_numpy_restatement(eng, n_out):
    import torch
    rng = np.random.default_rng(100 + n_out)
    for k in (1, 2, 8):
        srcs = sources_for(rng, k, n_out)
        for out_layout in ("planar", "rows"):
            want = mixdown_ref(srcs, n_out, out_layout)
            # (source offset, output offset) in floats: all aligned; sources off by one; output off by one; both; output off by two
            for s_off, o_off in ((0, 0), (1, 0), (0, 1), (1, 1), (0, 2)):
                p = Placed()
                job_src = [(p.put(a, s_off if i % 2 == 0 else 0), layout, a.shape[0 if layout == "rows" else 1], w) for i, (a, layout, w) in enumerate(srcs)]
                t, start = p.out(n_out, o_off)
                eng.mixdown_batch_dev([(job_src, t.data_ptr() + 4 * start, out_layout, n_out)], stream=torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                got = p.result(t, start, n_out, out_layout)
                assert np.array_equal(bits(got), bits(want)), (n_out, k, out_layout, s_off, o_off)


def test_three_jobs_in_one_call_and_two_runs(eng):
    import torch
    specs = [(4099, 8, "planar", 1), (65, 2, "rows", 0), (3, 1, "planar", 0)]
    runs = []
    for _ in range(2):
        p, jobs, outs = Placed(), [], []
        for n_out, k, layout, off in specs:
            srcs = sources_for(np.random.default_rng(n_out), k, n_out)
            t, start = p.out(n_out, off)
            jobs.append(([(p.put(a, off), lay, a.shape[0 if lay == "rows" else 1], w) for a, lay, w in srcs], t.data_ptr() + 4 * start, layout, n_out))
            outs.append((t, start, n_out, layout, mixdown_ref(srcs, n_out, layout)))
        eng.profile_enable(True)
        eng.mixdown_batch_dev(jobs, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        launches = sum(v["launches"] for v in eng.profile_read().values() if isinstance(v, dict) and "launches" in v)
        eng.profile_enable(False)
        assert launches == 1, launches                           # one launch for all jobs
        got = [p.result(t, start, n_out, layout) for t, start, n_out, layout, _ in outs]
        for g, (_, _, n_out, layout, want) in zip(got, outs):
            assert np.array_equal(bits(g), bits(want)), (n_out, layout)
        runs.append(got)
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b))


def test_host_call_and_refusals(eng):
    from audio_separator_amd import AsxError
    rng = np.random.default_rng(9)
    srcs = sources_for(rng, 8, 65)
    for layout in ("planar", "rows"):
        got = eng.mixdown(srcs, 65, layout)
        assert np.array_equal(bits(got), bits(mixdown_ref(srcs, 65, layout)))
    a = rng.standard_normal((2, 10)).astype(np.float32)
    assert eng.mixdown([(a, "planar", 2.0)]).shape == (2, 10)    # n_out: the longest source
    eng.mixdown_batch_dev([])                                    # no job: nothing to do
    with pytest.raises(ValueError, match="1 .. 8 sources"):
        eng.mixdown([(a, "planar", 1.0)] * 9)
    with pytest.raises(AsxError, match="n_out = 0"):
        eng.mixdown_batch_dev([([(0, "planar", 0, 1.0)], 16, "planar", 0)])
    with pytest.raises(AsxError, match="source 0 is null with n = 5"):
        eng.mixdown_batch_dev([([(0, "planar", 5, 1.0)], 16, "planar", 5)])
    with pytest.raises(AsxError, match="not finite"):
        eng.mixdown_batch_dev([([(16, "planar", 5, float("nan"))], 16, "planar", 5)])
