"""asx_resample_rational_complement -- the complement form of the writer-side converter -- per launch against its definition:

    y = asx_resample_rational_stem_dev(x)                       (bit for bit)
    c = fl( fl(s * mix) - fl(k * y) )                           (bit for bit: tests/complement_ref.py, numpy float32)
    |c - (s mix - k ref64)| <= k * 1e-6 + 6 * 2^-24             (ref64: the float64 definition of tests/resample_ref.py)

1e-6 is tests/test_gpu_resample_stem.py's own bound on y; the remaining 6 * 2^-24 is three float32 roundings on magnitudes <= 1.65 + 1 +
2.65, for inputs in [-1, 1], k <= 1.1 and |y| <= 1.5 -- which the test asserts on its signals.

One float64 reference per (pair, n_in): eight channels at the plan's n_out; every case compares against a part of it."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import complement_ref as CR
from tests import resample_ref as RR
from tests.test_gpu_resample_stem import GUARD, lengths, run_dev
from tests.test_gpu_resample_stem import signal as unit_signal

pytestmark = pytest.mark.gpu

TOL_Y = 1e-6
PAIRS = [(44100, 48000), (44100, 96000), (44100, 22050), (48000, 44100)]
SCALES = [(1.0, 1.0), (0.8125, 1.035), (float(np.float32(0.9 / 1.37)), 1.0)]
LAYOUTS = (("planar", 1), ("planar", 2), ("planar", 8), ("rows", 2))


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


def signal(n, seed):
    """tests/test_gpu_resample_stem.py's [8, n] signals at 3/4 of full scale: the float64 reference of full-scale noise overshoots to 1.88 at
    these pairs (measured on the reference alone), and the rounding bound above is worked out for |y| <= 1.5"""
    return (unit_signal(n, seed) * np.float32(0.75)).astype(np.float32)


def mix_signal(ch, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (ch, n)).astype(np.float32)


def run_comp(eng, x, layout, sr_in, sr_out, n_out, mix, s, k, want_y=True):
    """One launch into NaN-filled buffers with GUARD floats before and after y and c: (y planar [C, n_out] or None, c, guards intact).
    ``mix`` [C, stride] is passed with its own row stride."""
    import torch
    dev = torch.device("cuda", eng.device)
    ch, n_in = x.shape if layout == "planar" else x.shape[::-1]
    assert mix.shape[0] == ch and mix.shape[1] >= n_out
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    md = torch.from_numpy(np.ascontiguousarray(mix)).to(dev)
    ybuf = torch.full((2 * GUARD + ch * n_out,), float("nan"), dtype=torch.float32, device=dev)
    cbuf = torch.full((2 * GUARD + ch * n_out,), float("nan"), dtype=torch.float32, device=dev)
    y_ptr = ybuf[GUARD:].data_ptr() if want_y else 0
    eng.resample_rational_complement_dev(xd.data_ptr(), layout, ch, n_in, sr_in, sr_out, md.data_ptr(), mix.shape[1], s, k, y_ptr,
                                         cbuf[GUARD:].data_ptr(), n_out, stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.current_stream(dev).synchronize()
    yh, ch_ = ybuf.cpu().numpy(), cbuf.cpu().numpy()
    ok = bool(np.isnan(ch_[:GUARD]).all() and np.isnan(ch_[-GUARD:]).all() and np.isnan(yh[:GUARD]).all() and np.isnan(yh[-GUARD:]).all())
    if not want_y:
        ok = ok and bool(np.isnan(yh).all())
    return (yh[GUARD:-GUARD].reshape(ch, n_out) if want_y else None), ch_[GUARD:-GUARD].reshape(ch, n_out), ok


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_launch_against_its_definition(eng, sr_in, sr_out):
    L, M, half, T, _ = RR.design(sr_in, sr_out)
    tile, edge, ns = lengths(sr_in, sr_out)
    worst = 0.0
    for n_in in ns:
        plan = RR.plan_n_out(n_in, L, M)
        x8 = signal(n_in, n_in * 7 + sr_out)
        ref8 = RR.reference(x8, sr_in, sr_out, plan)
        assert np.abs(ref8).max() <= 1.5
        mix8 = mix_signal(8, plan + 3, n_in * 13 + sr_out)
        for n_out in sorted({1, max(plan - 1, 1), plan}):
            for layout, ch in LAYOUTS:
                x = x8[:ch] if layout == "planar" else np.ascontiguousarray(x8[:ch].T)
                stem, guards_intact = run_dev(eng, x, layout, sr_in, sr_out, n_out)       # asx_resample_rational_stem_dev
                assert guards_intact and np.abs(stem).max() <= 1.5
                for extra, (s, k), want_y in itertools.product((0, 3), SCALES, (True, False)):
                    where = (sr_in, sr_out, n_in, n_out, layout, ch, extra, s, k, want_y)
                    mix = np.ascontiguousarray(mix8[:ch, :n_out + extra])
                    y, c, guards_intact = run_comp(eng, x, layout, sr_in, sr_out, n_out, mix, s, k, want_y)
                    assert guards_intact, where
                    assert c.shape == (ch, n_out) and not np.isnan(c).any(), where
                    if want_y:
                        np.testing.assert_array_equal(y, stem, err_msg=str(where))
                    np.testing.assert_array_equal(c, CR.complement_f32(mix[:, :n_out], stem, s, k), err_msg=str(where))
                    err = np.abs(c - CR.complement_f64(mix[:, :n_out], ref8[:ch, :n_out], s, k))
                    worst = max(worst, float(err.max()))
                    assert err.max() <= float(np.float32(k)) * TOL_Y + CR.ROUNDING_BOUND, (where, float(err.max()), int(err.argmax()))
    print(f"{sr_in} -> {sr_out}: max |c - float64| = {worst:.3e} over n_in {ns}")


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 48000), (44100, 22050)])
def test_runs_are_bit_identical_and_host_equals_dev(eng, sr_in, sr_out):
    tile, edge, _ = lengths(sr_in, sr_out)
    n_in = edge + 777
    L, M = RR.design(sr_in, sr_out)[:2]
    n_out = RR.plan_n_out(n_in, L, M)
    x = signal(n_in, 11)[:2]
    rows = np.ascontiguousarray(x.T)
    mix = mix_signal(2, n_out + 3, 5)
    s, k = SCALES[1]
    ya, ca, ok_a = run_comp(eng, rows, "rows", sr_in, sr_out, n_out, mix, s, k)
    yb, cb, ok_b = run_comp(eng, rows, "rows", sr_in, sr_out, n_out, mix, s, k)
    assert ok_a and ok_b
    np.testing.assert_array_equal(ya, yb)
    np.testing.assert_array_equal(ca, cb)
    _, c_only, ok_c = run_comp(eng, rows, "rows", sr_in, sr_out, n_out, mix, s, k, want_y=False)
    assert ok_c
    np.testing.assert_array_equal(c_only, ca)
    yh, chost = eng.resample_rational_complement(rows, sr_in, sr_out, n_out, mix, s, k, layout="rows")
    assert yh.shape == chost.shape == (2, n_out) and yh.dtype == chost.dtype == np.float32
    np.testing.assert_array_equal(yh, ya)
    np.testing.assert_array_equal(chost, ca)
    none, c2 = eng.resample_rational_complement(x, sr_in, sr_out, n_out, mix, s, k, want_stem=False)
    assert none is None
    np.testing.assert_array_equal(c2, ca)
    np.testing.assert_array_equal(yh, eng.resample_rational_stem(rows, sr_in, sr_out, n_out, layout="rows"))


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 48000), (48000, 44100)])
def test_a_tile_wholly_past_the_input_gives_the_scaled_mix(eng, sr_in, sr_out):
    L, M, half, T, _ = RR.design(sr_in, sr_out)
    tile, edge, _ = lengths(sr_in, sr_out)
    n_in = edge
    plan = RR.plan_n_out(n_in, L, M)
    # (tests/test_gpu_resample_stem.py) the last of the three tiles of ``longest`` lies wholly past the input
    assert plan == tile and (2 * tile) // L * M - half // L >= n_in
    longest = plan + tile + 1
    x = signal(n_in, 3)[:2]
    mix = mix_signal(2, longest + 3, 9)
    stem, _ = run_dev(eng, x, "planar", sr_in, sr_out, longest)
    assert not stem[:, 2 * tile:].any()
    for (s, k), want_y in itertools.product(SCALES, (True, False)):
        y, c, ok = run_comp(eng, x, "planar", sr_in, sr_out, longest, mix, s, k, want_y)
        assert ok
        if want_y:
            np.testing.assert_array_equal(y, stem)
        np.testing.assert_array_equal(c[:, 2 * tile:], np.float32(s) * mix[:, 2 * tile:longest])
        np.testing.assert_array_equal(c, CR.complement_f32(mix[:, :longest], stem, s, k))


def test_every_refusal_names_its_argument_and_leaves_y_and_c_untouched(eng):
    import torch
    import audio_separator_amd as A
    dev = torch.device("cuda", eng.device)
    n_in, n_out = 1000, 1089
    xd = torch.zeros((2, n_in), dtype=torch.float32, device=dev)
    md = torch.zeros((2, n_out + 3), dtype=torch.float32, device=dev)
    yd = torch.full((2, n_out + 8), float("nan"), dtype=torch.float32, device=dev)
    cd = torch.full((2, n_out + 8), float("nan"), dtype=torch.float32, device=dev)
    lib, h = eng._lib, eng._h
    x, mix, y, c = xd.data_ptr(), md.data_ptr(), yd.data_ptr(), cd.data_ptr()
    big = (1 << 40) + 1
    st = n_out + 3
    inf, nan = float("inf"), float("nan")
    cases = [  # (x, layout, channels, n_in, sr_in, sr_out, mix, mix_stride, mix_scale, stem_scale, y, c, n_out), what the message names
        ((None, 0, 2, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), "x is null"),
        ((x, 0, 2, n_in, 44100, 48000, None, st, 1.0, 1.0, y, c, n_out), "mix is null"),
        ((x, 0, 2, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, None, n_out), "c is null"),
        ((x, 2, 2, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), "layout = 2"),
        ((x, -1, 2, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), "layout = -1"),
        ((x, 0, 0, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), "0 channels"),
        ((x, 1, 65536, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), "65536 channels"),
        ((x, 0, 2, 0, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), "n_in = 0"),
        ((x, 0, 2, big, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out), f"n_in = {big}"),
        ((x, 0, 2, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, 0), "n_out = 0"),
        ((x, 1, 2, n_in, 44100, 48000, mix, big, 1.0, 1.0, y, c, big), f"n_out = {big}"),
        ((x, 0, 2, n_in, 44100, 44100, mix, st, 1.0, 1.0, y, c, n_out), "equal"),
        ((x, 0, 2, n_in, 44100, 44056, mix, st, 1.0, 1.0, y, c, n_out), "2^20"),
        ((x, 0, 2, n_in, 0, 48000, mix, st, 1.0, 1.0, y, c, n_out), "sample rates"),
        ((x, 0, 2, n_in, 44100, 48000, mix, n_out - 1, 1.0, 1.0, y, c, n_out), f"mix_stride = {n_out - 1}"),
        ((x, 0, 2, n_in, 44100, 48000, mix, 0, 1.0, 1.0, None, c, n_out), "mix_stride = 0"),
        ((x, 0, 2, n_in, 44100, 48000, mix, st, inf, 1.0, y, c, n_out), "mix_scale"),
        ((x, 0, 2, n_in, 44100, 48000, mix, st, nan, 1.0, y, c, n_out), "mix_scale"),
        ((x, 0, 2, n_in, 44100, 48000, mix, st, 1.0, -inf, y, c, n_out), "stem_scale"),
        ((x, 0, 2, n_in, 44100, 48000, mix, st, 1.0, nan, None, c, n_out), "stem_scale"),
    ]
    for (cx, layout, ch, ni, a, b, cm, ms, s, k, cy, cc, no), text in cases:
        rc = lib.asx_resample_rational_complement_dev(h, cx, layout, ch, ni, a, b, cm, ms, s, k, cy, cc, no, None)
        msg = lib.asx_last_error().decode()
        assert rc == 1, (text, rc)                                              # ASX_ERR_INVALID
        assert msg.startswith("asx_resample_rational_complement_dev: ") and text in msg, (text, msg)
    assert lib.asx_resample_rational_complement_dev(None, x, 0, 2, n_in, 44100, 48000, mix, st, 1.0, 1.0, y, c, n_out, None) == 1
    assert "null engine" in lib.asx_last_error().decode()
    torch.cuda.synchronize(dev)
    assert torch.isnan(yd).all() and torch.isnan(cd).all()
    # the host-array entry checks the same before it stages anything
    xh, mh = np.zeros((2, n_in), np.float32), np.zeros((2, st), np.float32)
    yh, chh = np.full((2, n_out), np.nan, np.float32), np.full((2, n_out), np.nan, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    for (cx, layout, ch, ni, a, b, cm, ms, s, k, cy, cc, no), text in cases:
        rc = lib.asx_resample_rational_complement(h, fp(xh) if cx else None, layout, ch, ni, a, b, fp(mh) if cm else None, ms, s, k,
                                                  fp(yh) if cy else None, fp(chh) if cc else None, no)
        msg = lib.asx_last_error().decode()
        assert rc == 1 and msg.startswith("asx_resample_rational_complement: ") and text in msg, (text, rc, msg)
    assert np.isnan(yh).all() and np.isnan(chh).all()
    # ... and the binding
    with pytest.raises(ValueError, match="layout"):
        eng.resample_rational_complement(xh, 44100, 48000, n_out, mh, layout="columns")
    with pytest.raises(ValueError, match="mix"):
        eng.resample_rational_complement(xh, 44100, 48000, n_out, mh[:1])
    with pytest.raises(A.AsxError, match="mix_stride"):
        eng.resample_rational_complement(xh, 44100, 48000, n_out, mh[:, :n_out - 1])
    with pytest.raises(A.AsxError, match="equal"):
        eng.resample_rational_complement(xh, 44100, 44100, n_out, mh)


def test_normalize_scale_is_the_factor_normalize_applies(eng):
    """asx_normalize_scale_dev: the factor of the mix normalise, without bringing the mix to the host"""
    import torch
    dev = torch.device("cuda", eng.device)
    st = torch.cuda.current_stream(dev).cuda_stream
    x = np.random.default_rng(2).uniform(-1.0, 1.0, (2, 5001)).astype(np.float32)
    for gain, thr, amp in ((1.37, 0.9, 0.0), (0.5, 0.9, 0.0), (0.5, 0.9, None), (0.1, 0.9, 0.25), (0.9 / np.abs(x).max(), 0.9, 0.0)):
        a = (x * np.float32(gain)).astype(np.float32)
        d = torch.from_numpy(a).to(dev)
        s = eng.normalize_scale_dev(d.data_ptr(), a.size, thr, amp, stream=st)
        np.testing.assert_array_equal(d.cpu().numpy(), a)                     # only read
        peak = np.abs(a).max()
        want = np.float32(thr) / peak if peak > np.float32(thr) else (np.float32(amp) / peak if amp is not None and peak < np.float32(amp)
                                                                       else np.float32(1.0))
        assert np.float32(s) == np.float32(want), (gain, thr, amp, s, want)
        eng.normalize_dev(d.data_ptr(), a.size, thr, amp, stream=st)
        torch.cuda.current_stream(dev).synchronize()
        np.testing.assert_array_equal(d.cpu().numpy(), a * np.float32(s) if s != 1.0 else a)


def test_normalize_scale_refusals_name_their_argument(eng):
    import torch
    dev = torch.device("cuda", eng.device)
    d = torch.zeros(64, dtype=torch.float32, device=dev)
    lib, h = eng._lib, eng._h
    q = C.c_float(7.0)
    cases = [((None, d.data_ptr(), 64, 0.9, 0.0, 0, C.byref(q)), "null engine"), ((h, None, 64, 0.9, 0.0, 0, C.byref(q)), "wave is null"),
             ((h, d.data_ptr(), 64, 0.9, 0.0, 0, None), "scale is null"), ((h, d.data_ptr(), 0, 0.9, 0.0, 0, C.byref(q)), "numel = 0"),
             ((h, d.data_ptr(), 64, float("nan"), 0.0, 0, C.byref(q)), "threshold"),
             ((h, d.data_ptr(), 64, 0.9, 0.25, 1, C.byref(q)), "silent")]          # min_peak / 0
    for args, text in cases:
        assert lib.asx_normalize_scale_dev(*args, None) == 1, text
        msg = lib.asx_last_error().decode()
        assert msg.startswith("asx_normalize_scale_dev: ") and text in msg, (text, msg)
    assert q.value == 7.0
    assert eng.normalize_scale_dev(d.data_ptr(), 64, 0.9, None) == 1.0           # silent, no minimum: left alone
