"""asx_resample_rational_stem -- the writer-side form of the rational polyphase converter: planar or rows input, the caller's n_out --
per launch against the float64 definition (tests/resample_ref.py).

Bound: 1e-6 max abs on inputs in [-1, 1], the bound and the reasoning of tests/test_gpu_resample.py (a float32 dot product with float32
taps differs from float64 by <= 2.5e-7 on unit signals; 4x for the kernel's summation order).  Outputs from ``zero_from`` on -- the
filter has left the input -- are exact zeros.

One float64 reference per (pair, n_in): eight channels at the longest n_out; every n_out, channel count and layout of the case compares
against a part of it."""
import ctypes as C

import numpy as np
import pytest

from tests import resample_ref as RR

pytestmark = pytest.mark.gpu

TOL = 1e-6
PAIRS = [(44100, 48000), (44100, 96000), (44100, 88200), (44100, 22050), (44100, 32000), (48000, 44100)]
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


def lengths(sr_in, sr_out):
    L, M, _, T, _ = RR.design(sr_in, sr_out)
    tile = RR.tile_outputs(L, M, T)
    edge = -(-tile * M // L)              # the shortest input that fills one tile of outputs
    return tile, edge, sorted({1, 2, T - 1, edge - 1, edge, edge + 1})


def signal(n, seed):
    """[8, n] float32 in [-1, 1]: noise, but a sine near the band edge in channels 1 and 5"""
    x = np.random.default_rng(seed).uniform(-1.0, 1.0, (8, n)).astype(np.float32)
    i = np.arange(n, dtype=np.float64)
    x[1] = np.sin(0.83 * np.pi * 0.45 * i + 0.4)
    x[5] = np.sin(0.31 * np.pi * 0.45 * i + 2.1)
    return x


def run_dev(eng, x, layout, sr_in, sr_out, n_out):
    """One launch into a NaN-filled buffer with GUARD floats before and after y: (y planar [C, n_out], the guards are untouched)."""
    import torch
    dev = torch.device("cuda", eng.device)
    ch, n_in = x.shape if layout == "planar" else x.shape[::-1]
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    buf = torch.full((2 * GUARD + ch * n_out,), float("nan"), dtype=torch.float32, device=dev)
    y = buf[GUARD:GUARD + ch * n_out]
    eng.resample_rational_stem_dev(xd.data_ptr(), layout, ch, n_in, sr_in, sr_out, y.data_ptr(), n_out,
                                   stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.current_stream(dev).synchronize()
    host = buf.cpu().numpy()
    return host[GUARD:-GUARD].reshape(ch, n_out), bool(np.isnan(host[:GUARD]).all() and np.isnan(host[-GUARD:]).all())


@pytest.mark.parametrize("sr_in,sr_out", PAIRS)
def test_against_float64_definition(eng, sr_in, sr_out):
    L, M, half, T, _ = RR.design(sr_in, sr_out)
    assert eng.resample_rational_plan(sr_in, sr_out, 1)[1:] == (L, M, T)
    tile, edge, ns = lengths(sr_in, sr_out)
    worst = 0.0
    for n_in in ns:
        plan = RR.plan_n_out(n_in, L, M)
        zero = RR.zero_from(n_in, L, M, half)
        longest = plan + tile + 1
        x8 = signal(n_in, n_in * 7 + sr_out)
        ref8 = RR.reference(x8, sr_in, sr_out, longest)
        assert zero <= plan + T * max(L, M) // M + 2 and not ref8[:, zero:].any()
        if n_in == edge:
            # the last of the three tiles of ``longest`` lies wholly past the input: its span starts at or after n_in
            assert plan == tile and (2 * tile) // L * M - half // L >= n_in
        at_plan = eng.resample_rational(x8, sr_in, sr_out)                       # asx_resample_rational_dev, n_out = the plan's
        for n_out in sorted({1, max(plan - 1, 1), plan, plan + 3, longest}):
            for layout, ch in (("planar", 1), ("planar", 2), ("planar", 8), ("rows", 2)):
                x = x8[:ch] if layout == "planar" else np.ascontiguousarray(x8[:ch].T)
                got, guards_intact = run_dev(eng, x, layout, sr_in, sr_out, n_out)
                where = (sr_in, sr_out, n_in, n_out, layout, ch)
                assert guards_intact, where
                assert got.shape == (ch, n_out) and not np.isnan(got).any(), where
                err = np.abs(got - ref8[:ch, :n_out])
                worst = max(worst, float(err.max()))
                assert err.max() <= TOL, (where, float(err.max()), int(err.argmax()))
                assert not got[:, zero:].any(), where                            # exact zeros once the filter has left the input
                # the bits of the input-side entry wherever both compute the output
                k = min(n_out, plan)
                np.testing.assert_array_equal(got[:, :k], at_plan[:ch, :k], err_msg=str(where))
                if layout == "rows":                                             # rows == planar of the transposed data
                    planar, _ = run_dev(eng, x8[:ch], "planar", sr_in, sr_out, n_out)
                    np.testing.assert_array_equal(got, planar, err_msg=str(where))
    print(f"{sr_in} -> {sr_out}: max |kernel - float64| = {worst:.3e} over n_in {ns}")


@pytest.mark.parametrize("sr_in,sr_out", [(44100, 48000), (44100, 88200)])
def test_runs_are_bit_identical_and_host_equals_dev(eng, sr_in, sr_out):
    tile, edge, _ = lengths(sr_in, sr_out)
    n_in = edge + 777
    L, M = RR.design(sr_in, sr_out)[:2]
    n_out = RR.plan_n_out(n_in, L, M) + 5
    x = signal(n_in, 11)[:2]
    rows = np.ascontiguousarray(x.T)
    a, ok_a = run_dev(eng, rows, "rows", sr_in, sr_out, n_out)
    b, ok_b = run_dev(eng, rows, "rows", sr_in, sr_out, n_out)
    assert ok_a and ok_b
    np.testing.assert_array_equal(a, b)
    host = eng.resample_rational_stem(rows, sr_in, sr_out, n_out, layout="rows")
    assert host.shape == (2, n_out) and host.dtype == np.float32
    np.testing.assert_array_equal(host, a)
    np.testing.assert_array_equal(eng.resample_rational_stem(x, sr_in, sr_out, n_out), a)
    # a stem tensor [S, 2, N] in one launch (channels = 2 S) is its stems one by one
    stems = signal(n_in, 12).reshape(4, 2, n_in)
    all_at_once = eng.resample_rational_stem(stems.reshape(8, n_in), sr_in, sr_out, n_out).reshape(4, 2, n_out)
    for s in range(4):
        np.testing.assert_array_equal(all_at_once[s], eng.resample_rational_stem(stems[s], sr_in, sr_out, n_out))
    mono = eng.resample_rational_stem(x[0], sr_in, sr_out, n_out)
    assert mono.shape == (n_out,)
    np.testing.assert_array_equal(mono, a[0])


def test_every_refusal_names_its_argument_and_leaves_y_untouched(eng):
    import torch
    import audio_separator_amd as A
    dev = torch.device("cuda", eng.device)
    n_in, n_out = 1000, 1089
    xd = torch.zeros((2, n_in), dtype=torch.float32, device=dev)
    yd = torch.full((2, n_out + 8), float("nan"), dtype=torch.float32, device=dev)
    lib, h = eng._lib, eng._h
    x, y = xd.data_ptr(), yd.data_ptr()
    big = (1 << 40) + 1
    cases = [  # (x, layout, channels, n_in, sr_in, sr_out, y, n_out), what the message names
        ((None, 0, 2, n_in, 44100, 48000, y, n_out), "x is null"),
        ((x, 0, 2, n_in, 44100, 48000, None, n_out), "y is null"),
        ((x, 2, 2, n_in, 44100, 48000, y, n_out), "layout = 2"),
        ((x, -1, 2, n_in, 44100, 48000, y, n_out), "layout = -1"),
        ((x, 0, 0, n_in, 44100, 48000, y, n_out), "0 channels"),
        ((x, 1, 65536, n_in, 44100, 48000, y, n_out), "65536 channels"),
        ((x, 0, 2, 0, 44100, 48000, y, n_out), "n_in = 0"),
        ((x, 0, 2, big, 44100, 48000, y, n_out), f"n_in = {big}"),
        ((x, 0, 2, n_in, 44100, 48000, y, 0), "n_out = 0"),
        ((x, 1, 2, n_in, 44100, 48000, y, big), f"n_out = {big}"),
        ((x, 0, 2, n_in, 44100, 44100, y, n_out), "equal"),
        ((x, 0, 2, n_in, 44100, 44056, y, n_out), "2^20"),
        ((x, 0, 2, n_in, 0, 48000, y, n_out), "sample rates"),
    ]
    for (cx, layout, ch, ni, a, b, cy, no), text in cases:
        rc = lib.asx_resample_rational_stem_dev(h, cx, layout, ch, ni, a, b, cy, no, None)
        msg = lib.asx_last_error().decode()
        assert rc == 1, (text, rc)                                              # ASX_ERR_INVALID
        assert msg.startswith("asx_resample_rational_stem_dev: ") and text in msg, (text, msg)
    assert lib.asx_resample_rational_stem_dev(None, x, 0, 2, n_in, 44100, 48000, y, n_out, None) == 1
    assert "null engine" in lib.asx_last_error().decode()
    torch.cuda.synchronize(dev)
    assert torch.isnan(yd).all()
    # the host-array entry checks the same before it stages anything
    xh, yh = np.zeros((2, n_in), np.float32), np.full((2, n_out), np.nan, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    for (cx, layout, ch, ni, a, b, cy, no), text in cases:
        rc = lib.asx_resample_rational_stem(h, fp(xh) if cx else None, layout, ch, ni, a, b, fp(yh) if cy else None, no)
        msg = lib.asx_last_error().decode()
        assert rc == 1 and msg.startswith("asx_resample_rational_stem: ") and text in msg, (text, rc, msg)
    assert np.isnan(yh).all()
    # ... and the binding
    with pytest.raises(ValueError, match="layout"):
        eng.resample_rational_stem(xh, 44100, 48000, n_out, layout="columns")
    with pytest.raises(A.AsxError, match="n_out = 0"):
        eng.resample_rational_stem(xh, 44100, 48000, 0)
    with pytest.raises(A.AsxError, match="equal"):
        eng.resample_rational_stem(xh, 44100, 44100, n_out)
