"""The recurrent kernels against float64, one launch (or one chain of step launches) at a time through asx_op_hd_lstm_layer /
asx_op_hd_lstm_frames / asx_op_vr_lstm / asx_op_vr_lstm_layout -- the engines' own launch code (hd_lstm_recurrence in
csrc/engine_hd.h, vr51_lstm in csrc/engine_vr.h): hd_lstm_step_kernel, hd_lstm_frame_kernel, hd_lstm_unframe_kernel of the
HDemucs / Demucs v3 BLSTM and vr_lstm_seq_kernel<HS>, vr_lstm_in_kernel, vr_lstm_out_kernel of the VR 5.1 LSTMModule.

Error measure: worst element |kernel - float64| over the whole output (|h| < 1), NaN counting as infinite -- every output goes in
filled with NaN, so an element the kernel never wrote fails the bar.
Bar: MARGIN = 8 x max(e32, 2^-23), e32 being the worst-element error of the plain fp32 numpy evaluation of the same recurrence on
the same input (tests/lstm_ref.py, computed here at run time) and 2^-23 one fp32 ulp at 1.  The factor covers what the kernel may do
differently from that evaluation: the summation order of the 4-wave K split and the device expf / tanhf (three to four chained
per step, a couple of ulp each).  Nothing in it comes from the kernels' output.  The final cell state is held to the same bar
with the ulp scaled by max |c|.
Condition on the inputs: e32 < 1e-5 is asserted for every case -- a recurrence that amplifies rounding (weights x 16 go chaotic)
cannot judge a kernel.
The framing and layout kernels are copies plus one fp32 add and must be bit-exact.
"""
import functools

import numpy as np
import pytest

from tests import lstm_ref as R

pytestmark = pytest.mark.gpu

SCALES = ((1.0, 1.0), (4.0, 1.0), (1.0, 6.0))     # (s, s_x): the last two push the gates into saturation

# (N, H, steps) of hd_lstm_step_kernel, the smallest that reach each path:
HD_CASES = (
    (1, 16, 1),        # a single wave's K range (kc = 16), one step from zero state
    (15, 16, 3),       # one tile with a padding column
    (16, 48, 7),       # exactly one tile; kc = 16 with three working waves
    (17, 80, 5),       # two tiles, the second holding one sequence; kc = 32, the third wave takes a partial range
    (128, 32, 4),      # 8 tiles in one z block; waves 2 and 3 idle
    (129, 48, 200),    # 9 tiles -> nz 2, tpz 5: 5 + 4, the last tile holds one sequence; 200 steps
    (300, 64, 9),      # 19 tiles -> nz 3, tpz 7: 7 + 7 + 5
    (137, 192, 200),   # the hdemucs_mmi hidden sizes at full frame length
    (20, 384, 200),
)
HD_SATURATED = ((17, 80, 5), (129, 48, 200), (137, 192, 200))
HD_PARAMS = [c + SCALES[0] for c in HD_CASES] + [c + sc for c in HD_SATURATED for sc in SCALES[1:]]
# Measured on an MI355X, worst err / max(e32, 2^-23) over these cases (bar 8): h 1.06 ((137, 192, 200) at (1, 6); 1.02 at (129, 48, 200)
# x (1, 1), 0.32 - 0.99 elsewhere), final c 0.97 ((17, 80, 5) at (4, 1)) -- the step kernel is as close to float64 as the plain fp32
# evaluation.

VR_HS = (4, 8, 16, 32, 64, 128)
VR_PARAMS = [(hs, W, B) + SCALES[0] for hs in VR_HS for W, B in ((1, 1), (2, 3), (33, 2))] + \
            [(hs, 256, 2) + sc for hs in (64, 128) for sc in SCALES[:2]]
# Measured on an MI355X, worst err / max(e32, 2^-23) per hidden size (bar 8): hs 4 0.87, 8 0.91, 16 0.87, 32 1.10, 64 1.91 ((256, 2) at
# (4, 1)), 128 2.51 ((33, 2) at (1, 1) and (256, 2) at (4, 1)): vr_lstm_seq_kernel adds its hs products one after the other, the fp32
# evaluation's matrix product adds them in blocks, so the ratio grows with hs.


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def case(N, H, steps, s=1.0, s_x=1.0):
    """inputs, float64 reference and the error of the plain fp32 evaluation -- computed once, shared, read-only"""
    xp, whh = R.make_inputs(N, H, steps, s, s_x)
    ref, cref = R.lstm_layer(xp, whh, N, H, steps)
    o32, c32 = R.lstm_layer(xp, whh, N, H, steps, np.float32)
    for a in (xp, whh, ref, cref):
        a.setflags(write=False)
    return xp, whh, ref, cref, R.worst(o32, ref), R.worst(c32, cref)


def judge(label, out, c, ref, cref, e32, e32c):
    """the condition on the input, then the bar on h and on the final cell state; prints the measured ratios"""
    assert e32 < R.COND_CAP and e32c < R.COND_CAP, f"{label}: fp32 evaluation off by {e32:.2e} / {e32c:.2e}, the input cannot judge a kernel"
    err = R.worst(out.reshape(ref.shape), ref)
    cmax = float(np.abs(cref).max())
    print(f"{label}: h err {err:.3e} e32 {e32:.3e} ratio {err / max(e32, R.ULP):.2f}", end="")
    assert err <= R.bar(e32), f"{label}: h off by {err:.3e}, plain fp32 by {e32:.3e}"
    if c is not None:
        errc = R.worst(c, cref)
        print(f" | c err {errc:.3e} e32 {e32c:.3e} max|c| {cmax:.2f} ratio {errc / max(e32c, R.ULP * cmax):.2f}", end="")
        assert errc <= R.bar(e32c, cmax), f"{label}: final c off by {errc:.3e}, plain fp32 by {e32c:.3e} (max |c| {cmax:.2f})"
    print()
    return err


# ---- hd_lstm_step_kernel ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,steps,s,s_x", HD_PARAMS)
def test_hd_step_vs_float64(eng, N, H, steps, s, s_x):
    xp, whh, ref, cref, e32, e32c = case(N, H, steps, s, s_x)
    out, c = eng.op_hd_lstm_layer(xp, whh, N, H, steps)          # out and c go in as NaN: finite everywhere = everything written
    assert np.isfinite(out).all() and np.isfinite(c).all()
    judge(f"hd ({N}, {H}, {steps}) x ({s:g}, {s_x:g})", out, c, ref, cref, e32, e32c)


@pytest.mark.parametrize("N,H,steps", [(17, 80, 5), (300, 64, 9), (129, 48, 200)])
def test_hd_step_is_deterministic(eng, N, H, steps):
    xp, whh = case(N, H, steps)[:2]
    a, ca = eng.op_hd_lstm_layer(xp, whh, N, H, steps)
    b, cb = eng.op_hd_lstm_layer(xp, whh, N, H, steps)
    assert np.array_equal(a, b) and np.array_equal(ca, cb)


@pytest.mark.parametrize("victim", [128, 79])
def test_hd_step_sequences_are_isolated(eng, victim):
    """NaN in every input of one sequence -- 128 is the clamped source of the padding columns and a tile of its own, 79 sits inside
    z block 0 -- reaches that sequence alone; all others come out bit for bit as in the clean run"""
    N, H, steps = 129, 48, 6
    xp, whh = case(N, H, steps)[:2]
    clean, cclean = eng.op_hd_lstm_layer(xp, whh, N, H, steps)
    bad = xp.reshape(steps, N, 2, 4 * H).copy()
    bad[:, victim] = np.nan
    out, c = eng.op_hd_lstm_layer(bad, whh, N, H, steps)
    out, clean = out.reshape(steps, N, 2 * H), clean.reshape(steps, N, 2 * H)
    others = np.arange(N) != victim
    assert np.isfinite(clean).all()
    assert np.array_equal(out[:, others], clean[:, others]) and np.array_equal(c[:, others], cclean[:, others])
    assert np.isnan(out[:, victim]).all() and np.isnan(c[:, victim]).all()


@pytest.mark.parametrize("j", [0, 15, 79, 80, 128])
def test_hd_step_does_not_depend_on_the_column(eng, j):
    """a sequence's summation order does not depend on where it sits: sequence j of N = 129 equals, bit for bit, the same sequence
    run alone and run as the last of 17"""
    N, H, steps = 129, 48, 6
    xp, whh = case(N, H, steps)[:2]
    full, cfull = eng.op_hd_lstm_layer(xp, whh, N, H, steps)
    full = full.reshape(steps, N, 2 * H)
    x4 = xp.reshape(steps, N, 2, 4 * H)
    alone, calone = eng.op_hd_lstm_layer(x4[:, j:j + 1], whh, 1, H, steps)
    assert np.array_equal(alone.reshape(steps, 2 * H), full[:, j]) and np.array_equal(calone[:, 0], cfull[:, j])
    pick = [n for n in range(17) if n != j][:16] + [j]
    last, clast = eng.op_hd_lstm_layer(x4[:, pick], whh, 17, H, steps)
    assert np.array_equal(last.reshape(steps, 17, 2 * H)[:, 16], full[:, j]) and np.array_equal(clast[:, 16], cfull[:, j])


@pytest.mark.parametrize("N,H,steps,mutants", [R.MUTANT_CASE + (R.MUTANTS + (R.FINE_MUTANT,),), (16, 48, 7, ("drop_k_tail", R.FINE_MUTANT))])
def test_bar_catches_mutants(eng, N, H, steps, mutants):
    """the kernel stays under the bar on an input where each deliberately wrong recurrence (tests/lstm_ref.py) is beyond it; the fine
    mutant is 40-50 x the bar away, so this test fails if the bar is loosened 1000 x (test_host_lstm_ref.py pins that)"""
    xp, whh, ref, cref, e32, e32c = case(N, H, steps)
    out, c = eng.op_hd_lstm_layer(xp, whh, N, H, steps)
    judge(f"hd mutant input ({N}, {H}, {steps})", out, c, ref, cref, e32, e32c)
    for m in mutants:
        wrong, _ = R.lstm_layer(xp, whh, N, H, steps, mutant=m)
        assert R.worst(wrong, ref) > R.bar(e32), f"the bar {R.bar(e32):.2e} would pass mutant '{m}' ({R.worst(wrong, ref):.2e})"


def test_hd_step_refuses_other_shapes(eng):
    import audio_separator_amd as A
    for N, H, steps in ((2, 24, 3), (2, 8, 3), (0, 16, 3), (2, 16, 0), (2, 0, 3)):
        n = max(N, 0) * max(steps, 0)
        with pytest.raises(A.AsxError, match="asx error 1:"):
            eng.op_hd_lstm_layer(np.zeros((n, 2, 4 * H), np.float32), np.zeros((2, 4 * H, H), np.float32), N, H, steps,
                                 out=np.zeros((n, 2 * H), np.float32))


# ---- hd_lstm_frame_kernel / hd_lstm_unframe_kernel ---------------------------------------------------------------------------------
FRAME_PARAMS = [(T, B, 16) for T in (1, 47, 200, 201, 250, 299, 300, 301, 517) for B in (1, 2)] + [(517, 1, 192)]


@pytest.mark.parametrize("T,B,H", FRAME_PARAMS)
def test_hd_frames_bit_exact(eng, T, B, H):
    rng = np.random.default_rng([T, B, H])
    h = rng.standard_normal((B, T, H)).astype(np.float32)
    steps, nfr = R.framing(T)
    ntot, n_off = B * nfr + 5, 3
    want, _, _ = R.blstm_frames(h, T, ntot, n_off)
    rows, gsteps, gnfr = eng.op_hd_lstm_frames(h, ntot, n_off)              # rows go in as NaN
    assert (gsteps, gnfr) == (steps, nfr)
    assert np.array_equal(rows, want, equal_nan=True)
    r3 = rows.reshape(steps, ntot, H)
    assert np.isnan(r3[:, :n_off]).all() and np.isnan(r3[:, n_off + B * nfr:]).all(), "rows of other groups were written"
    mine = r3[:, n_off:n_off + B * nfr].reshape(steps, B, nfr, H)
    assert np.isfinite(mine).all()
    for k in range(nfr):                                                      # zero-padded frame tails are exactly 0
        assert not mine[max(T - k * 100, 0):, :, k].any()
    # the way back: other groups' rows are NaN and must not be read
    lin = np.full((steps * ntot, H), np.nan, np.float32)
    lin.reshape(steps, ntot, H)[:, n_off:n_off + B * nfr] = rng.standard_normal((steps, B * nfr, H)).astype(np.float32)
    got, gsteps, gnfr = eng.op_hd_lstm_frames(h, ntot, n_off, rows=lin, unframe=True)
    assert (gsteps, gnfr) == (steps, nfr)
    assert np.array_equal(got, R.blstm_unframe(lin, h, T, ntot, n_off)) and np.isfinite(got).all()


def test_hd_frames_refuses_rows_that_do_not_fit(eng):
    import audio_separator_amd as A
    h = np.zeros((2, 301, 16), np.float32)
    for ntot, n_off in ((7, 0), (8, 1), (8, -1)):                              # 2 x 4 sequences
        with pytest.raises(A.AsxError, match="asx error 1:"):
            eng.op_hd_lstm_frames(h, ntot, n_off, rows=np.zeros((200 * ntot, 16), np.float32))


# ---- vr_lstm_seq_kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hs,W,B,s,s_x", VR_PARAMS)
def test_vr_seq_vs_float64(eng, hs, W, B, s, s_x):
    xp, whh, ref, cref, e32, e32c = case(B, hs, W, s, s_x)
    out = eng.op_vr_lstm(xp, whh, W, B, hs)                                   # goes in as NaN
    assert out.shape == (W, B, 2 * hs) and np.isfinite(out).all()
    judge(f"vr hs {hs} ({W}, {B}) x ({s:g}, {s_x:g})", out, None, ref, cref, e32, e32c)
    assert np.array_equal(out, eng.op_vr_lstm(xp, whh, W, B, hs)), "two runs differ"


@pytest.mark.parametrize("hs", VR_HS)
def test_vr_seq_batch_items_are_independent(eng, hs):
    for W in (2, 33):
        xp, whh = case(3, hs, W)[:2]
        full = eng.op_vr_lstm(xp, whh, W, 3, hs)
        x4 = xp.reshape(W, 3, 2, 4 * hs)
        for b in range(3):
            assert np.array_equal(eng.op_vr_lstm(x4[:, b:b + 1], whh, W, 1, hs)[:, 0], full[:, b]), (W, b)


def test_vr_seq_refuses_other_sizes(eng):
    import audio_separator_amd as A
    for hs, W, B in ((24, 2, 1), (256, 2, 1), (0, 2, 1), (16, 0, 1), (16, 2, 0)):
        with pytest.raises(A.AsxError, match="asx error 1:"):
            eng.op_vr_lstm(np.zeros((W, B, 2, 4 * hs), np.float32), np.zeros((2, 4 * hs, hs), np.float32), W, B, hs,
                           out=np.zeros((W, B, 2 * hs), np.float32))


# (ld, ch0) = (4, 4) names channels beyond the pixel: vr_lstm_out_kernel's 16-byte store would land in the next pixel, so the hook refuses it
@pytest.mark.parametrize("ld,ch0", [(4, 0), (12, 0), (12, 4)])
def test_vr_layout_bit_exact(eng, ld, ch0):
    B, H, W = 2, 5, 37                                                         # 370 elements: two workgroups, the second partial
    rng = np.random.default_rng([ld, ch0])
    hc = rng.standard_normal((B, H, W, ld)).astype(np.float32)
    xs = eng.op_vr_lstm_layout(hc, B, H, W, ld, ch0)                         # goes in as NaN
    assert np.array_equal(xs, R.vr_lstm_in(hc, ch0))
    ys = rng.standard_normal((W, B, H)).astype(np.float32)
    dst = rng.standard_normal((B, H, W, ld)).astype(np.float32)
    got = eng.op_vr_lstm_layout(ys, B, H, W, ld, ch0, dst=dst, out=True)
    assert np.array_equal(got, R.vr_lstm_out(ys, dst, ch0))
    assert not got[..., ch0 + 1:ch0 + 4].any()
    keep = np.ones(ld, bool)
    keep[ch0:ch0 + 4] = False
    assert np.array_equal(got[..., keep], dst[..., keep])


def test_vr_layout_refuses_channels_outside_the_pixel(eng):
    import audio_separator_amd as A
    for ld, ch0, out in ((4, 4, True), (4, 4, False), (12, 10, True), (12, 2, True), (6, 0, True)):
        src = np.zeros((3, 2, 2) if out else (2, 2, 3, ld), np.float32)
        with pytest.raises(A.AsxError, match="asx error 1:"):
            eng.op_vr_lstm_layout(src, 2, 2, 3, ld, ch0, out=out)
