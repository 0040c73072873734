"""Every gathered-conv launch of HTDemucs, HDemucs / Demucs v3 and VR against float64, one ht_gg launch at a time through
asx_op_gconv, and the DConv chain through asx_op_dconv (csrc/engine_ht.h unchanged): gg_kernel<NREP, MREP, MS> (csrc/kernels_ht.h),
the halo-tile kernel (csrc/kernels_halo.h), the GATHER mode of the split-operand row GEMM (csrc/kernels_gemm3.h) in its bf16 x 6 and
fp16 x 3 arithmetics, rowstat_reduce_kernel and the GG_STATS / GG_GNGLU epilogues.

Error measure: the worst element of |kernel - float64| / S, NaN counting as infinite; S = sum |x| |w| + |b| of the pre-activation
(+ |res|; GLU: S_value + 0.25 |value| S_gate; tests/gconv_ref.py).  Every output goes in filled with NaN; whatever the launch does
not own -- columns outside [y_col0, y_col0 + Cout), the gaps between batch items -- must come back bit for bit.
Bar: 8 x max(e32, floor).  e32 is the same measure of the plain fp32 numpy evaluation of the same input, computed at run time
(tests/gconv_cases.py); floor = 2^-23 + the arithmetic's dropped term of the option text of include/asx.h (fp32 MFMA 0, bf16 x 6
2^-24, fp16 x 3 2^-22).  The factor 8 (that of test_gpu_lstm_kernels.py) covers the summation order (MFMA K steps, wave splits) and
the device erff, fast_sigmoid and fast_erf.  Nothing in it comes from the kernels' output.
Every case asserts `resolved` (kernel, N tile, lowai), runs twice and must repeat bit for bit.

gg_kernel's instantiations: the six that ht_gg_dispatch picks for launches with `lowai` set, and <1, 8>, <6, 2, true>, <2, 8>, which
need >= 1024 128-row blocks AND >= 90 flop / byte (the gg-grid1025-K216 cases: 131200 rows, 1.8e9 - 3.6e9 multiply-adds, the only
cases over 1e8).  The 256-row narrow tiles <N, 4, true> run only with ASX_GG_M128=0 in the environment and are not tested here.

Measured on an MI355X, the worst measured / bar per kernel over the cases below (all pass; the bar is 1.000):
  gg_kernel, lowai set     tile 16 <1, 2, true> 0.183 (gg-K32-n16), 32 <2, 2, true> 0.194 (gg-batch-gaps), 48 <3, 2, true> 0.236
                           (gather-N40-falls-back), 64 <1, 4> 0.252 (gg-IR5-N64), 96 <6, 1, true> 0.181 (convt-C24-Iout36-skip),
                           128 <2, 4> 0.139 (gg-N128)
  gg_kernel, lowai clear   tile 64 <1, 8> 0.140, 96 <6, 2, true> 0.126, 128 <2, 8> 0.134 (the gg-grid1025-K216 cases)
  halo-tile kernel         NT 32 0.209 (halo-3x3-O37), 64 0.193, 96 0.109 (halo-glu-C40), 128 0.126 (halo-N100)
  GATHER row GEMM          bf16 x 6 0.131 (gather-N136), fp16 x 3 0.059 (gather-k8s4); the fp16 x 3 dynamic-range case 3.3e-7 of a
                           row's own scale (bar 4e-6)
  DConv (asx_op_dconv)     y 0.079, h 0.238 (both G2 = 40), part 2 alone 0.119 (R = 8192, two workgroups); at an offset of 30
                           standard deviations y is 0.053 / 0.046 of the bar (err 5.1e-8 / 4.4e-8 of its scale against e32 5.0e-8 /
                           4.4e-8) and 6.1e-8 / 6.0e-8 of max |ref| -- level with the plain fp32 evaluation (the offset reaches the
                           normalised tensors through the column sums of random weights, and the fold adds the fp32 row sums
                           in float64)
"""
import numpy as np
import pytest

from tests import gconv_cases as K
from tests import gconv_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


def set_arith(eng, arith):
    eng.set_option("gemm_bf16x6", 1)
    eng.set_option("gemm_f16x3", 1 if arith == "f16x3" else 0)


def launch(eng, c, x, w, b, res):
    """the case through asx_op_gconv on a NaN-filled output, twice; the second run must repeat the first bit for bit"""
    B, OR = c["B"], c["OR"] or c["O"]
    img = c["O"] * c["Iout"] * c["ldy"] if c["mode"] == "convt" else OR * c["IR"] * c["ldy"]
    y0 = np.full(B * (img + c["y_gap"]), np.nan, np.float32)
    y, ran = eng.op_gconv(x, w, b, y0, res=res, variant=c["variant"], **K.desc(c))
    y2, ran2 = eng.op_gconv(x, w, b, y0, res=res, variant=c["variant"], **K.desc(c))
    assert ran == ran2 and np.array_equal(y.view(np.uint32), y2.view(np.uint32)), f"{c['name']}: two runs differ"
    v, own = K.y_view(c, y)
    assert np.array_equal(y.view(np.uint32)[~own], y0.view(np.uint32)[~own]), f"{c['name']}: wrote outside its view"
    return v, ran


def judge(c, v, ran, arith="fp32"):
    ref, S, e32 = K.reference(c["name"])
    exp = c["expect"]
    assert (ran[0] == exp) if isinstance(exp, str) else (ran == tuple(exp)), f"{c['name']}: ran {ran}, expected {exp}"
    err, bar = R.worst(v, ref, S), R.bar(e32, "fp32" if ran[0] != "gather" else arith)
    print(f"{c['name']} [{ran[0]} tile {ran[1]} lowai {ran[2]}{' ' + arith if ran[0] == 'gather' else ''}]: err {err:.3e} e32 {e32:.3e} bar {bar:.3e} "
          f"measured / bar {err / bar:.3f}")
    assert err <= bar, f"{c['name']}: off by {err:.3e} of its scale, plain fp32 by {e32:.3e} (bar {bar:.3e})"


@pytest.mark.parametrize("name", [c["name"] for c in K.GG])
def test_gg_kernel_vs_float64(eng, name):
    c = K.BY_NAME[name]
    v, ran = launch(eng, c, *K.inputs(name))
    judge(c, v, ran)


@pytest.mark.parametrize("name", [c["name"] for c in K.HALO])
def test_halo_kernel_vs_float64(eng, name):
    c = K.BY_NAME[name]
    v, ran = launch(eng, c, *K.inputs(name))
    judge(c, v, ran)


@pytest.mark.parametrize("arith", ["bf16x6", "f16x3"])
@pytest.mark.parametrize("name", [c["name"] for c in K.GATHER])
def test_gather_mode_vs_float64(eng, name, arith):
    c = K.BY_NAME[name]
    try:
        set_arith(eng, arith)
        n0, h0 = eng.counter("tdf3_gather_launches"), eng.counter("tdf3h_launches")
        v, ran = launch(eng, c, *K.inputs(name))
        n, h = eng.counter("tdf3_gather_launches") - n0, eng.counter("tdf3h_launches") - h0
    finally:
        set_arith(eng, "f16x3")
    if ran[0] == "gather":
        assert n == 2 and h == (2 if arith == "f16x3" else 0), f"{name}: the {arith} kernel did not run ({n}, {h})"
    else:
        assert n == 0 and h == 0
    judge(c, v, ran, arith)


@pytest.mark.parametrize("variant,kw", [
    ("halo", dict(O=5, I=16, Cin=8, Cout=32, SO=2, SI=2, OR=2, IR=8, KO=3, KI=3, PO=1, PI=1)),      # strided: not the halo kernel's
    ("halo", dict(O=5, I=16, Cin=12, Cout=32, KO=3, KI=3, PO=1, PI=1)),                             # Cin % 8
    ("halo", dict(O=6, I=8, Cin=8, Cout=32, KO=3, KI=3, DO=6, DI=2, PO=6, PI=2)),                   # haloed block over 512 pixels
    ("gather", dict(O=5, I=9, Cin=40, Cout=48, KO=3, KI=3, PO=1, PI=1)),
    ("gather", dict(O=5, I=9, Cin=32, Cout=40, KO=3, KI=3, PO=1, PI=1)),
    ("gather", dict(O=5, I=9, Cin=32, Cout=48)),                                                    # 1x1
    ("gg", dict(O=5, I=9, Cin=6, ldc=8, Cout=48)),                                                  # Cin % 4
    ("gg", dict(O=5, I=9, Cin=8, ldc=8, x_col0=4, Cout=48)),                                        # the view leaves the pixel
    ("gg", dict(O=5, I=9, Cin=8, Cout=8, ldy=12, y_col0=8)),
    ("gg", dict(O=5, I=9, Cin=8, Cout=8, KO=4, PO=1)),
    ("gg", dict(O=5, I=9, Cin=8, Cout=8, mode="glu", act=2)),
    ("gg", dict(O=5, I=9, IR=10, Cin=8, Cout=8, mode="convt", KI=2, PI=1, So=4, crop=2, Iout=36, SI=2)),
    ("wino", dict(O=5, I=9, Cin=8, Cout=8)),
])
def test_refused_launches_never_run(eng, variant, kw):
    """a descriptor or variant the launch code does not take is ASX_ERR_INVALID (raised by the binding), never a launch"""
    import audio_separator_amd as A
    c = K.mk("refused", variant, B=1, **kw)
    rng = np.random.default_rng(1)
    convt, glu = c["mode"] == "convt", c["mode"] == "glu"
    x = rng.standard_normal(c["O"] * c["I"] * c["ldc"]).astype(np.float32)
    w = rng.standard_normal((2 * c["So"] if convt else c["KO"] * c["KI"] * (2 if glu else 1)) * c["Cin"] * c["Cout"]).astype(np.float32)
    b = rng.standard_normal(c["Cout"] * (2 if glu else 1)).astype(np.float32)
    y0 = np.full(c["O"] * c["Iout"] * c["ldy"] if convt else (c["OR"] or c["O"]) * c["IR"] * c["ldy"], np.nan, np.float32)
    with pytest.raises(A.AsxError):
        eng.op_gconv(x, w, b, y0, variant=variant, **K.desc(c))


def test_gather_f16x3_dynamic_range(eng):
    """fp16 x 3 keeps one running exponent per gathered row: neighbouring pixels up to 2^18 apart (every output row gathers nine of
    them) and a 2^-20 decay along the channels; every output row within 4e-6 of its own scale, the bar of
    test_gpu_parity.py::test_rowgemm_f16x3_block_exponent"""
    B, O, I, Cin, N = 2, 9, 11, 64, 48
    rng = np.random.default_rng(77)
    pix = np.arange(B * O * I).reshape(B, O, I, 1)
    x = (rng.standard_normal((B, O, I, Cin)) * np.exp2(3.0 * (pix % 7) - 9.0) * np.exp2(-20.0 * np.arange(Cin) / Cin)).astype(np.float32)
    w = (rng.standard_normal((N, Cin, 3, 3)) / np.sqrt(9 * Cin)).astype(np.float32)
    b = np.zeros(N, np.float32)
    g = dict(KO=3, KI=3, PO=1, PI=1, IR=I)
    lin, _ = R.conv_pre(x, w, b, g)
    set_arith(eng, "f16x3")
    h0 = eng.counter("tdf3h_launches")
    y, ran = eng.op_gconv(x, w, b, np.full(lin.shape, np.nan, np.float32), variant="gather", B=B, O=O, I=I, Cin=Cin, ldc=Cin, Cout=N, ldy=N,
                          act=1, **g)
    assert ran[0] == "gather" and eng.counter("tdf3h_launches") == h0 + 1
    assert np.isfinite(y).all()
    scale = np.sqrt((lin ** 2).mean(axis=-1))
    err = np.sqrt(((y - np.maximum(lin, 0)) ** 2).mean(axis=-1))
    worst = float((err / scale).max())
    print(f"gather fp16 x 3, pixels 2^18 apart, 2^-20 along the channels: worst row error over its own scale {worst:.3e} (bar 4e-6)")
    assert worst < 4e-6, worst


# ---- the DConv chain -----------------------------------------------------------------------------------------------------------------
def dconv_run(eng, case, part=3, h=None):
    y, p = K.dconv_inputs(*case)
    a = eng.op_dconv(y, p, case[5], case[6], part, h)
    b = eng.op_dconv(y, p, case[5], case[6], part, h)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), "two runs differ"
    assert a[2] == 0 and b[2] == 0, "arrival counters left non-zero"
    return a[0], a[1]


def pad4(h):
    """h [B, O, I, hid] -> the engine's rows [B * O * I, hp] with zero padding channels"""
    hid = h.shape[-1]
    out = np.zeros((h.size // hid, (hid + 3) & ~3), np.float32)
    out[:, :hid] = h.reshape(-1, hid)
    return out


@pytest.mark.parametrize("case", K.DCONV, ids=lambda c: "-".join(str(v) for v in c))
def test_dconv_layer_vs_float64(eng, case):
    out, S, h, Sh, e32, e32h = K.dconv_reference(*case)
    y, hh = dconv_run(eng, case)
    hid = case[4]
    assert (hh[:, hid:] == 0).all(), "the padding channels of h must be zero"
    err, errh = R.worst(y, out, S), R.worst(hh[:, :hid], h, Sh)
    print(f"dconv {case}: y err {err:.3e} e32 {e32:.3e} measured / bar {err / R.bar(e32):.3f} | h err {errh:.3e} e32 {e32h:.3e} "
          f"measured / bar {errh / R.bar(e32h):.3f}")
    assert errh <= R.bar(e32h), f"h off by {errh:.3e} of its scale, plain fp32 by {e32h:.3e}"
    assert err <= R.bar(e32), f"y off by {err:.3e} of its scale, plain fp32 by {e32:.3e}"


@pytest.mark.parametrize("case", [K.DCONV[3], K.DCONV[10]], ids=lambda c: "-".join(str(v) for v in c))
def test_dconv_parts(eng, case):
    """part 1 alone leaves y alone and gives the h of part 3; part 2 alone, from the float64 h rounded to fp32, is judged against the
    tail restated from that h"""
    y0, p = K.dconv_inputs(*case)
    out, S, h, Sh, e32, e32h = K.dconv_reference(*case)
    y3, h3 = dconv_run(eng, case)
    y1, h1 = dconv_run(eng, case, part=1)
    assert np.array_equal(y1, y0) and np.array_equal(h1.view(np.uint32), h3.view(np.uint32))
    hin = pad4(h)
    ref2, S2 = R.dconv_tail(y0, hin[:, :case[4]].reshape(h.shape), None, p, case[5])
    r32, _ = R.dconv_tail(y0, hin[:, :case[4]].reshape(h.shape), None, p, case[5], np.float32)
    y2, h2 = dconv_run(eng, case, part=2, h=hin)
    assert np.array_equal(h2, hin)
    err, e = R.worst(y2, ref2, S2), R.worst(r32, ref2, S2)
    print(f"dconv {case} part 2: err {err:.3e} e32 {e:.3e} measured / bar {err / R.bar(e):.3f}")
    assert err <= R.bar(e)


@pytest.mark.parametrize("case", K.DCONV_OFF30, ids=lambda c: "-".join(str(v) for v in c))
def test_dconv_offset_30_is_finite(eng, case):
    """a mean of 30 standard deviations: the statistics are fp32 row sums of v and v^2, so the variance is a difference of large numbers
    (a CPU model of the fold gives about 7x the fp32 reference's error); only finiteness and the project's 1e-4 of max |ref| are held"""
    out, S, h, Sh, e32, e32h = K.dconv_reference(*case)
    y, hh = dconv_run(eng, case)
    assert np.isfinite(y).all() and np.isfinite(hh).all()
    err = R.worst(y, out, S)
    rel = float(np.abs(y - out).max() / np.abs(out).max())
    print(f"dconv {case}: y err {err:.3e} of its scale, e32 {e32:.3e}, measured / bar {err / R.bar(e32):.3f}; max |err| / max |ref| {rel:.3e}")
    assert rel < 1e-4, rel
