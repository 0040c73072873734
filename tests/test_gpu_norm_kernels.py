"""Every normalisation and statistics launch against float64, one launch at a time through asx_op_rownorm / asx_op_group_stats /
asx_op_group_norm (include/asx.h): rmsnorm_kernel, rownorm_kernel (csrc/kernels_rof.h), layernorm_kernel, gstats_kernel with its three
paths, gn_apply_kernel mode 2, std_norm_kernel, time_norm_kernel (csrc/kernels_ht.h), hd_gn_kernel, hd_time_norm_kernel
(csrc/kernels_hd.h), instnorm_stats_kernel, v3_gn_partial_kernel, v3_gn_finish_kernel, norm_act_kernel, gn_partial_kernel and the
ConvTDFNet gn_apply_kernel (csrc/kernels_fft.h).  The hooks go through the launch helpers the nets use (rof_rmsnorm, rof_rownorm, ht_ln,
ht_stats, ht_norm_out, ht_spec_standardize, ht_wave_standardize, hd_wave_standardize, the cores of hd_group_norm and v3_norm_act,
gn_launch).

Error measure (tests/norm_ref.py): the worst element of |kernel - f64| / s, s the sum of the magnitudes of the terms that form the
element; NaN counts as infinite; elements with s = 0 (the all-zero RMSNorm row, the pad sample of hd_time_norm_kernel) must come back
as exact zeros, asserted apart.  Bar: 8 x max(e32, 2^-23), e32 the same measure of torch's fp32 evaluation of the same input on the CPU
at run time; the factor 8 is that of test_gpu_gconv.py, test_gpu_lstm_kernels.py and test_gpu_stft_kernels.py.  Nothing in the bar
comes from the kernels' output.  The float64 sums of asx_op_group_stats must lie within n 2^-53 (sum |v|, sum v^2) of the reference's,
the (mean, rstd) table of "v3" within 2^-23 relative.  Every case goes in with a NaN-filled output (what the launch does not own -- pad
columns -- must come back bit for bit), runs twice and must repeat bit for bit; the in-place RMSNorm and GroupNorm cases must also equal
the out-of-place result bit for bit.

Measured on an MI355X, the worst measured / bar per kernel over the cases below (all pass; the bar is 1.000; errors are 0.3e-7 ..
2.2e-7 of the scale, level with torch's fp32 evaluation):
  rmsnorm_kernel          0.188 (rms-d384-M5-small)          rownorm_kernel       0.118 (rms-d72-M5-n)
  layernorm_kernel        0.153 (layer-C100-M3-small)        gstats + gn_apply 2  0.145 (ht-C100-N9-const)
  gstats + hd_gn_kernel   0.137 (hd-C96-gelu-skip-crop-n)    gstats + std_norm    0.125 (std-T5-c512-n)
  gstats + time_norm      0.169 (time-L255-n)                gstats + hd_time_norm 0.143 (hd_time-L255-small)
  instnorm_stats + norm_act 0.137 (v3-InstanceNorm-elu1.0-P1001-const)
  v3_gn_partial / finish + norm_act 0.149 (v3-GroupNorm1-split-P4096-n)   norm_act alone (None / BatchNorm) 0.098
  gn_partial + gn_apply (ConvTDFNet) 0.141 (mdx-C48-P1001-res-mul-small)
The float64 sums of gstats_kernel: at most 0.16 of their worst-case bound (stats-gdiv4-P512, the squares); the (mean, rstd) table of
"v3": at most 0.51 x 2^-23 relative.  No element without a scale came back other than an exact zero; the in-place launches equal the
out-of-place ones bit for bit (the aliasing qualifiers of rmsnorm_kernel stay), and a row scaled by 2^+-50 gives the unit-scale bits.
What was wrong: the repeat check failed for 14 of the 19 asx_op_group_stats cases.  gstats_kernel added its float64 partial sums with
LDS atomics inside a workgroup and global atomics across workgroups, in arrival order, so the low bits of the sums changed from run to
run.  It now leaves per-workgroup partial sums, added thread by thread, and gstats_finish_kernel adds them in a fixed order.
"""
import contextlib

import numpy as np
import pytest

from tests import norm_cases as K
from tests import norm_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import audio_separator_amd as A
    e = A.Engine(A.MDXConfig(n_fft=96, hop_length=16, dim_f=32, segment_size=16))
    yield e
    e.close()


@contextlib.contextmanager
def stop_on_hip_error():
    """a failed HIP call (ASX_ERR_HIP = 2: a launch error or a fault) ends the session: nothing more is started on that device"""
    from audio_separator_amd.engine import AsxError
    try:
        yield
    except AsxError as e:
        if str(e).startswith("asx error 2"):
            pytest.exit(f"HIP error, stopping: {e}", returncode=3)
        raise


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def twice(name, launch):
    """the launch's results (a tuple of arrays), run twice: they must repeat bit for bit"""
    with stop_on_hip_error():
        a, b = launch(), launch()
    assert all(same_bits(p, q) for p, q in zip(a, b)), f"{name}: two runs differ"
    return a


def report(name, got, ref, s, e32, what=""):
    err, zero_bad = R.measure(got, ref, s)
    bar = R.bar(e32)
    print(f"{name}{what}: err {err:.3e} e32 {e32:.3e} bar {bar:.3e} measured / bar {err / bar:.3f}; {zero_bad} scale-less elements not exact zeros")
    assert zero_bad == 0, f"{name}{what}: {zero_bad} elements without a scale are not exact zeros"
    assert err <= bar, f"{name}{what}: off by {err:.3e} of its scale, plain fp32 by {e32:.3e} (bar {bar:.3e})"


def padded(a, ld):
    """a [M, d] in rows of ld floats, the pad columns NaN"""
    out = np.full((a.shape[0], ld), np.nan, np.float32)
    out[:, :a.shape[1]] = a
    return out


# ---- asx_op_rownorm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in K.ROW if c["op"] == "rms"])
def test_rmsnorm_vs_float64(eng, name):
    c, d = K.BY_NAME[name], K.build(name)
    M, dd = c["M"], c["d"]
    lda, ldy = c.get("lda", dd), c.get("ldy", dd)
    x = padded(d["x"], lda)
    y0 = np.full((M, ldy), np.nan, np.float32)
    y, = twice(name, lambda: (eng.op_rownorm("rms", x, dd, d["gamma"], y=y0),))
    assert same_bits(y[:, dd:], y0[:, dd:]), f"{name}: wrote into the pad columns"
    report(name, y[:, :dd], d["y"], d["s"], d["e32"])
    if c.get("in_place"):
        z, = twice(name, lambda: (eng.op_rownorm("rms", x, dd, d["gamma"], in_place=True),))
        assert same_bits(z[:, dd:], x[:, dd:]), f"{name}: in place, wrote into the pad columns"
        assert same_bits(z[:, :dd], y[:, :dd]), f"{name}: the in-place launch differs from the out-of-place one"
    r, = twice(name, lambda: (eng.op_rownorm("rms_factor", x, dd),))
    report(name, r, d["r"], d["r_s"], d["r_e32"], " (rms_factor)")


def test_rmsnorm_power_of_two_rows(eng):
    """a row times 2^+50 and 2^-50: y equals the unit-scale y bit for bit, r is exactly 2^-+50 times the unit-scale r"""
    x, gamma = K.scale_rows()
    y, = twice("scale-rows", lambda: (eng.op_rownorm("rms", x, x.shape[1], gamma),))
    r, = twice("scale-rows", lambda: (eng.op_rownorm("rms_factor", x, x.shape[1]),))
    ref, s = R.rms(x[:1], gamma)
    report("scale-rows", y[:1], ref, s, 0.0)
    assert same_bits(y[1], y[0]) and same_bits(y[2], y[0]), "RMSNorm of a row scaled by a power of two differs from the unit-scale row"
    assert r[1] == r[0] * np.float32(2.0 ** -50) and r[2] == r[0] * np.float32(2.0 ** 50), r


@pytest.mark.parametrize("name", [c["name"] for c in K.ROW if c["op"] == "layer"])
def test_layernorm_vs_float64(eng, name):
    c, d = K.BY_NAME[name], K.build(name)
    y, = twice(name, lambda: (eng.op_rownorm("layer", d["x"], c["d"], d["gamma"], d["beta"], pos=d.get("pos")),))
    report(name, y, d["y"], d["s"], d["e32"])


def test_rownorm_refuses_what_the_launch_code_would_not_take(eng):
    from audio_separator_amd.engine import AsxError
    x = np.zeros((3, 8), np.float32)
    g = np.ones(8, np.float32)
    for bad in (lambda: eng.op_rownorm("rms", x, 8, g, y=np.zeros((3, 12), np.float32), in_place=True),      # in place with lda != ldy
                lambda: eng.op_rownorm("rms", x, 8, None),
                lambda: eng.op_rownorm("layer", x, 8, g, None),
                lambda: eng.op_rownorm("layer", padded(x, 12), 8, g, g),                                        # ht_ln takes dense rows
                lambda: eng.op_rownorm("batch", x, 8, g)):
        with pytest.raises(AsxError, match="asx error 1"):
            bad()


# ---- asx_op_group_stats ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in K.STATS])
def test_group_stats_vs_float64(eng, name):
    c, d = K.BY_NAME[name], K.build(name)
    _, _, _, gdiv, ld, cn, g2 = c["dims"]
    acc, = twice(name, lambda: (eng.op_group_stats(d["x"], gdiv, ld, cn, g2),))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(d["bound"] > 0, np.abs(acc - d["sums"]) / d["bound"], np.where(acc == d["sums"], 0.0, np.inf))
    ratio = np.where(np.isfinite(acc), ratio, np.inf)
    print(f"{name}: worst |sum - f64| / (n 2^-53 sum |v|) = {ratio[..., 0].max():.3f}, of the squares {ratio[..., 1].max():.3f}")
    assert ratio.max() <= 1.0, f"{name}: a float64 sum is off by {ratio.max():.3f} x its worst-case bound"


def test_group_stats_refuses_more_than_66_groups_per_workgroup(eng):
    from audio_separator_amd.engine import AsxError
    for G1, Rr, P, gdiv, ld, cn, g2 in K.STATS_REFUSED:
        with pytest.raises(AsxError, match="asx error 1.*66"):
            eng.op_group_stats(np.zeros((G1, Rr, P), np.float32), gdiv, ld, cn, g2)
    with pytest.raises(AsxError, match="asx error 1"):
        eng.op_group_stats(np.zeros((1, 2, 64), np.float32), 8, 8, 8, 7)           # 8 groups in the plane, room for 7


# ---- asx_op_group_norm -----------------------------------------------------------------------------------------------------------------
def _launch(eng, c, d, in_place):
    op = c["op"]
    kw = dict(in_place=int(in_place))
    if op == "hd":
        kw.update(g=c["G"], mode=c["mode"], r=c["R"], r0=c["r0"])
        return eng.op_group_norm("hd", d["x"], d["gamma"], d["beta"], aux=d.get("skip"), **kw)
    if op == "v3":
        x, c0 = d["x"], c.get("c0", 0)
        if "ctot" in c:                                                 # the case's channels as a view inside NaN channels
            x = np.full((x.shape[0], c["ctot"], x.shape[2]), np.nan, np.float32)
            x[:, c0:c0 + d["x"].shape[1]] = d["x"]
        return eng.op_group_norm("v3", x, d.get("gamma"), d.get("beta"), norm=c["norm"], act=c["act"], alpha=c["alpha"], c=d["x"].shape[1], c0=c0)
    if op == "mdx":
        return eng.op_group_norm("mdx", d["x"], d["gamma"], d["beta"], aux=d.get("res"), mul=d.get("mul"), **kw)
    return eng.op_group_norm(op, d["x"], d.get("gamma"), d.get("beta"))


@pytest.mark.parametrize("name", [c["name"] for c in K.GROUP])
def test_group_norm_vs_float64(eng, name):
    c, d = K.BY_NAME[name], K.build(name)
    res = twice(name, lambda: (lambda r: r if isinstance(r, tuple) else (r,))(_launch(eng, c, d, c.get("in_place", False))))
    report(name, res[0], d["y"], d["s"], d["e32"])
    if c.get("in_place"):
        out, = twice(name, lambda: (_launch(eng, c, d, False),))
        assert same_bits(out, res[0]), f"{name}: the in-place launch differs from the out-of-place one"
    if c["op"] == "v3":
        if d["stats"] is None:
            assert np.isnan(res[1]).all(), f"{name}: a launch without statistics wrote the (mean, rstd) table"
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(res[1] - d["stats"]) / np.abs(d["stats"])
            rel = np.where(np.isfinite(rel), rel, np.where(res[1] == d["stats"], 0.0, np.inf))
            print(f"{name}: (mean, rstd) off by {rel[..., 0].max() / R.U32:.3f} / {rel[..., 1].max() / R.U32:.3f} x 2^-23")
            assert rel.max() <= R.U32, f"{name}: the (mean, rstd) table is off by {rel.max():.3e} relative"


def test_group_norm_refuses_what_the_launch_code_would_not_take(eng):
    from audio_separator_amd.engine import AsxError
    x = np.zeros((2, 6, 16), np.float32)
    g = np.ones(16, np.float32)
    for bad in (lambda: eng.op_group_norm("hd", x, g, g, g=3, mode="none"),                      # C % G != 0
                lambda: eng.op_group_norm("hd", x, g, g, g=4, mode="none", r=6, r0=1),           # rows beyond rin
                lambda: eng.op_group_norm("hd", x, g, g, g=4, mode="glu", in_place=1),                # the GLU halves the channels
                lambda: eng.op_group_norm("v3", x, g[:6], g[:6], norm="GroupNorm4", act="relu"),  # 6 channels in 4 groups
                lambda: eng.op_group_norm("v3", x, None, None, norm=3, act="relu"),
                lambda: eng.op_group_norm("mdx", np.zeros((2, 7, 16), np.float32), g[:7], g[:7]),  # GroupNorm(2, 7)
                lambda: eng.op_group_norm("std", np.zeros((2, 3, 6), np.float32))):               # frames of 4 F floats
        with pytest.raises(AsxError, match="asx error 1"):
            bad()
