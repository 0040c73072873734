"""CPU checks of what tests/test_gpu_norm_kernels.py stands on: the float64 references of tests/norm_ref.py agree with torch's own
functions in float64 (F.normalize, F.layer_norm, F.group_norm, F.instance_norm, torch.std) to a few float64 ulps of the scale; every
case of tests/norm_cases.py meets the input condition e32 <= 4 x 2^-23; and the measure tells a wrong formula from the right one --
unbiased for biased (and the reverse), eps outside the root, statistics without the cropped rows -- when the wrong formula is fed
through it as if it were the kernel."""
import numpy as np
import pytest
import torch

from tests import norm_cases as K
from tests import norm_ref as R

F64_ULPS = 16 * 2.0 ** -52         # "a few float64 ulps of the scale": two evaluation orders of ~10 roundings each
CASES = K.ROW + K.GROUP


@pytest.mark.parametrize("op", sorted({c["op"] for c in CASES}))
def test_references_agree_with_torch_float64(op):
    worst = 0.0
    for c in (c for c in CASES if c["op"] == op):
        d = K.build(c["name"])
        err, zero_bad = R.measure(R.torch_eval(op, torch.float64, **d), d["y"], d["s"])
        worst = max(worst, err)
        assert zero_bad == 0 and err <= F64_ULPS, f"{c['name']}: torch float64 differs by {err:.3e} of the scale"
        if op == "rms":
            err = R.measure(R.torch_eval("rms_factor", torch.float64, **d), d["r"], d["r_s"])[0]
            assert err <= F64_ULPS, f"{c['name']}: rms_factor differs by {err:.3e}"
    print(f"{op}: worst |torch64 - ref| / s = {worst:.3e} ({worst * 2.0 ** 52:.2f} ulps)")


def test_v3_stats_table_agrees_with_torch_float64():
    for c in (c for c in K.GROUP if c["op"] == "v3" and c["norm"] not in (None, "BatchNorm")):
        d = K.build(c["name"])
        x = torch.from_numpy(d["x"]).double()
        G = x.shape[1] if c["norm"] == "InstanceNorm" else int(c["norm"][9:])
        xg = x.reshape(x.shape[0], G, -1)
        mean, var = xg.mean(dim=2), xg.var(dim=2, unbiased=False)
        want = torch.stack([mean, 1.0 / torch.sqrt(var + 1e-5)], dim=2).repeat_interleave(x.shape[1] // G, dim=1).numpy()
        assert np.allclose(d["stats"], want, rtol=1e-12, atol=1e-13), c["name"]   # atol: a mean that cancels to ~1e-3 from terms of ~1e3


def test_every_case_meets_the_input_condition():
    """e32 <= 4 x 2^-23: the inputs are such that plain fp32 arithmetic is accurate in this measure, so the bar is close to 8 x 2^-23"""
    worst = {}
    for c in CASES:
        d = K.build(c["name"])
        for k in ("e32", "r_e32"):
            if k in d:
                assert d[k] <= 4 * R.U32, f"{c['name']}: {k} = {d[k] / R.U32:.2f} x 2^-23"
                worst[c["op"] + ("" if k == "e32" else "_factor")] = max(worst.get(c["op"], 0.0), d[k] / R.U32)
    print({k: round(v, 2) for k, v in worst.items()})


def test_case_lists_cover_the_paths():
    names = set(K.BY_NAME)
    assert {(c["d"], c["M"]) for c in K.ROW if c["op"] == "rms"} >= {(d, m) for d in (8, 72, 100, 384, 513) for m in K.M_EDGES}
    assert {(c["d"], c["M"]) for c in K.ROW if c["op"] == "layer"} >= {(d, m) for d in (4, 100, 384, 512) for m in K.M_EDGES}
    for fam in ("ht", "hd", "std", "time", "hd_time", "v3", "mdx"):
        assert {c["variant"] for c in K.GROUP if c["op"] == fam} == set(K.VARIANTS), fam
    assert {c["variant"] for c in K.STATS} == set(K.VARIANTS)
    flat = [c["dims"][2] for c in K.STATS if c["name"].startswith("stats-flat")]
    assert flat == [1000, 65534, 65536, 2 * K.PRIME] and K.PRIME > 32768
    assert {"rms-inplace-d384-M9", "rms-zero-row-d72-M5"} <= names
    for c in K.ROW + K.STATS + K.GROUP:                           # a few hundred KB at most
        assert K.build(c["name"])["x"].nbytes <= 640 * 1024, c["name"]


def test_group_sums_bound_holds_for_numpy_sums():
    for c in K.STATS:
        d = K.build(c["name"])
        G1, Rr, P, gdiv, ld, cn, g2 = c["dims"]
        x = d["x"].astype(np.float64)
        i = np.arange(P)
        for g in range(g2):
            v = x[:, :, (i // gdiv == g) & (i % ld < cn)].reshape(G1, -1)
            got = np.stack([v.sum(axis=1), (v * v).sum(axis=1)], axis=1)
            assert (np.abs(got - d["sums"][:, g]) <= d["bound"][:, g]).all(), (c["name"], g)
    assert (K.build("stats-dconv-ld8-cn6")["bound"] > 0).all()


def test_measure_counts_nan_as_infinite_and_scaleless_elements_apart():
    ref, s = np.array([1.0, 0.0, 2.0]), np.array([1.0, 0.0, 2.0])
    assert R.measure(np.array([1.0, 0.0, 2.0], np.float32), ref, s) == (0.0, 0)
    assert R.measure(np.array([np.nan, 0.0, 2.0], np.float32), ref, s) == (np.inf, 0)
    assert R.measure(np.array([1.0, 1e-30, 2.0], np.float32), ref, s)[1] == 1
    assert R.measure(np.array([1.0, np.nan, 2.5], np.float32), ref, s) == (0.25, 1)
    assert R.bar(0.0) == 8 * 2.0 ** -23 and R.bar(2.0 ** -22) == 8 * 2.0 ** -22


def test_zero_scale_elements_of_the_references():
    d = K.build("rms-zero-row-d72-M5")
    assert (d["s"][2] == 0).all() and (d["y"][2] == 0).all() and (d["s"][[0, 1, 3, 4]] > 0).all() and d["r_s"][2] == 72 ** 0.5 / 1e-12
    d = K.build("hd_time-L255-n")
    assert d["y"].shape == (2, 256, 2) and (d["s"][:, 255] == 0).all() and (d["s"][:, :255] > 0).all()
    x, gamma = K.scale_rows()
    y, _ = R.rms(x, gamma)
    assert np.allclose(y[1], y[0], rtol=1e-13) and np.allclose(y[2], y[0], rtol=1e-13)   # neither scaled row meets the 1e-12 clamp


# ---- a wrong formula, fed through the measure as if it were the kernel, fails the bar ------------------------------------------------------
def _wrong_fails(name, wrong):
    d = K.build(name)
    err = R.measure(wrong.astype(np.float32), d["y"], d["s"])[0]
    assert err > R.bar(d["e32"]), f"{name}: the wrong formula is off by only {err:.3e} of the scale, the bar is {R.bar(d['e32']):.3e}"
    right = R.measure(d["y"].astype(np.float32), d["y"], d["s"])[0]
    assert right <= R.bar(d["e32"]), f"{name}: the reference rounded to fp32 is off by {right:.3e}"
    return err / R.bar(d["e32"])


# the shifted inputs are left out here: their scale holds |mean| = 1024 standard deviations, and a variance wrong by 1 / n or an eps
# moved by 1e-5 changes an element by less than 2^-23 of that
SEEN = ("n", "small")


def test_unbiased_for_biased_fails():
    r = [_wrong_fails(c["name"], R.v3_norm_act(K.build(c["name"])["x"], c["norm"], K.build(c["name"])["gamma"], K.build(c["name"])["beta"],
                                               c["act"], c["alpha"], unbiased=True)[0])
         for c in K.GROUP if c["op"] == "v3" and c["norm"] not in (None, "BatchNorm") and c["variant"] in SEEN and "split" not in c["name"]]
    assert len(r) >= 8
    print(f"unbiased for biased: {min(r):.1f} .. {max(r):.1f} x the bar")


def test_biased_for_unbiased_fails():
    r = [_wrong_fails(c["name"], R.standardize(K.build(c["name"])["x"], biased=True)[0])
         for c in K.GROUP if c["op"] == "std" and c["variant"] in SEEN]
    r += [_wrong_fails(c["name"], R.standardize(K.build(c["name"])["x"], biased=True)[0].transpose(0, 2, 1))
          for c in K.GROUP if c["op"] == "time" and c["variant"] in SEEN]
    assert len(r) >= 8
    print(f"biased for unbiased: {min(r):.1f} .. {max(r):.1f} x the bar")


def test_eps_misplaced_fails():
    r = [_wrong_fails(c["name"], R.v3_norm_act(K.build(c["name"])["x"], c["norm"], K.build(c["name"])["gamma"], K.build(c["name"])["beta"],
                                               c["act"], c["alpha"], eps_outside=True)[0])
         for c in K.GROUP if c["op"] == "v3" and c["norm"] not in (None, "BatchNorm") and c["variant"] in SEEN]
    r += [_wrong_fails(c["name"], R.standardize(K.build(c["name"])["x"], eps_inside=True)[0])
          for c in K.GROUP if c["op"] == "std" and c["variant"] == "small"]
    assert len(r) >= 8
    print(f"eps on the wrong side of the root: {min(r):.1f} .. {max(r):.1f} x the bar")


def test_statistics_without_the_cropped_rows_fail():
    r = []
    for c in K.GROUP:
        if c["op"] == "hd" and c["r0"] and c["variant"] != "shift":
            d = K.build(c["name"])
            r.append(_wrong_fails(c["name"], R.hd_group_norm(d["x"], d["G"], d["gamma"], d["beta"], d["mode"], d["r0"], d["R"], d.get("skip"),
                                                             crop_stats=True)[0]))
    assert len(r) >= 8
    print(f"statistics of the kept rows only: {min(r):.1f} .. {max(r):.1f} x the bar")


def test_crop_offset_off_by_one_fails():
    for c in K.GROUP:
        if c["op"] == "hd" and c["r0"]:
            d = K.build(c["name"])
            _wrong_fails(c["name"], R.hd_group_norm(d["x"], d["G"], d["gamma"], d["beta"], d["mode"], d["r0"] + 1, d["R"], d.get("skip"))[0])
