"""The float64 restatements of tests/gconv_ref.py against torch.nn.functional in channels-first float64, for every case of
tests/gconv_cases.py (every geometry class of tests/test_gpu_gconv.py), and the DConv restatement against the oracle's _dconv
(oracle/demucs_oracle.py).  Each case is also evaluated in plain fp32 -- e32, the figure the GPU test's bar is built from -- which
must be a rounding error, not a conditioning problem."""
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import demucs_oracle as DO
from tests import gconv_cases as K
from tests import gconv_ref as R

E32_CAP = 64 * R.ULP          # the plain fp32 evaluation of any case stays within a few dozen ulps of its error scale


def t64(a):
    return torch.from_numpy(np.array(a, np.float64))


def torch_act(v, code):
    return {0: lambda t: t, 1: torch.relu, 2: F.gelu, 6: F.gelu, 3: torch.tanh, 4: lambda t: F.leaky_relu(t, 0.01), 5: torch.sigmoid}[code](v)


def torch_case(c, x, w, b, res):
    """the case through torch, channels-first float64 -> channels-last numpy over the view"""
    xv = t64(K.x_view(c, x)).permute(0, 3, 1, 2)                       # [B, Cin, O, I]
    B, O, I = c["B"], c["O"], c["I"]
    r = None if res is None else t64(res[:, :c["Cout"]])
    if c["mode"] == "convt":
        seq = xv.permute(0, 2, 1, 3).reshape(B * O, c["Cin"], I)       # one sequence per (b, o)
        full = F.conv_transpose1d(seq, t64(w), t64(b), stride=c["So"])
        y = torch_act(full[:, :, c["crop"]:c["crop"] + c["Iout"]], c["act"]).permute(0, 2, 1).reshape(B, O, c["Iout"], c["Cout"])
        return (y if r is None else y + r.reshape(y.shape)).numpy()
    OR, IR = c["OR"] or O, c["IR"]
    # the descriptor fixes the output size: pad right / bottom with the zeros its last rows read, then crop
    need_o = (OR - 1) * c["SO"] + c["DO"] * (c["KO"] - 1) + 1
    need_i = (IR - 1) * c["SI"] + c["DI"] * (c["KI"] - 1) + 1
    xp = F.pad(xv, (c["PI"], max(0, need_i - I - c["PI"]), c["PO"], max(0, need_o - O - c["PO"])))
    v = F.conv2d(xp, t64(w).permute(0, 1, 3, 2), t64(b), stride=(c["SO"], c["SI"]), dilation=(c["DO"], c["DI"]))[:, :, :OR, :IR]
    y = F.glu(v, dim=1) if c["mode"] == "glu" else torch_act(v, c["act"])
    y = y.permute(0, 2, 3, 1)
    if r is not None:
        rows = torch.arange(B * OR * IR) % c["res_mod"] if c["res_mod"] else torch.arange(B * OR * IR)
        y = y + r[rows].reshape(y.shape)
    return y.numpy()


@pytest.mark.parametrize("name", sorted(K.BY_NAME))
def test_restatement_matches_torch(name):
    c = K.BY_NAME[name]
    x, w, b, res = K.inputs(name)
    ref, S, e32 = K.reference(name)
    got = torch_case(c, x, w, b, res)
    assert got.shape == ref.shape
    assert (S > 0).all() and np.isfinite(S).all()
    assert R.worst(got, ref, S) < 1e-13, "the float64 restatement and torch differ by more than float64 rounding"
    print(f"{name}: e32 {e32:.3e} = {e32 / R.ULP:.2f} ulp")
    assert 0 < e32 < E32_CAP, e32


def test_views_cover_what_they_should():
    c = K.BY_NAME["vr-3x3-s2-act1"]
    y = np.arange(c["B"] * 4 * 5 * c["ldy"], dtype=np.float32)
    v, own = K.y_view(c, y)
    assert v.shape == (2, 4, 5, 16) and own.sum() == v.size and v[0, 0, 0, 0] == 8 and v[1, 3, 4, 15] == y.size - 40 + 8 + 15
    c = K.BY_NAME["gg-batch-gaps"]
    v, own = K.y_view(c, np.zeros(c["B"] * (3 * 7 * 32 + 32), np.float32))
    assert own.reshape(3, -1)[:, -32:].sum() == 0 and own.sum() == v.size


def test_error_measure_counts_nan_as_infinite():
    ref, S = np.ones((2, 3)), np.full((2, 3), 2.0)
    got = ref.copy()
    got[1, 2] = 1.5
    assert R.worst(got, ref, S) == 0.25
    got[0, 0] = np.nan
    assert R.worst(got, ref, S) == np.inf
    assert R.bar(0.0) == 8 * 2.0 ** -23 and R.bar(1e-6, "f16x3") == 8e-6 and R.bar(0.0, "f16x3") == 8 * (2.0 ** -23 + 2.0 ** -22)


@pytest.mark.parametrize("case", K.DCONV + K.DCONV_OFF30, ids=lambda c: "-".join(str(v) for v in c))
def test_dconv_restatement_matches_the_oracle(case):
    B, O, I, C, hid, along_outer, d, off = case
    y, p = K.dconv_inputs(*case)
    out, S, h, Sh, e32, e32h = K.dconv_reference(*case)
    # the oracle's DConv runs layers 0 .. d with dilation 2^layer: layers before d get a zero LayerScale (x + 0 y = x exactly)
    sd = {}
    for l in range(d + 1):
        q = f"dc.layers.{l}"
        z = 0.0 if l < d else 1.0
        sd.update({f"{q}.0.weight": t64(p["w1"]), f"{q}.0.bias": t64(p["b1"]), f"{q}.1.weight": t64(p["g1w"]), f"{q}.1.bias": t64(p["g1b"]),
                   f"{q}.3.weight": t64(p["w2"])[:, :, None], f"{q}.3.bias": t64(p["b2"]), f"{q}.4.weight": t64(p["g2w"]),
                   f"{q}.4.bias": t64(p["g2b"]), f"{q}.6.scale": z * t64(p["ls"])})
    # sequences [N, C, T]: (b, i) over o for the spectrogram branch (hdemucs.py:152-158), b over i for the waveform
    seq = t64(y).permute(0, 2, 3, 1).reshape(B * I, C, O) if along_outer else t64(y)[:, 0].permute(0, 2, 1)
    got = DO._dconv(seq, sd, "dc", types.SimpleNamespace(dconv_depth=d + 1))
    got = got.reshape(B, I, C, O).permute(0, 3, 1, 2) if along_outer else got.permute(0, 2, 1)[:, None]
    assert R.worst(got.numpy(), out, S) < 1e-12
    # h against the same composition's first half
    q = f"dc.layers.{d}"
    hh = F.gelu(F.group_norm(F.conv1d(seq, sd[f"{q}.0.weight"], sd[f"{q}.0.bias"], dilation=2 ** d, padding=2 ** d), 1, sd[f"{q}.1.weight"],
                             sd[f"{q}.1.bias"]))
    hh = hh.reshape(B, I, hid, O).permute(0, 3, 1, 2) if along_outer else hh.permute(0, 2, 1)[:, None]
    assert R.worst(hh.numpy(), h, Sh) < 1e-12
    # and the two halves chain: the tail from the reference's own h is the whole layer
    out2, _ = R.dconv_tail(y, h, Sh, p, along_outer)
    assert np.array_equal(out2, out)
    print(f"dconv {case}: e32 {e32:.3e} ({e32 / R.ULP:.2f} ulp), h {e32h:.3e}")
    assert np.isfinite(e32) and np.isfinite(e32h)
