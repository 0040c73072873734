"""Plain numpy restatements of the gathered convolutions of the channels-last nets (asx_op_gconv / asx_op_dconv, include/asx.h):
strided and dilated convolution, GLU, ConvTranspose with crop, residual (also through a `res_mod` table), the activations of
tdf_act, and the DConv layer of demucs.py:99-179.  Channels-last in and out.  Every function takes the dtype it computes in:
float64 is the reference, float32 the "plain fp32 evaluation" whose own error sets the bar of tests/test_gpu_gconv.py.

Per output element the functions return the value and its error scale S: S = sum |x| |w| + |b| of the pre-activation (+ |res| with a
residual); GLU: S = S_value + 0.25 |value| S_gate (0.25 = the largest slope of the sigmoid).  The scale is always computed in float64.
GroupNorm (DConv) carries a scale through as S' = (S + |mean|) rstd |gamma| + |beta|; LayerScale and the residual as |ls| S' + |y|.
"""
import math

import numpy as np

ULP = 2.0 ** -23
# the dropped term of each arithmetic, from the option text of include/asx.h ("gemm_bf16x6", "gemm_f16x3"): fp32 MFMA none,
# bf16 x 6 2^-24, fp16 x 3 2^-22
FLOOR = {"fp32": ULP, "bf16x6": ULP + 2.0 ** -24, "f16x3": ULP + 2.0 ** -22}
MARGIN = 8.0

_erf = np.vectorize(math.erf, otypes=[np.float64])


def erf(v):
    """erf in the dtype of v (float32: the float64 value rounded once, as a correctly rounded erff gives)"""
    return _erf(v.astype(np.float64)).astype(v.dtype)


def act(v, code):
    """tdf_act of csrc/kernels_net.h: 0 none, 1 relu, 2 / 6 gelu (erf), 3 tanh, 4 leaky relu 0.01, 5 sigmoid"""
    t = v.dtype.type
    if code == 1:
        return np.maximum(v, t(0))
    if code in (2, 6):
        return t(0.5) * v * (t(1) + erf(v * t(0.70710678118654752440)))
    if code == 3:
        return np.tanh(v)
    if code == 4:
        return np.where(v > 0, v, t(0.01) * v)
    if code == 5:
        return t(1) / (t(1) + np.exp(-v))
    return v


def sigmoid(v):
    t = v.dtype.type
    return t(1) / (t(1) + np.exp(-v))


def _gather(x, to, ti, g):
    """x [B, O, I, C] -> the tap (to, ti) of every output pixel [B, OR, IR, C], zero outside the image"""
    B, O, I, C = x.shape
    OR, IR = g.get("OR") or O, g["IR"]
    o = np.arange(OR) * g.get("SO", 1) - g.get("PO", 0) + to * g.get("DO", 1)
    i = np.arange(IR) * g.get("SI", 1) - g.get("PI", 0) + ti * g.get("DI", 1)
    ok = ((o >= 0) & (o < O))[:, None] & ((i >= 0) & (i < I))[None, :]
    t = x[:, np.clip(o, 0, O - 1)][:, :, np.clip(i, 0, I - 1)]
    return t * ok[None, :, :, None].astype(x.dtype)


def conv_pre(x, w, b, g, dtype=np.float64):
    """pre-activation of the gathered convolution: x [B, O, I, Cin], w [N, Cin, KI, KO] (torch layout with the INNER kernel axis
    first), b [N]; g: dict of KO KI DO DI PO PI SO SI OR IR.  Returns (v, S) [B, OR, IR, N]."""
    taps = [(to, ti) for to in range(g.get("KO", 1)) for ti in range(g.get("KI", 1))]

    def rows_times_weights(xs, ws):
        # every output pixel's taps side by side [B, OR, IR, taps * Cin], one matrix product with the weights laid out alike
        col = np.concatenate([_gather(xs, to, ti, g) for to, ti in taps], axis=-1)
        return col @ np.concatenate([ws[:, :, ti, to] for to, ti in taps], axis=1).T

    v = rows_times_weights(x.astype(dtype), w.astype(dtype)) + b.astype(dtype)
    S = rows_times_weights(np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))) + np.abs(b.astype(np.float64))
    return v, S


def _res_rows(res, shape, res_mod, dtype):
    """res [rows, C] (or the table [res_mod, C] read at row % res_mod) -> shape [..., C]"""
    rows = int(np.prod(shape[:-1]))
    r = res[np.arange(rows) % res_mod] if res_mod else res
    return r.reshape(shape).astype(dtype)


def conv_dense(x, w, b, g, a=0, res=None, res_mod=0, dtype=np.float64):
    v, S = conv_pre(x, w, b, g, dtype)
    y = act(v, a)
    if res is not None:
        y = y + _res_rows(res, y.shape, res_mod, dtype)
        S = S + np.abs(_res_rows(res, y.shape, res_mod, np.float64))
    return y, S


def conv_glu(x, w, b, g, res=None, res_mod=0, dtype=np.float64):
    """w [2 C, Cin, KI, KO]: rows [0, C) the values, [C, 2 C) the gates (torch's F.glu over channels)"""
    v, S = conv_pre(x, w, b, g, dtype)
    C = v.shape[-1] // 2
    val, gate = v[..., :C], v[..., C:]
    y = val * sigmoid(gate)
    S = S[..., :C] + 0.25 * np.abs(val.astype(np.float64)) * S[..., C:]
    if res is not None:
        y = y + _res_rows(res, y.shape, res_mod, dtype)
        S = S + np.abs(_res_rows(res, y.shape, res_mod, np.float64))
    return y, S


def conv_transpose(x, w, b, So, crop, Iout, a=0, res=None, dtype=np.float64):
    """ConvTranspose along the inner axis: x [B, O, I, Cin], w [Cin, Cout, 2 So] (torch), stride So; full[i So + k] += x[i] w[:, :, k],
    y = act(full[crop : crop + Iout] + b) (+ res [B, O, Iout, Cout]).  Returns (y, S) [B, O, Iout, Cout]."""
    B, O, I, Cin = x.shape
    Cout, K = w.shape[1], w.shape[2]
    assert K == 2 * So and crop + Iout <= (I + 1) * So
    xd, wd = x.astype(dtype), w.astype(dtype)
    xa, wa = np.abs(x.astype(np.float64)), np.abs(w.astype(np.float64))
    full = np.zeros((B, O, (I + 1) * So, Cout), dtype)
    Sf = np.zeros((B, O, (I + 1) * So, Cout), np.float64)
    # output position p = i So + k gets exactly two terms: (i, k) = (p // So, p % So) and (p // So - 1, p % So + So); the older input first
    for k in list(range(So, K)) + list(range(So)):
        full[:, :, k:k + I * So:So] += xd @ wd[:, :, k]
        Sf[:, :, k:k + I * So:So] += xa @ wa[:, :, k]
    y = act(full[:, :, crop:crop + Iout] + b.astype(dtype), a)
    S = Sf[:, :, crop:crop + Iout] + np.abs(b.astype(np.float64))
    if res is not None:
        y = y + res.reshape(y.shape).astype(dtype)
        S = S + np.abs(res.reshape(y.shape).astype(np.float64))
    return y, S


def _group_norm(v, S, gamma, beta, axes, dtype, eps=1e-5):
    """GroupNorm(1, C) of v over `axes` (two-pass statistics in dtype), and the scale carried through"""
    t = dtype
    mean = v.mean(axis=axes, keepdims=True, dtype=dtype)
    var = ((v - mean) ** 2).mean(axis=axes, keepdims=True, dtype=dtype)
    rstd = t(1) / np.sqrt(var + t(eps))
    y = (v - mean) * rstd * gamma.astype(dtype) + beta.astype(dtype)
    S2 = (S + np.abs(mean.astype(np.float64))) * rstd.astype(np.float64) * np.abs(gamma.astype(np.float64)) + np.abs(beta.astype(np.float64))
    return y, S2


def dconv_head(y, p, along_outer, d, dtype=np.float64):
    """First half of one DConv layer (demucs.py:99-179) on y [B, O, I, C] channels-last: conv k3 with dilation 2^d (over O when
    along_outer -- one sequence per (b, i), as the spectrogram branch folds frequency into the batch -- else over I with O == 1),
    GroupNorm(1, hid), GELU.  p: w1 [hid, C, 3], b1, g1w, g1b [hid].  Returns (h, S_h) [B, O, I, hid]."""
    B, O, I, C = y.shape
    dil = 1 << d
    assert along_outer or O == 1
    w1 = p["w1"].reshape(-1, C, 3)
    if along_outer:
        g = dict(KO=3, DO=dil, PO=dil, IR=I)
        w1 = w1[:, :, None, :]           # [hid, C, KI = 1, KO = 3]
    else:
        g = dict(KI=3, DI=dil, PI=dil, IR=I)
        w1 = w1[:, :, :, None]
    v, S = conv_pre(y, w1, p["b1"], g, dtype)
    v, S = _group_norm(v, S, p["g1w"], p["g1b"], (1, 3) if along_outer else (1, 2, 3), dtype)
    return act(v, 2), S


def dconv_tail(y, h, Sh, p, along_outer, dtype=np.float64):
    """Second half: conv 1x1 of h [B, O, I, hid], GroupNorm(1, 2 C), GLU, LayerScale, + y.  p: w2 [2 C, hid], b2, g2w, g2b [2 C],
    ls [C].  Sh: the scale h arrives with (None: h is exact input, |h|).  Returns (y_out, S_out)."""
    C = y.shape[-1]
    hid = h.shape[-1]
    w2 = p["w2"].reshape(2 * C, hid)
    z = h.astype(dtype) @ w2.astype(dtype).T + p["b2"].astype(dtype)
    Sz = (np.abs(h.astype(np.float64)) if Sh is None else Sh) @ np.abs(w2.astype(np.float64)).T + np.abs(p["b2"].astype(np.float64))
    z, Sz = _group_norm(z, Sz, p["g2w"], p["g2b"], (1, 3) if along_outer else (1, 2, 3), dtype)
    val, gate = z[..., :C], z[..., C:]
    Sg = Sz[..., :C] + 0.25 * np.abs(val.astype(np.float64)) * Sz[..., C:]
    out = y.astype(dtype) + p["ls"].astype(dtype) * (val * sigmoid(gate))
    return out, np.abs(y.astype(np.float64)) + np.abs(p["ls"].astype(np.float64)) * Sg


def dconv_layer(y, p, along_outer, d, dtype=np.float64):
    """both halves: (y_out, S_out, h, S_h)"""
    h, Sh = dconv_head(y, p, along_outer, d, dtype)
    out, S = dconv_tail(y, h, Sh, p, along_outer, dtype)
    return out, S, h, Sh


def worst(got, ref, S):
    """the worst element of |got - ref| / S; NaN (or an infinity) counts as infinite"""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - ref) / S).max())


def bar(e32, arith="fp32"):
    return MARGIN * max(e32, FLOOR[arith])
