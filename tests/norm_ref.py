"""Float64 evaluations of the normalisation and statistics launches on their float32 inputs, the error measure the per-launch tests
share, and torch's fp32 evaluation of the same operations (the e32 of the bar).  The formulas are the reference's:
  RMSNorm (bs_roformer.py:42-52)                 x / max(||x||, 1e-12) sqrt(d) gamma
  LayerNorm / GroupNorm / InstanceNorm           (x - mean) / sqrt(var + 1e-5) gamma + beta, biased variance, eps inside the root
  Demucs standardisation (htdemucs.py:511-519)   (x - mean) / (1e-5 + std), unbiased std
  HDemucs decoder norm (hdemucs.py:321-327)      statistics over all rin rows, output cropped to rows [r0, r0 + r)
Every evaluation returns (y64, s): s, the scale of an element, is the sum of the magnitudes of the terms that form it --
|gamma| (|x| + |mean|) rstd + |beta| before the activation ((|x| + |mean|) / (1e-5 + std) for the standardisations, |y64| for RMSNorm),
unchanged through ReLU / GELU / ELU (alpha <= 1), s_value + |value64| s_gate / 4 through the GLU, then + |res| (or + |skip|), then
times |mul|.  measure() is the worst element of |got - y64| / s, NaN counting as infinite; elements with s = 0 must be exact zeros and
are counted apart."""
import math

import numpy as np

EPS = 1e-5
U32 = 2.0 ** -23
_erf = np.frompyfunc(math.erf, 1, 1)


def f64(a):
    return np.asarray(a, np.float64)


# ---- the measure -----------------------------------------------------------------------------------------------------------------
def measure(got, ref, s):
    """(worst |got - ref| / s over the elements with s > 0, how many elements with s == 0 are not exact zeros)"""
    got, ref, s = f64(got), f64(ref), f64(s)
    assert got.shape == ref.shape == s.shape, (got.shape, ref.shape, s.shape)
    own = s > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.abs(got - ref)[own] / s[own]
    e = np.where(np.isfinite(e), e, np.inf)
    return (float(e.max()) if e.size else 0.0), int(np.count_nonzero(got[~own] != 0))   # NaN != 0


def bar(e32):
    return 8.0 * max(e32, U32)


# ---- activations, written out in float64 ------------------------------------------------------------------------------------------------
def gelu(v):
    return 0.5 * v * (1.0 + _erf(v * math.sqrt(0.5)).astype(np.float64))


def elu(v, alpha):
    return np.where(v > 0, v, alpha * np.expm1(np.minimum(v, 0.0)))


def glu(v, s, axis):
    """value * sigmoid(gate) over the halves of `axis`; s = s_value + |value| s_gate / 4 (the sigmoid's slope is at most 1 / 4)"""
    a, g = np.split(v, 2, axis=axis)
    sa, sg = np.split(s, 2, axis=axis)
    return a / (1.0 + np.exp(-g)), sa + np.abs(a) * sg / 4.0


def act(v, kind, alpha=1.0):
    if kind in (None, "none"):
        return v
    if kind == "relu":
        return np.maximum(v, 0.0)
    if kind == "gelu":
        return gelu(v)
    assert kind == "elu" and alpha <= 1.0, (kind, alpha)
    return elu(v, alpha)


def _affine(x, mean, rstd, gamma, beta):
    """(x - mean) rstd gamma + beta and its scale, all arguments broadcast against x"""
    return (x - mean) * rstd * gamma + beta, np.abs(gamma) * (np.abs(x) + np.abs(mean)) * rstd + np.abs(beta)


def _moments(x, axes):
    mean = x.mean(axis=axes, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=axes, keepdims=True)          # biased
    return mean, 1.0 / np.sqrt(var + EPS)


# ---- rows -----------------------------------------------------------------------------------------------------------------------
def rms(x, gamma):
    """x [M, d] -> y [M, d]"""
    x, gamma = f64(x), f64(gamma)
    n = np.sqrt((x * x).sum(axis=1, keepdims=True))
    y = x / np.maximum(n, 1e-12) * math.sqrt(x.shape[1]) * gamma
    return y, np.abs(y)


def rms_factor(x):
    x = f64(x)
    r = math.sqrt(x.shape[1]) / np.maximum(np.sqrt((x * x).sum(axis=1)), 1e-12)
    return r, np.abs(r)


def layer(x, gamma, beta, pos=None):
    """LayerNorm over the columns of x [M, C] (+ pos[row % pos_mod] after the affine, transformer.py:528,536)"""
    x = f64(x)
    mean, rstd = _moments(x, 1)
    y, s = _affine(x, mean, rstd, f64(gamma), f64(beta))
    if pos is not None:
        p = f64(pos)[np.arange(x.shape[0]) % len(pos)]
        y, s = y + p, s + np.abs(p)
    return y, s


# ---- statistics --------------------------------------------------------------------------------------------------------------------
def group_sums(x, gdiv, ld, cn, g2):
    """ht_stats over x [G1, R, P]: plane element i belongs to group i // gdiv and counts when i % ld < cn.  Returns the float64 sums
    [G1, g2, 2] = (sum, sum of squares) and their bounds n 2^-53 (sum |v|, sum v^2): the worst case of a float64 sum of n terms in any
    order (the squares of floats are exact in double)."""
    x = f64(x)
    G1, R, P = x.shape
    i = np.arange(P)
    sums, bound = np.zeros((G1, g2, 2)), np.zeros((G1, g2, 2))
    for g in range(g2):
        sel = (i // gdiv == g) & (i % ld < cn)
        v = x[:, :, sel].reshape(G1, -1)
        n = v.shape[1]
        sums[:, g, 0], sums[:, g, 1] = [math.fsum(r) for r in v], [math.fsum(r) for r in v * v]
        bound[:, g, 0], bound[:, g, 1] = n * 2.0 ** -53 * np.abs(v).sum(axis=1), n * 2.0 ** -53 * (v * v).sum(axis=1)
    return sums, bound


# ---- group norms -------------------------------------------------------------------------------------------------------------------
def ht_norm_out(x, gamma, beta):
    """MyGroupNorm(1, C) of HTDemucs: x [B, N, C], statistics per item over (N, C)"""
    x = f64(x)
    mean, rstd = _moments(x, (1, 2))
    return _affine(x, mean, rstd, f64(gamma), f64(beta))


def hd_group_norm(x, G, gamma, beta, mode, r0=0, R=None, skip=None, crop_stats=False):
    """GroupNorm(G, C) over x [B, Rin, C] channels-last, statistics over all Rin rows, output rows [r0, r0 + R); mode "gelu" / "glu" /
    "none"; the skip is added last.  crop_stats: the WRONG formula that takes the statistics of the kept rows only (for the host test)."""
    x = f64(x)
    B, Rin, C = x.shape
    R = Rin if R is None else R
    xs = x[:, r0:r0 + R] if crop_stats else x
    mean, rstd = _moments(xs.reshape(B, xs.shape[1], G, C // G), (1, 3))
    xc = x[:, r0:r0 + R].reshape(B, R, G, C // G)
    v, s = _affine(xc, mean, rstd, f64(gamma).reshape(G, C // G), f64(beta).reshape(G, C // G))
    v, s = v.reshape(B, R, C), s.reshape(B, R, C)
    if mode == "glu":
        v, s = glu(v, s, 2)
    else:
        v = act(v, mode)
    if skip is not None:
        v, s = v + f64(skip), s + np.abs(f64(skip))
    return v, s


def standardize(x, biased=False, eps_inside=False):
    """(x - mean) / (1e-5 + std) per item over everything else, std unbiased.  biased / eps_inside: WRONG formulas for the host test."""
    x = f64(x)
    ax = tuple(range(1, x.ndim))
    n = x[0].size
    mean = x.mean(axis=ax, keepdims=True)
    var = ((x - mean) ** 2).sum(axis=ax, keepdims=True) / (n if biased else n - 1)
    den = np.sqrt(var + EPS) if eps_inside else EPS + np.sqrt(var)
    return (x - mean) / den, (np.abs(x) + np.abs(mean)) / den


def time_norm(seg, pad_even=False):
    """seg [B, 2, L] -> [B, L (rounded up to even when pad_even, the pad sample zero with s = 0), 2]"""
    y, s = standardize(seg)
    y, s = y.transpose(0, 2, 1), s.transpose(0, 2, 1)
    if pad_even and y.shape[1] % 2:
        z = np.zeros((y.shape[0], 1, 2))
        y, s = np.concatenate([y, z], 1), np.concatenate([s, z], 1)
    return np.ascontiguousarray(y), np.ascontiguousarray(s)


def v3_norm_act(x, norm, gamma, beta, kind, alpha=1.0, unbiased=False, eps_outside=False):
    """norm -> act of TFC-TDF v3 on x [B, C, P]: norm None / "InstanceNorm" / "BatchNorm" (gamma, beta = the folded scale, shift) /
    "GroupNorm<g>".  Returns (y, s, stats [B, C, 2] = (mean, rstd) or None).  unbiased / eps_outside: WRONG formulas for the host test."""
    x = f64(x)
    B, C, P = x.shape
    stats = None
    if norm is None:
        v, s = x, np.abs(x)
    elif norm == "BatchNorm":
        g, b = f64(gamma)[:, None], f64(beta)[:, None]
        v, s = x * g + b, np.abs(x) * np.abs(g) + np.abs(b)
    else:
        G = C if norm == "InstanceNorm" else int(norm[9:])
        xg = x.reshape(B, G, -1)
        mean = xg.mean(axis=2, keepdims=True)
        n = xg.shape[2]
        var = ((xg - mean) ** 2).sum(axis=2, keepdims=True) / (n - 1 if unbiased else n)
        rstd = 1.0 / (np.sqrt(var) + EPS) if eps_outside else 1.0 / np.sqrt(var + EPS)
        mean, rstd = (np.repeat(a, C // G, axis=1).reshape(B, C, 1) for a in (mean, rstd))
        v, s = _affine(x, mean, rstd, f64(gamma)[:, None], f64(beta)[:, None])
        stats = np.concatenate([mean, rstd], axis=2)
    return act(v, kind, alpha), s, stats


def mdx_group_norm(x, gamma, beta, res=None, mul=None):
    """GroupNorm(2, C) over x [B, C, P], ReLU, then + res, then * mul (mdxnet.py:48-49, 113; modules.py:74)"""
    y, s, _ = v3_norm_act(x, "GroupNorm2", gamma, beta, "relu")
    if res is not None:
        y, s = y + f64(res), s + np.abs(f64(res))
    if mul is not None:
        y, s = y * f64(mul), s * np.abs(f64(mul))
    return y, s


# ---- torch, in the dtype of its arguments (float32: the e32 of the bar; float64: what the host test pins the above to) ----------------
def _t(a, dt):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt)


def _t_act(v, kind, alpha):
    import torch.nn.functional as F
    return v if kind in (None, "none") else F.relu(v) if kind == "relu" else F.gelu(v) if kind == "gelu" else F.elu(v, alpha)


def torch_eval(op, dt, **a):
    """the operation `op` of a case (tests/norm_cases.py) by torch's own functions in dtype dt, as a float64 array"""
    import torch
    import torch.nn.functional as F
    x, g, b = _t(a["x"], dt), _t(a.get("gamma"), dt), _t(a.get("beta"), dt)
    if op == "rms":
        y = F.normalize(x, dim=-1) * x.shape[1] ** 0.5 * g
    elif op == "rms_factor":
        y = x.shape[1] ** 0.5 / x.norm(dim=-1).clamp(min=1e-12)
    elif op == "layer":
        y = F.layer_norm(x, (x.shape[1],), g, b, EPS)
        if a.get("pos") is not None:
            p = _t(a["pos"], dt)
            y = y + p[torch.arange(x.shape[0]) % p.shape[0]]
    elif op == "ht":
        y = F.group_norm(x.permute(0, 2, 1), 1, g, b, EPS).permute(0, 2, 1)
    elif op == "hd":
        r0, R = a.get("r0", 0), a.get("R") or x.shape[1]
        y = F.group_norm(x.permute(0, 2, 1), a["G"], g, b, EPS)[:, :, r0:r0 + R]
        y = F.glu(y, dim=1) if a["mode"] == "glu" else _t_act(y, a["mode"], 1.0)
        y = y.permute(0, 2, 1)
        if a.get("skip") is not None:
            y = y + _t(a["skip"], dt)
    elif op in ("std", "time", "hd_time"):
        ax = tuple(range(1, x.ndim))
        y = (x - x.mean(dim=ax, keepdim=True)) / (1e-5 + x.std(dim=ax, keepdim=True))
        if op != "std":
            y = y.permute(0, 2, 1)
            if op == "hd_time" and y.shape[1] % 2:
                y = F.pad(y, (0, 0, 0, 1))
    elif op in ("v3", "mdx"):
        norm = a["norm"] if op == "v3" else "GroupNorm2"
        if norm is None:
            y = x
        elif norm == "BatchNorm":
            y = x * g[:, None] + b[:, None]
        elif norm == "InstanceNorm":
            y = F.instance_norm(x, weight=g, bias=b, eps=EPS)
        else:
            y = F.group_norm(x, int(norm[9:]), g, b, EPS)
        y = _t_act(y, a["act"] if op == "v3" else "relu", a.get("alpha", 1.0))
        if a.get("res") is not None:
            y = y + _t(a["res"], dt)
        if a.get("mul") is not None:
            y = y * _t(a["mul"], dt)
    else:
        raise KeyError(op)
    return y.contiguous().double().numpy()


def ref_eval(op, **a):
    """the float64 evaluation of the same case: (y64, s)"""
    if op == "rms":
        return rms(a["x"], a["gamma"])
    if op == "rms_factor":
        return rms_factor(a["x"])
    if op == "layer":
        return layer(a["x"], a["gamma"], a["beta"], a.get("pos"))
    if op == "ht":
        return ht_norm_out(a["x"], a["gamma"], a["beta"])
    if op == "hd":
        return hd_group_norm(a["x"], a["G"], a["gamma"], a["beta"], a["mode"], a.get("r0", 0), a.get("R"), a.get("skip"))
    if op == "std":
        return standardize(a["x"])
    if op in ("time", "hd_time"):
        return time_norm(a["x"], op == "hd_time")
    if op == "v3":
        return v3_norm_act(a["x"], a["norm"], a.get("gamma"), a.get("beta"), a["act"], a.get("alpha", 1.0))[:2]
    if op == "mdx":
        return mdx_group_norm(a["x"], a["gamma"], a["beta"], a.get("res"), a.get("mul"))
    raise KeyError(op)
