"""The cases of tests/test_gpu_norm_kernels.py and tests/test_host_norm_ref.py: the smallest shapes that reach every path of the
normalisation and statistics launches (include/asx.h: asx_op_rownorm, asx_op_group_stats, asx_op_group_norm), each a few hundred KB
at most.  Every family gets four inputs: standard normal ("n"), the same shifted by 1024 standard deviations ("shift": a variance
formed in fp32 is off by about 2^4 x the bar), the same scaled by 2^-10 ("small": eps dominates the variance) and one constant
group ("const": a variance of exactly zero).  build(name) adds the arrays, the float64 reference (y, s) and e32, the measure of
torch's fp32 evaluation of the same input on the CPU; it is cached, and nothing in it comes from a kernel."""
import functools
import zlib

import numpy as np

from tests import norm_ref as R

VARIANTS = ("n", "shift", "small", "const")
M_EDGES = (1, 3, 4, 5, 9)          # the tail of a four-rows-per-workgroup kernel
PRIME = 32771                      # a prime above 32768: 2 * PRIME floats fold to 2 rows
assert all(PRIME % k for k in range(2, 182))

ROW, STATS, GROUP = [], [], []


def _add(lst, name, **kw):
    lst.append(dict(name=name, **kw))


def _v(i):
    return VARIANTS[i % 4]


# ---- asx_op_rownorm ------------------------------------------------------------------------------------------------------------------
i = 0
for d in (8, 72, 100, 384, 513):
    for M in M_EDGES:
        _add(ROW, f"rms-d{d}-M{M}-{_v(i)}", op="rms", M=M, d=d, variant=_v(i))
        i += 1
for v in VARIANTS:
    _add(ROW, f"rms-pad-d100-M5-{v}", op="rms", M=5, d=100, lda=104, ldy=108, variant=v)      # pad columns keep their NaN fill
_add(ROW, "rms-inplace-d384-M9", op="rms", M=9, d=384, variant="n", in_place=True)
_add(ROW, "rms-inplace-pad-d100-M5", op="rms", M=5, d=100, lda=104, ldy=104, variant="shift", in_place=True)
_add(ROW, "rms-zero-row-d72-M5", op="rms", M=5, d=72, variant="n", zero_row=2)
i = 0
for C in (4, 100, 384, 512):
    for M in M_EDGES:
        _add(ROW, f"layer-C{C}-M{M}-{_v(i)}", op="layer", M=M, d=C, variant=_v(i))
        i += 1
for v in VARIANTS:
    _add(ROW, f"layer-every-C100-M6-{v}", op="layer", M=6, d=100, variant=v)
for pm in (1, 3, 7):
    _add(ROW, f"layer-pos{pm}-C100-M7", op="layer", M=7, d=100, variant=_v(pm), pos_mod=pm)
_add(ROW, "layer-pos3-C384-M9", op="layer", M=9, d=384, variant="n", pos_mod=3)

# ---- asx_op_group_stats: (G1, R, P, gdiv, ld, cn, g2) --------------------------------------------------------------------------------
i = 0
for C, N, B in ((48, 20, 2), (384, 20, 2), (48, 200, 2), (384, 200, 1)):                     # norm_out; N = 200: two row slices
    _add(STATS, f"stats-normout-C{C}-N{N}-{_v(i)}", dims=(B, N, C, C, C, C, 1), variant=_v(i))
    i += 1
for C, Rin in ((16, 7), (96, 7), (96, 200), (768, 7)):                                       # HDemucs GroupNorm(4, C); 768: a group straddles workgroups
    _add(STATS, f"stats-hd-C{C}-R{Rin}-{_v(i)}", dims=(2, Rin, C, C // 4, C, C, 4), variant=_v(i))
    i += 1
for v in VARIANTS:
    _add(STATS, f"stats-spec-T5-F128-{v}", dims=(2, 5, 512, 512, 4, 4, 1), variant=v)          # spectrogram standardisation
for n2l in (1000, 65534, 65536, 2 * PRIME):                                                   # flat waveform; 65536 folds to 256 rows
    _add(STATS, f"stats-flat-{n2l}-{_v(i)}", dims=(2, 1, n2l, n2l, 1, 1, 1), variant=_v(i))
    i += 1
_add(STATS, "stats-dconv-ld8-cn6", dims=(2, 6, 320, 8, 8, 6, 40), variant="shift")            # padded pixels, 33 groups per workgroup
_add(STATS, "stats-gdiv4-P512", dims=(2, 3, 512, 4, 4, 4, 128), variant="n")                  # 65 group slots of the 66
_add(STATS, "stats-short-plane-P200-gdiv4", dims=(2, 9, 200, 4, 4, 3, 50), variant="small")   # P < 256, one row per workgroup
# what ht_stats refuses: more than 66 group slots per workgroup
STATS_REFUSED = [(2, 3, 512, 2, 2, 2, 256), (2, 3, 512, 3, 3, 3, 171), (1, 1, 256, 1, 1, 1, 256), (2, 3, 200, 2, 2, 2, 100)]

# ---- asx_op_group_norm ---------------------------------------------------------------------------------------------------------------
i = 0
for C, N in ((48, 20), (384, 20), (48, 200)):
    _add(GROUP, f"ht-C{C}-N{N}-{_v(i)}", op="ht", shape=(2, N, C), variant=_v(i))
    i += 1
for v in VARIANTS:
    _add(GROUP, f"ht-C100-N9-{v}", op="ht", shape=(2, 9, 100), variant=v)
for C in (16, 768):
    for mode in ("gelu", "glu", "none"):
        for skip in (False, True):
            for crop in (False, True):
                _add(GROUP, f"hd-C{C}-{mode}{'-skip' if skip else ''}{'-crop' if crop else ''}-{_v(i)}", op="hd", G=4, mode=mode, skip=skip,
                     shape=(2, 11 if crop else 6, C), R=6, r0=2 if crop else 0, variant=_v(i))
                i += 1
for v in VARIANTS:
    _add(GROUP, f"hd-C96-gelu-skip-crop-{v}", op="hd", G=4, mode="gelu", skip=True, shape=(2, 11, 96), R=6, r0=2, variant=v)
_add(GROUP, "hd-C16-gelu-inplace", op="hd", G=4, mode="gelu", skip=False, shape=(2, 6, 16), R=6, r0=0, variant="n", in_place=True)
_add(GROUP, "hd-C768-none-skip-inplace", op="hd", G=4, mode="none", skip=True, shape=(2, 6, 768), R=6, r0=0, variant="shift", in_place=True)
for T, c in ((5, 512), (1, 4), (3, 252)):
    for v in VARIANTS:
        _add(GROUP, f"std-T{T}-c{c}-{v}", op="std", shape=(2, T, c), variant=v)
for L in (2, 255, 256, 1001):
    for v in VARIANTS:
        _add(GROUP, f"time-L{L}-{v}", op="time", shape=(2, 2, L), variant=v)
for L in (2, 3, 255, 256, 1001):
    for v in VARIANTS:
        _add(GROUP, f"hd_time-L{L}-{v}", op="hd_time", shape=(2, 2, L), variant=v)
i = 0
for norm in (None, "InstanceNorm", "BatchNorm", "GroupNorm1", "GroupNorm2", "GroupNorm4"):
    for act, alpha in (("relu", 1.0), ("gelu", 1.0), ("elu", 0.5), ("elu", 1.0)):
        for P in (64, 1001):
            _add(GROUP, f"v3-{norm}-{act}{alpha if act == 'elu' else ''}-P{P}-{_v(i)}", op="v3", norm=norm, act=act, alpha=alpha, shape=(2, 8, P),
                 variant=_v(i))
            i += 1
for norm in ("InstanceNorm", "GroupNorm2", "BatchNorm", None):
    for P in (64, 1001):                                                                      # channels [3, 11) of 13
        _add(GROUP, f"v3-view-{norm}-P{P}-{_v(i)}", op="v3", norm=norm, act="gelu", alpha=1.0, shape=(2, 8, P), ctot=13, c0=3, variant=_v(i))
        i += 1
for P in (4096, 4097):                                                                        # 32768 floats per group: two slices of v3_gn_splits
    for v in ("n", "shift"):
        _add(GROUP, f"v3-GroupNorm1-split-P{P}-{v}", op="v3", norm="GroupNorm1", act="relu", alpha=1.0, shape=(2, 8, P), variant=v, splits=2)
for C in (8, 48):
    for P in (64, 1001):
        for extra in ("plain", "res", "mul", "res-mul"):
            for inp in (False, True):
                _add(GROUP, f"mdx-C{C}-P{P}-{extra}{'-inplace' if inp else ''}-{_v(i)}", op="mdx", shape=(2, C, P), res="res" in extra,
                     mul="mul" in extra, in_place=inp, variant=_v(i))
                i += 1
del i

BY_NAME = {c["name"]: c for c in ROW + STATS + GROUP}
assert len(BY_NAME) == len(ROW) + len(STATS) + len(GROUP)


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _vary(x, variant, const_index):
    """the case's input from standard normal x; const_index: the index expression of the group made constant"""
    if variant == "shift":
        x = x + 1024.0
    elif variant == "small":
        x = x * 2.0 ** -10
    x = x.astype(np.float32)
    if variant == "const":
        x[const_index] = np.float32(3.0)
    return x


def _affine(rng, C):
    return (1.0 + 0.5 * rng.standard_normal(C)).astype(np.float32), (0.5 * rng.standard_normal(C)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def build(name):
    c = BY_NAME[name]
    rng = _rng(name)
    d = {}
    if c in STATS:
        G1, Rr, P, gdiv, ld, cn, g2 = c["dims"]
        x = rng.standard_normal((G1, Rr, P))
        const = (0, slice(None), slice(0, min(gdiv, P)))                                       # group 0 of item 0
        d["x"] = _vary(x, c["variant"], const)
        d["sums"], d["bound"] = R.group_sums(d["x"], gdiv, ld, cn, g2)
        return d
    op = c["op"]
    if c in ROW:
        M, dd = c["M"], c["d"]
        d["x"] = _vary(rng.standard_normal((M, dd)), c["variant"], (M // 2,))                   # one constant row
        if "zero_row" in c:
            d["x"][c["zero_row"]] = 0.0
        d["gamma"], d["beta"] = _affine(rng, dd)
        if op == "rms":
            del d["beta"]
        if c.get("pos_mod"):
            d["pos"] = rng.standard_normal((c["pos_mod"], dd)).astype(np.float32)
    else:
        shape = c["shape"]
        x = rng.standard_normal(shape)
        if op in ("std", "time", "hd_time"):
            # s has the floor |mean| / (1e-5 + std), so against an item whose sample mean is far below its standard error n^-1/2 the
            # measure is one of the absolute error of a mean formed in fp32 (e32 of such draws: 5 .. 55 x 2^-23): they are redrawn
            for it in x:
                while abs(it.mean()) < it.size ** -0.5:
                    it[...] = rng.standard_normal(it.shape)
        if op in ("ht", "std", "time", "hd_time"):
            const = (1,)                                                                       # item 1 (the group is the item)
        elif op == "hd":
            const = (1, slice(None), slice(0, shape[2] // c["G"]))                             # group 0 of item 1, cropped rows included
        else:
            G = {None: 0, "BatchNorm": 0, "InstanceNorm": shape[1]}.get(c.get("norm", "GroupNorm2"), None)
            G = int(c.get("norm", "GroupNorm2")[9:]) if G is None else G
            const = (1, slice(0, shape[1] // G)) if G else (1, 0)
        d["x"] = _vary(x, c["variant"], const)
        if op in ("time", "hd_time", "std") and c["variant"] == "shift":
            d["x"] = x.astype(np.float32)
            d["x"][0] += np.float32(1024.0)                                                    # one item with a DC offset, the other without
        C = shape[1] if op in ("v3", "mdx") else shape[2]
        if op not in ("std", "time", "hd_time") and not (op == "v3" and c["norm"] is None):
            d["gamma"], d["beta"] = _affine(rng, C)
        if op == "hd":
            d.update(G=c["G"], mode=c["mode"], r0=c["r0"], R=c["R"])
            if c["skip"]:
                d["skip"] = rng.standard_normal((shape[0], c["R"], C // 2 if c["mode"] == "glu" else C)).astype(np.float32)
        if op == "v3":
            d.update(norm=c["norm"], act=c["act"], alpha=c["alpha"])
        if op == "mdx":
            if c["res"]:
                d["res"] = rng.standard_normal(shape).astype(np.float32)
            if c["mul"]:
                d["mul"] = rng.standard_normal(shape).astype(np.float32)
    d["y"], d["s"] = R.ref_eval(op, **d)
    import torch
    d["e32"] = R.measure(R.torch_eval(op, torch.float32, **d), d["y"], d["s"])[0]
    if op == "rms":
        d["r"], d["r_s"] = R.rms_factor(d["x"])
        d["r_e32"] = R.measure(R.torch_eval("rms_factor", torch.float32, **d), d["r"], d["r_s"])[0]
    if op == "v3":
        d["stats"] = R.v3_norm_act(d["x"], c["norm"], d.get("gamma"), d.get("beta"), c["act"], c["alpha"])[2]
    return d


def scale_rows(d=384):
    """asx_op_rownorm's power-of-two rows: a unit-scale row u and the same row times 2^+50 and 2^-50.  |u_i| lies in [2, 2^10], so every
    square stays a normal float at 2^-50 (>= 2^-98); ||u|| 2^-50 stays above the 1e-12 = 2^-39.9 clamp only when ||u|| >= 2^10.2, and
    ||u||^2 2^100 must stay finite at 2^+50: u = 128 x (a normal sample pushed out to |.| >= 1 / 64 and clipped to 8), ||u|| ~
    128 sqrt(d) = 2^11.3, both asserted.  Powers of two pass through the squares, the sum, the root and the division exactly."""
    rng = _rng(f"scale-rows-{d}")
    u = rng.standard_normal(d)
    u = np.clip(np.sign(u) * np.maximum(np.abs(u), 2.0 ** -6), -8.0, 8.0) * 128.0
    u = u.astype(np.float32)
    assert np.abs(u).min() >= 2.0 and 2.0 ** 10.5 <= np.sqrt((u.astype(np.float64) ** 2).sum()) <= 2.0 ** 13
    x = np.stack([u, u * np.float32(2.0 ** 50), u * np.float32(2.0 ** -50)]).astype(np.float32)
    gamma = _affine(rng, d)[0]
    return x, gamma
