"""The cases of tests/test_gpu_gconv.py (and of tests/test_host_gconv_ref.py, which checks the float64 restatement of every one of
them against torch): descriptors of single ht_gg launches (asx_op_gconv, include/asx.h), their inputs, the float64 reference and
the error of the plain fp32 evaluation -- computed once per case, shared, read-only.

A case is a dict: the fields of asx_gconv_desc (left out = the binding's default), plus
  variant  what asx_op_gconv may run ("auto" / "gg" / "halo" / "gather"),
  expect   the kernel `resolved` must report (for gg also the N tile, from gg_tile below),
  res      True: a residual (with res_mod: the table), x_gap / y_gap: floats added to the dense batch strides.
"""
import functools
import zlib

import numpy as np

from tests import gconv_ref as R


def gg_tile(n, glu=False):
    """gg_tile_n of csrc/kernels_ht.h"""
    if glu and n <= 64:
        return 32
    for t in (16, 32, 48, 64):
        if n <= t:
            return t
    return 96 if -(-n // 96) * 96 < -(-n // 128) * 128 else 128


def glu_rows(c):
    return 32 * -(-c // 16)


def gg_bm(tile):
    """rows per gg_kernel workgroup under the default knobs for launches with lowai set: the narrow tiles run <NREP, 2, true> (128
    rows), the others <1, 4>, <6, 1, true>, <2, 4> (64 rows; 128 with lowai clear)"""
    return 128 if tile <= 48 else 64


def mk(name, variant="gg", expect=None, **kw):
    c = dict(name=name, variant=variant, B=1, O=1, I=1, mode="dense", act=0, KO=1, KI=1, DO=1, DI=1, PO=0, PI=0, SO=1, SI=1, OR=0,
             x_col0=0, y_col0=0, res=False, res_mod=0, Iout=0, crop=0, So=1, x_gap=0, y_gap=0, no_halo=0)
    c.update(kw)
    c.setdefault("IR", c["I"])
    c.setdefault("ldc", c["Cin"] + c["x_col0"])
    c.setdefault("ldy", c["Cout"] + c["y_col0"])
    c["expect"] = expect or variant
    return c


def k3o(d):     # k3 along the outer axis, dilation d, "same" padding
    return dict(KO=3, DO=d, PO=d)


def k3i(d):
    return dict(KI=3, DI=d, PI=d)


def k33(do=1, di=1):
    return dict(KO=3, KI=3, DO=do, DI=di, PO=do, PI=di)


# ---- gg_kernel ---------------------------------------------------------------------------------------------------------------------
GG = []
# N tiles 16 / 32 / 48 / 64 / 96 / 128, ragged last tiles (80, 100, 160, 200) and the col >= N guard; 150 rows = two 128- / three 64-row blocks
for n in (4, 16, 24, 32, 48, 64, 80, 96, 100, 128, 160, 200):
    GG.append(mk(f"gg-N{n}", O=3, I=50, Cin=64, Cout=n, act=1))
# K: 32 (the half-LDS launch), 36 and 100 (a partial last stage), 8 (a stage of one MFMA group)
GG += [mk("gg-K32", O=3, I=50, Cin=32, Cout=96), mk("gg-K32-n16", O=3, I=50, Cin=32, Cout=16),
       mk("gg-K36", O=3, I=50, Cin=12, Cout=64, **k3i(1)), mk("gg-K100", O=3, I=50, Cin=100, Cout=32),
       mk("gg-K100-taps", O=3, I=50, Cin=20, Cout=48, KI=5, PI=2), mk("gg-K8", O=3, I=50, Cin=8, Cout=128)]
# rows: M = 1, BM - 1, BM, BM + 1 for the tile's BM
for n in (16, 48, 64, 96, 128):
    bm = gg_bm(gg_tile(n))
    for m in (1, bm - 1, bm, bm + 1):
        GG.append(mk(f"gg-N{n}-M{m}", I=m, Cin=8, Cout=n, **k3i(1)))
# tile rows crossing (b, o) lines: the incremental carries of `advance`
for ir in (5, 7, 37):
    for n in (32, 64):
        GG.append(mk(f"gg-IR{ir}-N{n}", B=2, O=3, I=ir, Cin=8, Cout=n, act=2, **k33()))
GG.append(mk("gg-batch-gaps", B=3, O=3, I=7, Cin=8, Cout=32, x_gap=64, y_gap=32, **k33()))
# 128-row block counts just over knobs().gg_smallgrid = 1024 at K = 64: at most 32 flop / byte, under knobs().gg_lowai = 90, so `lowai`
# is still set and the 64-row instantiations run on a grid of that size ...
for n in (64, 96, 128):
    GG.append(mk(f"gg-grid1025-N{n}", O=1025, I=128, Cin=64, Cout=n))
# ... and the same grid at 90.8 / 96 / 98.6 flop / byte (12 channels x 3 x 6 taps, K = 216 with a partial last stage): `lowai` clear, the
# 128-row instantiations <1, 8>, <6, 2, true>, <2, 8>
for n in (64, 96, 128):
    GG.append(mk(f"gg-grid1025-K216-N{n}", O=1025, I=128, Cin=12, Cout=n, KO=3, KI=6, PO=1, PI=2, act=1, lowai=0))
# Demucs: encoder conv k8 / s4 / pad 2 along the inner axis
for cin in (4, 48):
    GG.append(mk(f"enc-k8s4-C{cin}", B=2, O=3, I=64, IR=16, Cin=cin, Cout=48, KI=8, PI=2, SI=4, act=2))
# waveform layer 0: 1001 samples as 501 pairs x 2 channels, the last pair carrying a zero sample the caller put there
GG.append(mk("enc-wave0", B=2, I=501, IR=251, Cin=4, Cout=48, KI=4, PI=1, SI=2, act=2))
# DConv k3, dilated, along either axis; O (or I) no larger than the dilation: both side taps wholly in padding
for o, i, d in ((6, 5, 1), (2, 5, 2), (5, 3, 2), (4, 3, 4), (9, 4, 4)):
    GG.append(mk(f"dconv-outer-O{o}-d{d}", B=2, O=o, I=i, Cin=48, Cout=8, **k3o(d)))
for i, d in ((37, 1), (2, 2), (19, 2), (4, 4), (50, 4)):
    GG.append(mk(f"dconv-inner-I{i}-d{d}", B=2, I=i, Cin=48, Cout=8, **k3i(d)))
# rewrite 1x1 + GLU + frequency embedding (res_mod); Cout 24 / 40: GLU padding rows and the oc >= Cout guard
for c, o, i in ((24, 3, 7), (40, 3, 7), (24, 10, 37), (40, 10, 37), (48, 4, 9)):
    GG.append(mk(f"glu-1x1-C{c}-M{2 * o * i}", B=2, O=o, I=i, Cin=c, Cout=c, mode="glu", res=True, res_mod=i))
GG += [mk("glu-1x1-nores", B=2, O=3, I=7, Cin=24, Cout=24, mode="glu"),
       mk("glu-1x1-res-rows", B=2, O=3, I=7, Cin=24, Cout=24, mode="glu", res=True),
       mk("glu-3x3", B=2, O=5, I=9, Cin=16, Cout=16, mode="glu", **k33()), mk("glu-3x3-C40", B=2, O=5, I=9, Cin=8, Cout=40, mode="glu", **k33()),
       mk("glu-k3", B=2, I=70, Cin=16, Cout=16, mode="glu", **k3i(1)), mk("glu-k3-C72", B=2, I=70, Cin=16, Cout=72, mode="glu", **k3i(1))]
# ConvTranspose k8 / s4 as two taps + scatter: with skip + GELU and bare, full length and shorter
for cout in (4, 24, 48):
    for iout, res in ((36, True), (36, False), (33, True)):
        GG.append(mk(f"convt-C{cout}-Iout{iout}{'-skip' if res else ''}", B=2, O=3, I=9, IR=10, Cin=8, Cout=cout, mode="convt", KI=2, PI=1,
                     crop=2, So=4, Iout=iout, res=res, act=2 if res else 0))
GG.append(mk("convt-1d", B=2, I=70, IR=71, Cin=16, Cout=8, mode="convt", KI=2, PI=1, crop=2, So=4, Iout=280, res=True, act=2))
# dense + residual rows (no table)
GG.append(mk("dense-res", B=2, O=3, I=7, Cin=8, Cout=24, res=True, act=1))
# VR: 3x3, stride 1 / 2, reading a channel slice of a wider tensor and writing a concat slot; act 1 (ReLU) / 4 (leaky)
VRV = dict(Cin=8, x_col0=4, ldc=16, Cout=16, y_col0=8, ldy=40)
for a in (1, 4):
    GG.append(mk(f"vr-3x3-s1-act{a}", B=2, O=8, I=10, act=a, **VRV, **k33()))
    GG.append(mk(f"vr-3x3-s2-act{a}", B=2, O=8, I=10, OR=4, IR=5, SO=2, SI=2, act=a, **VRV, **k33()))
GG += [mk("vr-dil4x2", B=2, O=4, I=8, act=1, **VRV, **k33(4, 2)), mk("vr-dil12x6", B=2, O=4, I=8, act=1, **VRV, **k33(12, 6)),
       mk("vr-1xW-k1", B=2, I=33, Cin=16, Cout=8, act=1), mk("vr-N4-sigmoid", B=2, O=4, I=9, Cin=16, Cout=4, act=5),
       mk("act3-tanh", O=3, I=7, Cin=8, Cout=16, act=3), mk("act6-fast-gelu", O=3, I=7, Cin=8, Cout=16, act=6)]
for c in GG:
    glu = c["mode"] == "glu"
    n = glu_rows(c["Cout"]) if glu else (c["So"] * c["Cout"] if c["mode"] == "convt" else c["Cout"])
    c["expect"] = ("gg", gg_tile(n, glu), c.get("lowai", 1))

# ---- the halo-tile kernel ----------------------------------------------------------------------------------------------------------
HALO = []
for i in (8, 16, 48, 49):                     # every til2 of hg_geometry for KO = 3 (blocks of 32 x 8, 16 x 16, 8 x 32, 4 x 64 pixels)
    HALO.append(mk(f"halo-3x3-I{i}", "halo", B=2, O=5, I=i, Cin=8, Cout=32, act=1, **k33()))
HALO.append(mk("halo-3x3-O37", "halo", B=1, O=37, I=8, Cin=16, Cout=32, act=4, **k33()))    # two block rows
for i in (255, 256, 257):                     # KO = 1: rows of 256 pixels
    HALO.append(mk(f"halo-k3-I{i}", "halo", B=2, I=i, Cin=8, Cout=32, act=1, **k3i(1)))
for n in (32, 64, 96, 100, 128):
    HALO.append(mk(f"halo-N{n}", "halo", B=2, O=5, I=16, Cin=16, Cout=n, act=1, **k33()))
HALO += [mk("halo-glu-C16", "halo", B=2, O=5, I=16, Cin=16, Cout=16, mode="glu", **k33()),
         mk("halo-glu-C40", "halo", B=2, O=5, I=16, Cin=16, Cout=40, mode="glu", **k33()),
         mk("halo-glu-k3", "halo", B=2, I=70, Cin=16, Cout=48, mode="glu", **k3i(1)),
         mk("halo-vr-slot", "halo", B=2, O=8, I=10, act=4, **VRV, **k33()),
         mk("halo-dil4x2", "auto", "halo", B=2, O=4, I=8, act=1, **VRV, **k33(4, 2)),
         # haloed block of (32 + 2 DO) x (8 + 2 DI) pixels: 504 at (5, 2) -- the kernel's; 528 at (6, 2) -- over 512, gg_kernel's
         mk("halo-npix504", "auto", "halo", B=2, O=6, I=8, Cin=8, Cout=32, act=1, **k33(5, 2)),
         mk("halo-npix528", "auto", ("gg", 32, 1), B=2, O=6, I=8, Cin=8, Cout=32, act=1, **k33(6, 2)),
         mk("halo-k3-npix512", "auto", "halo", B=2, I=300, Cin=8, Cout=32, act=1, **k3i(128)),
         mk("halo-k3-npix514", "auto", ("gg", 32, 1), B=2, I=300, Cin=8, Cout=32, act=1, **k3i(129)),
         mk("halo-none-loaded", "auto", ("gg", 32, 1), B=2, O=5, I=16, Cin=8, Cout=32, act=1, no_halo=1, **k33())]

# ---- GATHER mode of the split-operand row GEMM, under both arithmetics -----------------------------------------------------------------
GATHER = []
for cin in (32, 64, 48, 80):                  # 48 / 80: the partial last chunk of every tap
    GATHER.append(mk(f"gather-C{cin}", "auto", "gather", B=2, O=5, I=9, Cin=cin, Cout=48, act=1, **k33()))
GATHER += [mk("gather-C40-falls-back", "auto", ("gg", 48, 1), B=2, O=5, I=9, Cin=40, Cout=48, act=1, no_halo=1, **k33()),
           mk("gather-N40-falls-back", "auto", ("gg", 48, 1), B=2, O=5, I=9, Cin=32, Cout=40, act=1, no_halo=1, **k33()),
           mk("gather-N56", "gather", B=2, O=5, I=9, Cin=32, Cout=56, act=4, **k33()),
           mk("gather-N136", "gather", B=2, O=5, I=9, Cin=32, Cout=136, act=2, **k33()),
           mk("gather-N200", "gather", B=2, O=5, I=9, Cin=32, Cout=200, act=1, **k33()),
           mk("gather-M257", "gather", B=1, O=1, I=257, Cin=32, Cout=48, act=1, **k3i(1)),
           mk("gather-glu-N96", "auto", "gather", B=2, O=5, I=9, Cin=32, Cout=48, mode="glu", **k33()),
           mk("gather-glu-C40", "gather", B=2, O=5, I=9, Cin=32, Cout=40, mode="glu", **k33()),
           mk("gather-glu-N64-falls-back", "auto", ("gg", 32, 1), B=2, O=5, I=9, Cin=32, Cout=32, mode="glu", no_halo=1, **k33()),
           mk("gather-s2", "auto", "gather", B=2, O=8, I=10, OR=4, IR=5, SO=2, SI=2, Cin=32, Cout=48, act=1, **k33()),
           mk("gather-k8s4", "auto", "gather", B=2, O=3, I=64, IR=16, Cin=48, Cout=96, KI=8, PI=2, SI=4, act=2),
           mk("gather-taps-in-padding", "gather", B=2, O=2, I=3, Cin=32, Cout=48, act=1, **k33(2, 4)),
           mk("gather-slot", "gather", B=2, O=5, I=9, Cin=32, x_col0=8, ldc=48, Cout=48, y_col0=4, ldy=56, act=1, **k33())]

# ---- one DConv layer (asx_op_dconv): (B, O, I, C, hid, along_outer, d, offset in standard deviations of the input) -----------------------
DCONV = []
for i in (1, 15, 16, 17, 40):                 # G2 = I groups per item: the 16-group fold of rowstat_reduce_kernel and its ragged end
    DCONV.append((2, 6, i, 48, 6, True, 1, 0.0))
DCONV += [(2, 37, 17, 96, 12, True, 0, 0.0), (1, 3, 5, 48, 6, True, 2, 0.0), (2, 300, 3, 48, 6, True, 2, 0.0)]
# the waveform form, G2 = 1: R = I rows per item; 4096 x 2 rows and more take two and more workgroups and the arrival counters
DCONV += [(2, 1, 100, 48, 6, False, 0, 0.0), (2, 1, 8191, 48, 6, False, 1, 0.0), (2, 1, 8192, 48, 6, False, 1, 0.0),
          (3, 1, 20001, 96, 12, False, 2, 0.0)]
for off in (4.0, 8.0):                        # GroupNorm statistics are fp32 row sums of v and v^2: a mean of `off` deviations
    DCONV += [(2, 6, 17, 48, 6, True, 1, off), (2, 1, 8192, 48, 6, False, 1, off)]
DCONV_OFF30 = [(2, 6, 17, 48, 6, True, 1, 30.0), (2, 1, 8192, 48, 6, False, 1, 30.0)]


@functools.lru_cache(maxsize=None)
def dconv_inputs(B, O, I, C, hid, along_outer, d, off):
    """y [B, O, I, C] and the layer's torch tensors (the value ranges of oracle/demucs_oracle.py: make_ht_state), read-only"""
    rng = np.random.default_rng(zlib.crc32(repr((B, O, I, C, hid, along_outer, d, off)).encode()))
    f = lambda a: np.asarray(a, np.float32)
    y = f(rng.standard_normal((B, O, I, C)) + off)
    p = dict(w1=f(rng.standard_normal((hid, C, 3)) / np.sqrt(3 * C)), b1=f(0.05 * rng.standard_normal(hid)),
             g1w=f(0.8 + 0.4 * rng.random(hid)), g1b=f(0.1 * rng.standard_normal(hid)),
             w2=f(rng.standard_normal((2 * C, hid)) / np.sqrt(hid)), b2=f(0.05 * rng.standard_normal(2 * C)),
             g2w=f(0.8 + 0.4 * rng.random(2 * C)), g2b=f(0.1 * rng.standard_normal(2 * C)), ls=f(0.3 + 0.4 * rng.random(C)))
    for a in (y, *p.values()):
        a.setflags(write=False)
    return y, p


@functools.lru_cache(maxsize=None)
def dconv_reference(*case):
    """float64 (y_out, S, h, S_h) and the worst scaled errors (e32 of y_out, e32 of h) of the plain fp32 evaluation"""
    y, p = dconv_inputs(*case)
    along_outer, d = case[5], case[6]
    out, S, h, Sh = R.dconv_layer(y, p, along_outer, d, np.float64)
    o32, _, h32, _ = R.dconv_layer(y, p, along_outer, d, np.float32)
    for a in (out, S, h, Sh):
        a.setflags(write=False)
    return out, S, h, Sh, R.worst(o32, out, S), R.worst(h32, h, Sh)


BY_NAME = {c["name"]: c for c in GG + HALO + GATHER}
assert len(BY_NAME) == len(GG) + len(HALO) + len(GATHER)


def desc(c):
    """the keyword arguments of Engine.op_gconv"""
    keys = ("B", "O", "I", "Cin", "ldc", "Cout", "ldy", "KO", "KI", "DO", "DI", "PO", "PI", "SO", "SI", "OR", "IR", "x_col0", "y_col0", "mode",
            "act", "ldr", "res_mod", "Iout", "crop", "So", "no_halo", "x_bs", "y_bs")
    d = {k: c[k] for k in keys if k in c}
    OR = c["OR"] or c["O"]
    if c["x_gap"]:
        d["x_bs"] = c["O"] * c["I"] * c["ldc"] + c["x_gap"]
    if c["y_gap"]:
        d["y_bs"] = OR * c["IR"] * c["ldy"] + c["y_gap"]
    if c["res"]:
        d["ldr"] = c["Cout"] + 4
    return d


def y_view(c, y):
    """the launch's view [B, rows..., Cout] of the flat output tensor, and the boolean mask of the elements it owns"""
    B, OR = c["B"], c["OR"] or c["O"]
    rows = (c["O"], c["Iout"]) if c["mode"] == "convt" else (OR, c["IR"])
    img = rows[0] * rows[1] * c["ldy"]
    y = np.asarray(y).reshape(B, -1)
    v = y[:, :img].reshape(B, rows[0], rows[1], c["ldy"])[..., c["y_col0"]:c["y_col0"] + c["Cout"]]
    cols = np.zeros((B, rows[0], rows[1], c["ldy"]), bool)
    cols[..., c["y_col0"]:c["y_col0"] + c["Cout"]] = True
    own = np.zeros(y.shape, bool)
    own[:, :img] = cols.reshape(B, img)
    return v, own.reshape(-1)


@functools.lru_cache(maxsize=None)
def inputs(name, xscale=None):
    """x (the whole tensor the view lives in), w, b, res -- float32, read-only; everything outside the view is random too, so a read
    off the view shows in the result"""
    c = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    B, O, I = c["B"], c["O"], c["I"]
    x = rng.standard_normal((B, O * I * c["ldc"] + c["x_gap"])).astype(np.float32)
    glu, convt = c["mode"] == "glu", c["mode"] == "convt"
    K = c["KO"] * c["KI"] * c["Cin"]
    if convt:
        w = rng.standard_normal((c["Cin"], c["Cout"], 2 * c["So"]))
    else:
        w = rng.standard_normal(((2 if glu else 1) * c["Cout"], c["Cin"], c["KI"], c["KO"]))
    w = (w / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal((2 if glu else 1) * c["Cout"]).astype(np.float32)
    res = None
    if c["res"]:
        OR = c["OR"] or O
        rows = c["res_mod"] or (B * O * c["Iout"] if convt else B * OR * c["IR"])
        res = rng.standard_normal((rows, c["Cout"] + 4)).astype(np.float32)
    for a in (x, w, b, res):
        if a is not None:
            a.setflags(write=False)
    return x, w, b, res


def x_view(c, x):
    B, O, I = c["B"], c["O"], c["I"]
    return x[:, :O * I * c["ldc"]].reshape(B, O, I, c["ldc"])[..., c["x_col0"]:c["x_col0"] + c["Cin"]]


def evaluate(c, x, w, b, res, dtype):
    """the launch in numpy: (y, S) over the view"""
    g = {k: c[k] for k in ("KO", "KI", "DO", "DI", "PO", "PI", "SO", "SI", "OR", "IR")}
    xv = x_view(c, x)
    r = None if res is None else res[:, :c["Cout"]]
    if c["mode"] == "convt":
        assert c["PI"] == 1 and c["IR"] == c["I"] + 1 and c["KI"] == 2
        return R.conv_transpose(xv, w, b, c["So"], c["crop"], c["Iout"], c["act"], r, dtype)
    if c["mode"] == "glu":
        return R.conv_glu(xv, w, b, g, r, c["res_mod"], dtype)
    return R.conv_dense(xv, w, b, g, c["act"], r, c["res_mod"], dtype)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(float64 reference, S, e32 = the worst |fp32 evaluation - reference| / S) of the case"""
    c = BY_NAME[name]
    x, w, b, res = inputs(name)
    ref, S = evaluate(c, x, w, b, res, np.float64)
    y32, _ = evaluate(c, x, w, b, res, np.float32)
    for a in (ref, S):
        a.setflags(write=False)
    return ref, S, R.worst(y32, ref, S)
