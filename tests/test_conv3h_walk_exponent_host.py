"""conv3h_kernel's block exponent (kernels_conv3h.h, split_store) in numpy, for one strip: the exponent of a four-row block is the block's
need rounded down to a multiple of EQ = 8 -- a function of the block alone -- and a block without a nonzero element keeps the exponent of
the block split before it.  Walking T in one piece gives the same exponents (where a block has a nonzero element) and the same output bits as
walking it in every split into units, whatever exponent a unit inherits from the unit its workgroup walked before; and the arithmetic keeps
the bound of tests/test_conv3h_host.py against float64.  No GPU."""
import itertools

import numpy as np
import pytest

C, EQ = 48, 8


def f16(x):
    return x.astype(np.float32).astype(np.float16).astype(np.float64)


def need_of(m):
    """f16_scale_exp(m) - 1, clamped as the kernel clamps it: the largest |x| 2^need lies in [2^13, 2^14) -- a bit of headroom under the
    [2^14, 2^15) of the weights."""
    return min((15 - int(np.frexp(np.float32(m))[1]) if m > 0 else 15) - 1, 100)


def walk(x, w, bias, relu, pieces, stale):
    """x [48, T, F] (one strip, F <= 32) walked as the units `pieces` = [(t0, tiles)], unit i starting from the inherited exponent stale[i].
    Returns y [48, T, F] and {block: exponent} per unit."""
    T, F = x.shape[1:]
    ew = np.zeros(C, np.int64)
    for co in range(C):
        m = np.abs(w[co]).max()
        ew[co] = 15 - np.frexp(m)[1] if m > 0 else 0
    ws = w.astype(np.float64) * 2.0 ** ew[:, None, None, None]
    wh = f16(ws)
    wl = f16(ws - wh)
    tilesT = (T + 3) // 4
    xp = np.zeros((C, 4 * (tilesT + 1) + 4, F + 2))           # row t at index t + 3: block k = rows 4 k + 1 .. 4 k + 4 = index 4 k + 4 ..
    xp[:, 3:3 + T, 1:1 + F] = x
    y = np.full((C, T, F), np.nan)
    exps = []
    for (t0, tiles), e_prev in zip(pieces, stale):
        eb = {}
        xh, xl = np.zeros_like(xp), np.zeros_like(xp)
        for k in range(t0 - 1, t0 + tiles):
            blk = xp[:, 4 * k + 4: 4 * k + 8]
            m = np.abs(blk).max()
            e = (need_of(m) // EQ) * EQ if m > 0 else e_prev
            e_prev = e
            eb[k] = e
            s = blk * 2.0 ** e
            xh[:, 4 * k + 4: 4 * k + 8] = f16(s)
            xl[:, 4 * k + 4: 4 * k + 8] = f16(s - xh[:, 4 * k + 4: 4 * k + 8])
        exps.append(eb)
        for j in range(t0, t0 + tiles):
            for r in range(4):
                t = 4 * j + r
                if t >= T:
                    continue
                acc = np.zeros((C, F), np.float32)
                e_at = None
                for ky in range(3):
                    row = t + ky - 1 + 3
                    e_row = eb[(row - 4) // 4]                  # floor: index 3 (row -0: image row 0) is block -1
                    if e_at is not None and e_row != e_at:
                        acc = np.ldexp(acc, e_row - e_at).astype(np.float32)
                    e_at = e_row
                    for kx in range(3):
                        a_h, a_l = xh[:, row, kx:kx + F], xl[:, row, kx:kx + F]
                        acc = (acc.astype(np.float64) + wl[:, :, ky, kx] @ a_h + wh[:, :, ky, kx] @ a_l + wh[:, :, ky, kx] @ a_h).astype(np.float32)
                out = acc.astype(np.float64) * 2.0 ** (-(e_at + ew))[:, None] + bias[:, None]
                assert np.isnan(y[:, t]).all(), "two units computed the same row"
                y[:, t] = np.maximum(out, 0) if relu else out
    assert not np.isnan(y).any()
    return y, exps


def splits(tilesT):
    """every way to cut tile rows 0 .. tilesT - 1 into contiguous units (granularity 1)"""
    for cuts in itertools.product((0, 1), repeat=tilesT - 1):
        edges = [0] + [i + 1 for i, c in enumerate(cuts) if c] + [tilesT]
        yield [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]


def make(T, kind, seed):
    rng = np.random.default_rng(seed)
    F = 8
    x = rng.standard_normal((C, T, F)).astype(np.float32)
    if kind == "spread":
        # rows 2^2.1 apart at most: a block's rows and the row beside it stay within 2^8.4, inside the 2^12 under a block maximum down to
        # which the rule keeps an element's 22 bits (the "steps" case sits on that edge)
        x *= (10.0 ** (3.0 * np.cos(0.21 * np.arange(T))))[None, :, None].astype(np.float32)
    elif kind == "steps":                                        # 2^+-12 exactly at block edges (rows 4 k + 1) and at tile edges (rows 4 k)
        g = np.ones(T, np.float32)
        g[5:9] = 2.0 ** 12
        g[9:12] = 2.0 ** -12
        g[12:16] = 2.0 ** 12
        x *= g[None, :, None]
    elif kind == "zeros":                                        # a loud block, all-zero blocks behind it (one of them at a unit start in some splits), unit data
        x[:, :5] *= np.float32(1e15)
        x[:, 5:13] = 0
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C) * 10.0 ** rng.uniform(-1, 1, size=(C, 1, 1, 1))).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32).astype(np.float64)
    return x, w, bias


@pytest.mark.parametrize("T,kind,relu", [(19, "spread", False), (18, "steps", True), (17, "zeros", False)])
def test_every_split_gives_the_bits_of_the_whole_walk(T, kind, relu):
    x, w, bias = make(T, kind, T)
    tilesT = (T + 3) // 4
    y0, e0 = walk(x, w, bias, relu, [(0, tilesT)], [0])
    assert len(set(e0[0].values())) > 1, "the exponent never moved: the rescale path is untested"
    def blkmax(k):                                               # largest |x| of block k = image rows 4 k + 1 .. 4 k + 4 (0 where it has none)
        rows = x[:, max(0, 4 * k + 1): max(0, 4 * k + 5)]
        return float(np.abs(rows).max()) if rows.size else 0.0

    nonzero = {k for k in e0[0] if blkmax(k) > 0}
    rng = np.random.default_rng(1)
    n = 0
    for pieces in splits(tilesT):
        stale = [int(v) for v in rng.integers(-40, 60, size=len(pieces))]
        y, exps = walk(x, w, bias, relu, pieces, stale)
        for eb in exps:
            for k, e in eb.items():
                if k in nonzero:
                    assert e == e0[0][k] and e % EQ == 0
        assert np.array_equal(y.view(np.uint64), y0.view(np.uint64)), pieces
        n += 1
    assert n == 2 ** (tilesT - 1)
    # the precision bound of the rule: a block's largest element is in the fp16 range and at most EQ - 1 bits under where its need puts it
    # (2^5 was the floor of the rule with hysteresis: the need's [2^13, 2^14) and up to 8 bits)
    for k in nonzero:
        m = blkmax(k) * 2.0 ** e0[0][k]
        assert 2.0 ** (14 - EQ) <= m < 2.0 ** 14
    # ... and the result against float64, relative to sum |w x| (the bound of tests/test_conv3h_host.py)
    F = x.shape[2]
    xp = np.pad(x.astype(np.float64), ((0, 0), (1, 1), (1, 1)))
    ref = np.zeros((C, T, F))
    mag = np.zeros((C, T, F))
    for ky in range(3):
        for kx in range(3):
            ref += np.einsum("oc,ctf->otf", w[:, :, ky, kx].astype(np.float64), xp[:, ky:ky + T, kx:kx + F])
            mag += np.einsum("oc,ctf->otf", np.abs(w[:, :, ky, kx]).astype(np.float64), np.abs(xp[:, ky:ky + T, kx:kx + F]))
    ref += bias[:, None, None]
    mag += np.abs(bias)[:, None, None]
    if relu:
        ref = np.maximum(ref, 0)
    worst = float((np.abs(y0 - ref) / (mag + 1e-300)).max())
    print(f"{kind}: worst |y - ref| / sum |w x| = {worst:.3e}")
    assert (np.abs(y0 - ref) <= 2e-6 * mag + 1e-300).all(), worst
