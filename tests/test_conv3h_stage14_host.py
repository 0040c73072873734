"""CPU checks of conv3h_kernel's 14-stage consumer (csrc/kernels_conv3h.h, Conv3hCfg::PLAN): the stage plan is cut out of the header and
compiled with g++, then
  * every (kernel row, k group) pair of the 3 x 18 is multiplied exactly once per program, by the weight fragment and the ring row of its own
    kernel row -- followed lane by lane through the addresses the kernel forms -- and no stage of a program mixes rows of different exponent
    blocks for a wave that runs it, the accumulator's scale going old -> cur through the plan's one rescale;
  * the merged half stage's x and weight fragment reads are conflict-free under the `ds_read_b128` service groups of tests/test_conv3h_host.py;
  * a numpy emulation of the kernel's arithmetic in the NEW stage order (one fp32 rounding per stage, the rescale where the plan puts it) holds
    the bar of the 15-stage emulation, |y - ref| <= 2e-6 sum |w| |x|, on its four parametrisations (the bounded-rise case among them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "python-audio-separator_amd", "csrc", "kernels_conv3h.h")

C, CG8, IW, PSTR = 48, 6, 34, 96
ROWB = IW * PSTR
PART = 12 * ROWB
KGY = 18
WKY = 4 * 6144 + 3 * 2 * 512
W_OFF, X_OFF = 0, 3 * WKY
ZERO_SLOT = X_OFF + 2 * PART + 48
FULL, MERGED, PADDED = 0, 1, 2

# the lane groups one `ds_read_b128` is serviced in (tests/test_conv3h_host.py)
B128_READ_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)),
                    list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
                    list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)),
                    list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]


def worst_conflict(addr_of_lane, groups, nbanks):
    worst = 0
    for grp in groups:
        banks = {}
        for lane in grp:
            a = addr_of_lane(lane)
            for w in range(4):
                banks.setdefault(((a + 4 * w) // 4) % nbanks, set()).add(a)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """Conv3hCfg's stage plan as the compiler sees it: {"nst", "prog_of_wave" [4], "plan" [prog][stage] = dict(kind, ky, kyb, sg, rfrom, rto)}"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = open(HDR).read()
    a, b = src.index("struct Conv3hCfg {"), src.index("// Block walk.")
    prog = ("#include <cstdint>\n#include <cstring>\n#include <cmath>\n#include <cstdio>\n#include <vector>\n#include <algorithm>\n" + src[a:b] +
            "int main() { using CFG = Conv3hCfg; static_assert(CFG::NST == 14 && CFG::WKY == 27648 && CFG::WBYTES == 82944 && CFG::IMG_U32 == 20784, \"\");\n"
            "  static_assert(CFG::plan_find(0, CFG::MERGED).kind == CFG::MERGED && CFG::plan_find(1, CFG::PADDED).kind == CFG::PADDED, \"\");\n"
            "  printf(\"%d %d %d %d %d %d\\n\", CFG::NST, CFG::NPROG, CFG::PROG_OF_WAVE[0], CFG::PROG_OF_WAVE[1], CFG::PROG_OF_WAVE[2], CFG::PROG_OF_WAVE[3]);\n"
            "  for (int p = 0; p < CFG::NPROG; ++p) for (int s = 0; s < CFG::NST; ++s) { const CFG::Stage t = CFG::PLAN[p][s];\n"
            "    printf(\"%d %d %d %d %d %d\\n\", t.kind, t.ky, t.kyb, t.sg, t.rfrom, t.rto); }\n"
            "  printf(\"%d %d %d\\n\", (int)CFG::FULL, (int)CFG::MERGED, (int)CFG::PADDED); return 0; }\n")
    d = tmp_path_factory.mktemp("plan3h")
    cpp, exe = d / "plan3h.cpp", d / "plan3h"
    cpp.write_text(prog)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", str(exe), str(cpp)])
    rows = [[int(v) for v in ln.split()] for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    nst, nprog = rows[0][:2]
    assert rows[-1] == [FULL, MERGED, PADDED]
    keys = ("kind", "ky", "kyb", "sg", "rfrom", "rto")
    return {"nst": nst, "prog_of_wave": rows[0][2:], "plan": [[dict(zip(keys, rows[1 + p * nst + s])) for s in range(nst)] for p in range(nprog)]}


def lane_reads(st, lane, qq, part, c, ring_row):
    """(weight fragment address, x fragment address) lane `lane` reads in stage `st` for pixel tile qq, channel tile c and part: the kernel's
    address arithmetic.  ring_row [ky] is the ring row of kernel row ky (any block slot: rows of one slot are ROWB apart)."""
    li, g = lane & 15, lane >> 4
    if st["kind"] == FULL:
        kk = 4 * st["sg"] + g
        wa = W_OFF + st["ky"] * WKY + st["sg"] * 6144 + (c * 2 + part) * 1024 + lane * 16
        row = st["ky"]
    else:
        kk = KGY - 2 + (g & 1)                           # vl[4]: lanes past the last k group re-read groups 16 / 17
        row = st["ky"] if (g < 2 or st["kind"] == PADDED) else st["kyb"]
        wa = W_OFF + row * WKY + 4 * 6144 + (c * 2 + part) * 512 + (lane & 31) * 16
        if st["kind"] == PADDED and g >= 2:
            wa = ZERO_SLOT
    xa = X_OFF + ring_row[row] * ROWB + (kk // CG8 + li + 16 * qq) * PSTR + (kk % CG8) * 16 + part * PART
    return wa, xa


def weight_slot(wa):
    """fragment address -> (ky, k group, channel tile, part, output channel in the tile) by conv3h_pack's layout; None for the zero slot"""
    if wa == ZERO_SLOT:
        return None
    ky, r = divmod(wa - W_OFF, WKY)
    if r < 4 * 6144:
        sg, r = divmod(r, 6144)
        cp, r = divmod(r, 1024)
        lane = r // 16
        return ky, 4 * sg + (lane >> 4), cp // 2, cp % 2, lane & 15
    cp, r = divmod(r - 4 * 6144, 512)
    lane = r // 16
    assert lane < 32
    return ky, 16 + (lane >> 4), cp // 2, cp % 2, lane & 15


def test_plan_multiplies_every_k_group_once_with_its_own_row(plan):
    assert plan["nst"] == 14 and plan["prog_of_wave"] == [0, 1, 0, 0] and len(plan["plan"]) == 2
    for wave, prog in enumerate(plan["prog_of_wave"]):
        stages = plan["plan"][prog]
        # ring rows of the tile: u = wave + ky; u = 0, 1 are rows 2, 3 of the previous block's slot, u = 2..5 rows 0..3 of this block's
        u_of = [wave + ky for ky in range(3)]
        blk_of = ["old" if u < 2 else "cur" for u in u_of]
        ring_row = [(4 + 2 + u) if u < 2 else (8 + u - 2) for u in u_of]   # previous block in slot 1, this one in slot 2
        for qq in range(2):
            for c in range(3):
                seen = {}
                for st in stages:
                    for lane in range(64):
                        li, g = lane & 15, lane >> 4
                        slots = [weight_slot(lane_reads(st, lane, qq, part, c, ring_row)[0]) for part in range(2)]
                        if slots[0] is None:
                            assert slots[1] is None and st["kind"] == PADDED and g >= 2
                            continue
                        for part in range(2):
                            assert slots[part][2:] == (c, part, li)
                        assert slots[0][:2] == slots[1][:2]
                        ky, kk = slots[0][:2]
                        # the x fragment of the same lane: the ring row of THIS kernel row, the pixel and channels of THIS k group
                        xa = lane_reads(st, lane, qq, 0, c, ring_row)[1] - X_OFF
                        row, r = divmod(xa, ROWB)
                        pix, r = divmod(r, PSTR)
                        assert row == ring_row[ky] and pix == kk // CG8 + li + 16 * qq and r == (kk % CG8) * 16, (wave, st, lane)
                        assert lane_reads(st, lane, qq, 1, c, ring_row)[1] - X_OFF == xa + PART
                        seen[(ky, kk, li)] = seen.get((ky, kk, li), 0) + 1
                assert seen == {(ky, kk, li): 1 for ky in range(3) for kk in range(KGY) for li in range(16)}, (wave, qq, c)
        # exponent blocks: the accumulator's scale starts at the first stage's block, moves only through the plan's rescale, and every row a
        # stage reads is of the block the accumulators are scaled to
        scale = blk_of[stages[0]["ky"]]
        assert scale == blk_of[0]
        nresc = 0
        for st in stages:
            rows = {st["ky"], st["kyb"]}
            assert st["kyb"] == st["ky"] or st["kind"] == MERGED
            assert {blk_of[r] for r in rows} == {scale}, (wave, st)
            if st["rto"] >= 0:
                assert blk_of[st["rfrom"]] == scale
                scale = blk_of[st["rto"]]
                nresc += 1
        assert scale == "cur" and nresc == 1               # the epilogue divides by the CURRENT block's exponent
        kinds = [st["kind"] for st in stages]
        assert kinds.count(MERGED) == 1 and kinds.count(PADDED) == 1 and kinds.count(FULL) == 12
        m = stages[kinds.index(MERGED)]
        assert abs(m["ky"] - m["kyb"]) == 1                # adjacent ring rows of one block slot: the ring never wraps between them


def test_merged_stage_reads_are_conflict_free(plan):
    for prog, stages in enumerate(plan["plan"]):
        st = [s for s in stages if s["kind"] == MERGED][0]
        for wave in [w for w, p in enumerate(plan["prog_of_wave"]) if p == prog]:
            ring_row = [(4 + 2 + u) if u < 2 else (8 + u - 2) for u in (wave + ky for ky in range(3))]
            for part in range(2):
                for qq in range(2):
                    assert worst_conflict(lambda lane: lane_reads(st, lane, qq, part, 0, ring_row)[1], B128_READ_GROUPS, 64) == 1, (prog, wave, part, qq)
                for c in range(3):
                    assert worst_conflict(lambda lane: lane_reads(st, lane, 0, part, c, ring_row)[0], B128_READ_GROUPS, 64) == 1, (prog, wave, part, c)


def f16(x):
    return x.astype(np.float32).astype(np.float16).astype(np.float64)


def emulate14(x, w, bias, relu, plan):
    """conv3h_kernel's arithmetic for one strip walk, 14-stage order: x [48, T, F], F <= 32.  The preamble (weight exponents, blocks of four
    rows, the running exponent's three rules, the two-part split) is emulate()'s of tests/test_conv3h_host.py; the tile loop follows the plan:
    wave r = output row t % 4 runs program PROG_OF_WAVE[r], one fp32 rounding per stage, the rescale where the plan has it."""
    T, F = x.shape[1:]
    tilesT = (T + 3) // 4
    ew = np.zeros(C, np.int64)
    for co in range(C):
        m = np.abs(w[co]).max()
        ew[co] = 15 - np.frexp(m)[1] if m > 0 else 0
    ws = w.astype(np.float64) * 2.0 ** ew[:, None, None, None]
    wh = f16(ws)
    wl = f16(ws - wh)
    xp = np.zeros((C, 4 * (tilesT + 1) + 4, F + 2))                       # rows -3 .. : block j = rows 4 j + 1 .. 4 j + 4 -> index 4 j + 4 ..
    xp[:, 3:3 + T, 1:1 + F] = x
    xh, xl, eb = np.zeros_like(xp), np.zeros_like(xp), []
    e_prev = 0
    for j in range(-1, tilesT):
        blk = xp[:, 4 * j + 4: 4 * j + 8]
        m = np.float32(np.abs(blk).max())
        need = min((15 - np.frexp(m)[1] if m > 0 else 15) - 1, 100)
        e = e_prev
        if j < 0 or need < e_prev:
            e = need
        elif need > e_prev + 8:
            e = min(need, e_prev + 40)
        e_prev = e
        eb.append(e)
        s = blk * 2.0 ** e
        xh[:, 4 * j + 4: 4 * j + 8] = f16(s)
        xl[:, 4 * j + 4: 4 * j + 8] = f16(s - xh[:, 4 * j + 4: 4 * j + 8])
    y = np.zeros((C, T, F))
    nresc = 0
    for j in range(tilesT):
        e_old, e_cur = eb[j], eb[j + 1]                 # eb[0] is block -1
        for r in range(4):
            t = 4 * j + r
            if t >= T:
                continue
            eky = [e_old if r + ky < 2 else e_cur for ky in range(3)]
            acc = np.zeros((C, F), np.float32)
            for st in plan["plan"][plan["prog_of_wave"][r]]:
                if st["kind"] == FULL:
                    groups = [(st["ky"], 4 * st["sg"] + g) for g in range(4)]
                elif st["kind"] == MERGED:
                    groups = [(st["ky"], 16), (st["ky"], 17), (st["kyb"], 16), (st["kyb"], 17)]
                else:
                    groups = [(st["ky"], 16), (st["ky"], 17)]
                add = np.zeros((C, F))
                for ky, kk in groups:
                    row, kx, c0 = t + ky - 1 + 3, kk // CG8, (kk % CG8) * 8
                    a_h, a_l = xh[c0:c0 + 8, row, kx:kx + F], xl[c0:c0 + 8, row, kx:kx + F]
                    wh_, wl_ = wh[:, c0:c0 + 8, ky, kx], wl[:, c0:c0 + 8, ky, kx]
                    add += wl_ @ a_h + wh_ @ a_l + wh_ @ a_h             # products exact; the MFMA's order inside a stage is not modelled
                acc = (acc.astype(np.float64) + add).astype(np.float32)
                if st["rto"] >= 0 and eky[st["rto"]] != eky[st["rfrom"]]:
                    acc = np.ldexp(acc, eky[st["rto"]] - eky[st["rfrom"]]).astype(np.float32)
                    nresc += 1
            out = acc.astype(np.float64) * 2.0 ** (-(e_cur + ew))[:, None] + bias[:, None]
            y[:, t] = np.maximum(out, 0) if relu else out
    return y, eb, nresc


@pytest.mark.parametrize("T,spread,relu", [(12, 0.0, True), (37, 3.0, False), (67, 8.0, False), (21, -1.0, False)])
def test_stage14_emulation_vs_float64(plan, T, spread, relu):
    rng = np.random.default_rng(T)
    F = 32
    x = rng.standard_normal((C, T, F)).astype(np.float32)
    if spread >= 0:
        x *= (10.0 ** (spread * np.cos(0.21 * np.arange(T))))[None, :, None].astype(np.float32)
    else:
        # a loud passage (1e15), two all-zero blocks, then unit-size data: the exponent has to rise by more than 2^40 -- the bounded-rise rule
        x[:, :8] *= np.float32(1e15)
        x[:, 8:16] = 0
    w = (rng.standard_normal((C, C, 3, 3)) / np.sqrt(9 * C) * 10.0 ** rng.uniform(-1, 1, size=(C, 1, 1, 1))).astype(np.float32)
    bias = rng.standard_normal(C).astype(np.float32)
    y, eb, nresc = emulate14(x, w, bias.astype(np.float64), relu, plan)
    assert (len(set(eb)) > 1 and nresc > 0) or spread == 0, "the exponent never moved: the rescale path is untested"
    if spread < 0:
        assert np.diff(eb).max() == 40, "the bounded rise (a block more than 2^40 quieter) did not occur"
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
    assert (np.abs(y - ref) <= 2e-6 * mag + 1e-300).all(), float((np.abs(y - ref) / (mag + 1e-300)).max())
