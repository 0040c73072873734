"""CPU checks of conv3h_kernel's tile order (csrc/kernels_conv3h.h, template flags XT / YT, engine option "conv3h_tiled"): the layout of the
tensors between the 3x3 convs of a TFC block.  The address map is a constexpr function of Conv3hCfg, cut out of the header and compiled with g++
into a stand-alone program that prints every offset, as tests/test_conv3h_partial_host.py does for the scratch.  For T in {4, 12}, F in {32, 96}:
  * the map is a bijection of the slice's elements onto its bytes [0, 48 T F 4) -- the planar slice's size;
  * every consumer store instruction (wave = row of the tile, store k) covers exactly one aligned, contiguous 1 KB, lane l at 16 l, and the
    offset the kernel forms (lane part + wave-uniform part + (k % 2) 3 + k / 2 blocks) is the map's;
  * every producer item's eight pieces are one aligned 128-byte line, 16 bytes apart, at the address the kernel forms (lane part + wave-uniform
    part in unsigned arithmetic) -- so a load instruction of a wave touches one line per in-image lane: counted and pinned, halo quads included;
  * the lane -> item map is the planar form's (nothing about the LDS side moves: tests/test_conv3h_host.py still speaks for the bank conflicts);
  * `pack` / `unpack`, the numpy helpers the GPU test uses, are built from the map and round-trip."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "python-audio-separator_amd", "csrc", "kernels_conv3h.h")

C = 48
CASES = list(itertools.product((4, 12), (32, 96)))           # (T, F)


def build_map_program(workdir):
    """compiles Conv3hCfg out of the header into a program that prints the map; None without g++"""
    if shutil.which("g++") is None:
        return None
    src = open(HDR).read()
    a, b = src.index("struct Conv3hCfg {"), src.index("// Block walk.")
    prog = ("#include <cstdint>\n#include <cstring>\n#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <vector>\n#include <algorithm>\n" + src[a:b] +
            "int main(int argc, char **argv) { using CFG = Conv3hCfg; const int T = atoi(argv[1]), F = atoi(argv[2]);\n"
            "  static_assert(CFG::TL_BLOCK == 1024 && CFG::TL_PIECE == 16, \"\");\n"
            "  static_assert(CFG::tl_off(8, 64, 5, 37, 29) == ((5 * 4 + 2) * 3 + 1) * 1024 + 1 * 256 + 13 * 16 + 1 * 4, \"\");\n"
            "  printf(\"%lld\\n\", (long long)CFG::tl_item_bytes(T, F));\n"
            "  for (int c = 0; c < CFG::C; ++c) for (int t = 0; t < T; ++t) for (int f = 0; f < F; ++f) printf(\"%lld\\n\", (long long)CFG::tl_off(T, F, t, f, c));\n"
            "  // consumer: tile (jt, strip), wave r, store k, lane l -- the kernel's pieces\n"
            "  for (int jt = 0; jt < T / 4; ++jt) for (int s = 0; s < F / 32; ++s) for (int r = 0; r < 4; ++r) for (int k = 0; k < 6; ++k) for (int l = 0; l < 64; ++l)\n"
            "    printf(\"%lld\\n\", (long long)(CFG::tl_store_lane(l) + CFG::tl_store_off(F, jt * 4 + r, s * 32, 0) + (unsigned)(((k % 2) * 3 + k / 2) * CFG::TL_BLOCK)));\n"
            "  // producer: block (j = -1 .. T / 4 - 1: rows 4 j + 1 ..), strip, item (row, cig, q), piece e -- the kernel's pieces, unsigned as the kernel adds them\n"
            "  for (int j = -1; j < T / 4; ++j) for (int s = 0; s < F / 32; ++s) for (int row = 0; row < 4; ++row) for (int cig = 0; cig < 6; ++cig) for (int q = 0; q < 10; ++q)\n"
            "    for (int e = 0; e < 8; ++e)\n"
            "      printf(\"%lld\\n\", (long long)(unsigned)(CFG::tl_fetch_lane(F, row, cig, q) + CFG::tl_fetch_org(F, 4 * j + 1, s * 32) + (unsigned)(e * CFG::TL_PIECE)));\n"
            "  return 0; }\n")
    cpp, exe = os.path.join(workdir, "tl3h.cpp"), os.path.join(workdir, "tl3h")
    with open(cpp, "w") as fh:
        fh.write(prog)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, cpp])
    return exe


def read_map(exe, T, F):
    """dict(bytes, off [48, T, F], store [T / 4, F / 32, 4, 6, 64], fetch [T / 4 + 1, F / 32, 4, 6, 10, 8]) of the compiled map"""
    v = np.array(subprocess.run([exe, str(T), str(F)], capture_output=True, text=True, check=True).stdout.split(), dtype=np.int64)
    n0, n1, n2 = C * T * F, (T // 4) * (F // 32) * 4 * 6 * 64, (T // 4 + 1) * (F // 32) * 4 * 6 * 10 * 8
    assert v.size == 1 + n0 + n1 + n2
    return {"bytes": int(v[0]), "off": v[1:1 + n0].reshape(C, T, F), "store": v[1 + n0:1 + n0 + n1].reshape(T // 4, F // 32, 4, 6, 64),
            "fetch": v[1 + n0 + n1:].reshape(T // 4 + 1, F // 32, 4, 6, 10, 8)}


def pack(x, off):
    """planar [..., 48 n, T, F] float32 -> the same bytes with every 48-channel slice in tile order (off: the map of one slice, [48, T, F])"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    lead, (c, T, F) = x.shape[:-3], x.shape[-3:]
    assert c % C == 0 and off.shape == (C, T, F)
    src = x.reshape(-1, C * T * F).view(np.uint32)
    dst = np.empty_like(src)
    dst[:, (off // 4).ravel()] = src
    return dst.view(np.float32).reshape(*lead, c, T, F)


def unpack(y, off):
    """the inverse of `pack`"""
    y = np.ascontiguousarray(y, dtype=np.float32)
    lead, (c, T, F) = y.shape[:-3], y.shape[-3:]
    assert c % C == 0 and off.shape == (C, T, F)
    src = y.reshape(-1, C * T * F).view(np.uint32)
    return np.ascontiguousarray(src[:, (off // 4).ravel()]).view(np.float32).reshape(*lead, c, T, F)


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    exe = build_map_program(str(tmp_path_factory.mktemp("tl3h")))
    if exe is None:
        pytest.skip("g++ not available")
    return {(T, F): read_map(exe, T, F) for T, F in CASES}


def producer_item(ptid):                                     # the kernel's lane -> item map (tests/test_conv3h_host.py)
    if ptid < 160:
        return ptid // 40, (ptid >> 1) & 3, (ptid & 1) + 2 * ((ptid >> 3) % 5)
    u = ptid - 160
    return ((u >> 2) & 1) + 2 * (u // 40), 4 + ((u >> 1) & 1), (u & 1) + 2 * ((u >> 3) % 5)


@pytest.mark.parametrize("T,F", CASES)
def test_the_map_is_a_bijection_onto_the_planar_slice_bytes(maps, T, F):
    m = maps[(T, F)]
    off = m["off"].ravel()
    assert m["bytes"] == C * T * F * 4, "a tile-order slice takes the planar slice's bytes"
    assert (off % 4 == 0).all() and np.array_equal(np.sort(off), 4 * np.arange(C * T * F))


@pytest.mark.parametrize("T,F", CASES)
def test_a_store_instruction_is_one_aligned_contiguous_kilobyte(maps, T, F):
    m = maps[(T, F)]
    for jt, s, r, k in itertools.product(range(T // 4), range(F // 32), range(4), range(6)):
        got = m["store"][jt, s, r, k]
        assert got[0] % 1024 == 0 and np.array_equal(got, got[0] + 16 * np.arange(64)), (jt, s, r, k)
        # lane (g, li) of store k holds pixels 16 (k % 2) + 4 g .. + 3 of channel 16 (k / 2) + li of row 4 jt + r
        lane = np.arange(64)
        want = m["off"][16 * (k // 2) + (lane & 15), 4 * jt + r, 32 * s + 16 * (k % 2) + 4 * (lane >> 4)]
        assert np.array_equal(got, want), (jt, s, r, k)
    # all of them together: every 16-byte quad of the slice exactly once
    assert np.array_equal(np.sort(m["store"].ravel()), 16 * np.arange(C * T * F // 4))


@pytest.mark.parametrize("T,F", CASES)
def test_a_producer_item_is_one_line_where_the_kernel_looks_for_it(maps, T, F):
    m = maps[(T, F)]
    per_wave = {}                                            # (block, strip) -> lines touched per load instruction, by producer wave
    lines = {}                                               # (in-image lanes, distinct lines) of a wave's load instruction -> how many
    for jb, s in itertools.product(range(T // 4 + 1), range(F // 32)):
        j = jb - 1
        for wave in range(4):
            for e in range(8):
                touched = set()
                lanes = 0
                for lane in range(64):
                    ptid = wave * 64 + lane
                    if ptid >= 240:
                        continue
                    row, cig, q = producer_item(ptid)
                    t, f = 4 * j + 1 + row, 32 * s - 4 + 4 * q
                    if not (0 <= t < T and 0 <= f < F):      # the kernel's predicate: the offset is never used
                        continue
                    a = int(m["fetch"][jb, s, row, cig, q, e])
                    assert a == m["off"][8 * cig + e, t, f], "the kernel's pieces do not add up to the map"
                    assert a % 128 == 16 * e and a - 16 * e == int(m["fetch"][jb, s, row, cig, q, 0]), "an item is one aligned 128-byte line, 16 bytes a channel"
                    touched.add(a // 128)
                    lanes += 1
                assert len(touched) == lanes, "every item has a line of its own"
                if e == 0:
                    per_wave.setdefault((jb, s), []).append(lanes)
                lines[lanes] = lines.get(lanes, 0) + 1
    # pinned: the lines a wave's load instruction touches = its in-image lanes.  A block with all four rows and ten quads inside the image: 64,
    # 64, 64, 48 for the four producer waves (240 items); with both halo quads outside (F = 32) the 48 items of quads 0 and 9 are gone (an
    # 8-lane group k of the map holds quads 2 (k % 5), 2 (k % 5) + 1: groups with k % 5 == 0 or 4 lose four lanes -- 3, 4, 2, 3 such groups a wave)
    if T == 12:
        jb = 2                                               # rows 5 .. 8
        want = [64, 64, 64, 48] if F == 96 else [52, 48, 56, 36]
        s_mid = 1 if F == 96 else 0
        assert per_wave[(jb, s_mid)] == want, per_wave[(jb, s_mid)]
        assert sum(want) == (240 if F == 96 else 192)
    total = sum(k * v for k, v in lines.items())
    rows_in = sum(1 for jb in range(T // 4 + 1) for row in range(4) if 0 <= 4 * (jb - 1) + 1 + row < T)
    quads_in = sum(1 for s in range(F // 32) for q in range(10) if 0 <= 32 * s - 4 + 4 * q < F)
    assert total == 8 * rows_in * quads_in * 6, "lines touched in all: one per in-image item and instruction"
    assert rows_in == T and quads_in == (F // 32) * 10 - 2


def test_the_lane_to_item_map_is_the_planar_one():
    src = open(HDR).read()
    body = src[src.index("=== producer ==="):src.index("const bool item_ok")]
    assert "if (ptid < 160) {" in body and "XT" not in body, "XT must not change which item a producer lane fetches (the LDS bank check assumes it)"


@pytest.mark.parametrize("T,F", CASES)
def test_pack_and_unpack_round_trip(maps, T, F):
    off = maps[(T, F)]["off"]
    rng = np.random.default_rng(T * 100 + F)
    x = rng.standard_normal((2, 96, T, F)).astype(np.float32)
    p = pack(x, off)
    assert p.shape == x.shape and not np.array_equal(p, x)
    assert np.array_equal(unpack(p, off).view(np.uint32), x.view(np.uint32))
    # element (c, t, f) of slice 1 of item 1 sits at the map's offset inside that slice
    flat = p[1, 48:].reshape(-1)
    for c, t, f in [(0, 0, 0), (47, T - 1, F - 1), (17, 2, 21)]:
        assert flat[off[c, t, f] // 4] == x[1, 48 + c, t, f]
