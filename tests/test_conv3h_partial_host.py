"""CPU checks of the partial-sum scratch of conv3h_kernel (csrc/kernels_conv3h.h, template parameter PS): the address map is a constexpr function of
Conv3hCfg, cut out of the header and compiled with g++ into a stand-alone program that prints every slot.  For tilesT in {1, 3}, tilesF in
{1, 2} and B in {1, 3}:
  * every (batch item, tile, wave, store, lane) has its own 16-byte slot -- the in-place launch (partial in AND out) relies on a lane never
    touching another lane's bytes;
  * a tile's slots cover exactly its 24576 bytes, a (wave, store) instruction 1024 contiguous bytes in lane order;
  * the offset the kernel forms (the item in the buffer resource's base, a wave-uniform 32-bit offset, store * 1024, lane * 16) is the map's;
  * the size the engine allocates (Conv3hCfg::ps_bytes) is the largest offset plus 16."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "python-audio-separator_amd", "csrc", "kernels_conv3h.h")

CASES = list(itertools.product((1, 3), (1, 2), (1, 3)))    # (tilesT, tilesF, B)
TILE, WAVE, STORE = 24576, 6144, 1024


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{(tilesT, tilesF, B): dict(bytes, item, off [B, tilesF, tilesT, 4, 6, 64], kern (the same from the kernel's own pieces))}"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = open(HDR).read()
    a, b = src.index("struct Conv3hCfg {"), src.index("// Block walk.")
    prog = ("#include <cstdint>\n#include <cstring>\n#include <cmath>\n#include <cstdio>\n#include <cstdlib>\n#include <vector>\n#include <algorithm>\n" + src[a:b] +
            "int main(int argc, char **argv) { using CFG = Conv3hCfg; const int tT = atoi(argv[1]), tF = atoi(argv[2]), B = atoi(argv[3]);\n"
            "  static_assert(CFG::PS_STORE == 1024 && CFG::PS_WAVE == 6144 && CFG::PS_TILE == 24576, \"\");\n"
            "  static_assert(CFG::PS_TILE == CFG::C * CFG::TH * CFG::TW * 4, \"a tile of the scratch is a tile of fp32 outputs\");\n"
            "  static_assert(CFG::ps_off(3, 2, 1, 1, 2, 3, 5, 63) == 2 * 3 * 24576 + ((1 * 3 + 2) * 4 + 3) * 6144 + 5 * 1024 + 63 * 16, \"\");\n"
            "  printf(\"%lld %lld\\n\", (long long)CFG::ps_bytes(B, tT, tF), (long long)CFG::ps_item_bytes(tT, tF));\n"
            "  for (int b = 0; b < B; ++b) for (int s = 0; s < tF; ++s) for (int j = 0; j < tT; ++j) for (int r = 0; r < 4; ++r)\n"
            "    for (int k = 0; k < 6; ++k) for (int l = 0; l < 64; ++l)\n"
            "      printf(\"%lld %lld\\n\", (long long)CFG::ps_off(tT, tF, b, s, j, r, k, l),\n"
            "             (long long)b * CFG::ps_item_bytes(tT, tF) + (long long)CFG::ps_wave_off(tT, s, j, r) + k * CFG::PS_STORE + l * 16);\n"
            "  return 0; }\n")
    d = tmp_path_factory.mktemp("ps3h")
    cpp, exe = d / "ps3h.cpp", d / "ps3h"
    cpp.write_text(prog)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", str(exe), str(cpp)])
    out = {}
    for tT, tF, B in CASES:
        rows = np.array([[int(v) for v in ln.split()] for ln in
                         subprocess.run([str(exe), str(tT), str(tF), str(B)], capture_output=True, text=True, check=True).stdout.splitlines()], dtype=np.int64)
        assert rows.shape == (1 + B * tF * tT * 4 * 6 * 64, 2)
        out[(tT, tF, B)] = {"bytes": int(rows[0, 0]), "item": int(rows[0, 1]), "off": rows[1:, 0].reshape(B, tF, tT, 4, 6, 64),
                            "kern": rows[1:, 1].reshape(B, tF, tT, 4, 6, 64)}
    return out


@pytest.mark.parametrize("tT,tF,B", CASES)
def test_every_lane_has_its_own_slot(maps, tT, tF, B):
    m = maps[(tT, tF, B)]
    off = m["off"].ravel()
    assert (off >= 0).all() and (off % 16 == 0).all()
    assert np.unique(off).size == off.size == B * tF * tT * 4 * 6 * 64, "two (tile, wave, store, lane) share a slot"
    assert np.array_equal(m["off"], m["kern"]), "the kernel's pieces (item base, wave offset, store, lane) do not add up to the map"
    # the offset inside the item -- what the kernel keeps in 32 bits -- is below the item's size
    inside = m["off"] - (np.arange(B, dtype=np.int64) * m["item"]).reshape(B, 1, 1, 1, 1, 1)
    assert (inside >= 0).all() and (inside + 16 <= m["item"]).all() and m["item"] == tF * tT * TILE


@pytest.mark.parametrize("tT,tF,B", CASES)
def test_tiles_and_instructions_are_contiguous(maps, tT, tF, B):
    off = maps[(tT, tF, B)]["off"]
    for b in range(B):
        for s in range(tF):
            for j in range(tT):
                t = off[b, s, j]
                base = ((b * tF + s) * tT + j) * TILE
                assert np.array_equal(np.sort(t.ravel()), base + 16 * np.arange(TILE // 16)), "a tile's slots are not exactly its 24576 bytes"
                for r in range(4):
                    for k in range(6):
                        # one store / load instruction: lane l at 16 l of 1024 contiguous bytes
                        assert np.array_equal(t[r, k], base + r * WAVE + k * STORE + 16 * np.arange(64)), (b, s, j, r, k)


@pytest.mark.parametrize("tT,tF,B", CASES)
def test_buffer_size_is_last_slot_plus_16(maps, tT, tF, B):
    m = maps[(tT, tF, B)]
    assert m["bytes"] == int(m["off"].max()) + 16 == B * tF * tT * TILE
