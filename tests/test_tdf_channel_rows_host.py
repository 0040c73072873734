"""CPU checks of the channel-grouped row tiles of tdf3_kernel (csrc/kernels_gemm3.h, template flag CG): the row map and the final lane ->
(output channel, column) map are constexpr functions of TdfCgMap, cut out of the header and compiled with g++ into a stand-alone program that
prints them.  For T in {4, 8, 12} and B in {1, 3}:
  * every global row (b, c, t) of the [B, 48, T] row space appears in exactly one (tile, local row);
  * a tile holds one batch item and four consecutive frames, all 48 channels of each; the sixteen rows of accumulator group m are channels
    4 m .. 4 m + 3 in the lane's low two bits and the four frames in the next two -- what the epilogue's quad-permute steps rely on;
  * every (output channel, frame, column) of a tile's 4 x 4 x 128 outputs is stored by exactly one (wave, lane, j)."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "python-audio-separator_amd", "csrc", "kernels_gemm3.h")

CASES = list(itertools.product((4, 8, 12), (1, 3)))    # (T, B)
C, TQ, BM, BN = 48, 4, 192, 128


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{(T, B): rows [tiles, 192] of (global row, channel, frame in the tile)}, and the store map [4 waves, 64 lanes, 8] of (oc, frame, column)"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = open(HDR).read()
    a, b = src.index("struct TdfCgMap {"), src.index("// (end of TdfCgMap)")
    prog = ("#include <cstdint>\n#include <cstdio>\n#include <cstdlib>\n" + src[a:b] +
            "int main(int argc, char **argv) { using M = TdfCgMap; const int T = atoi(argv[1]), B = atoi(argv[2]);\n"
            "  static_assert(M::C == 48 && M::TQ == 4 && M::BM == 192 && M::BN == 128 && M::MREP * 16 == M::BM, \"\");\n"
            "  static_assert(M::row(5, 16 * 3 + 4 * 2 + 1, 8) == (2 * 48 + 13) * 8 + 4 + 2, \"tile 5 of T = 8: item 2, frames 4 .. 7\");\n"
            "  if (T > 0) { for (long long t = 0; t < (long long)B * (T / 4); ++t) for (int r = 0; r < M::BM; ++r)\n"
            "      printf(\"%lld %d %d\\n\", M::row(t, r, T), M::chan(r), M::frame(r)); }\n"
            "  else { for (int w = 0; w < 4; ++w) for (int l = 0; l < 64; ++l) for (int j = 0; j < 8; ++j)\n"
            "      printf(\"%d %d %d\\n\", M::out_oc(l), M::out_frame(l), M::out_col(w, l, j)); }\n"
            "  return 0; }\n")
    d = tmp_path_factory.mktemp("tdfcg")
    cpp, exe = d / "tdfcg.cpp", d / "tdfcg"
    cpp.write_text(prog)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", str(exe), str(cpp)])

    def run(*args):
        out = subprocess.run([str(exe)] + [str(v) for v in args], capture_output=True, text=True, check=True).stdout.splitlines()
        return np.array([[int(v) for v in ln.split()] for ln in out], dtype=np.int64)

    res = {(T, B): run(T, B).reshape(B * (T // 4), BM, 3) for T, B in CASES}
    res["store"] = run(0, 0).reshape(4, 64, 8, 3)
    return res


@pytest.mark.parametrize("T,B", CASES)
def test_every_row_is_in_exactly_one_tile(maps, T, B):
    rows = maps[(T, B)][:, :, 0].ravel()
    assert rows.size == B * C * T
    assert np.array_equal(np.sort(rows), np.arange(B * C * T)), "a global row is missing or held twice"


@pytest.mark.parametrize("T,B", CASES)
def test_a_tile_is_one_item_and_four_consecutive_frames(maps, T, B):
    m = maps[(T, B)]
    for tile in range(m.shape[0]):
        row, chan, fr = m[tile, :, 0], m[tile, :, 1], m[tile, :, 2]
        b, c, t = row // (C * T), (row // T) % C, row % T
        assert (b == tile // (T // TQ)).all(), "a tile mixes batch items"
        t0 = TQ * (tile % (T // TQ))
        assert np.array_equal(t, t0 + fr) and set(fr) == {0, 1, 2, 3}, "not four consecutive frames"
        assert np.array_equal(c, chan)
        # all 48 channels of each frame, once
        assert np.array_equal(np.sort(c * TQ + fr), np.arange(C * TQ))
        # accumulator group m = r >> 4: lane li = r & 15 holds channel 4 m + (li & 3) of frame li >> 2
        r = np.arange(BM)
        assert np.array_equal(chan, (r >> 4) * 4 + (r & 3)) and np.array_equal(fr, (r & 15) >> 2)


def test_every_output_is_stored_by_exactly_one_lane(maps):
    s = maps["store"]
    oc, fr, col = s[..., 0].ravel(), s[..., 1].ravel(), s[..., 2].ravel()
    assert (oc >= 0).all() and (oc < 4).all() and (fr >= 0).all() and (fr < TQ).all() and (col >= 0).all() and (col < BN).all()
    key = (oc * TQ + fr) * BN + col
    assert key.size == 4 * TQ * BN and np.unique(key).size == key.size, "an output element is stored twice or never"
    # a lane's eight values are two float4 of ONE output channel and frame: columns j = 0 .. 3 contiguous from a multiple of 4, j = 4 .. 7 sixteen on
    assert (s[..., 0] == s[..., :1, 0]).all() and (s[..., 1] == s[..., :1, 1]).all()
    c = s[..., 2]
    assert (c[..., 0] % 4 == 0).all() and np.array_equal(c[..., 1:4], c[..., :1] + np.arange(1, 4)) and np.array_equal(c[..., 4:], c[..., :4] + 16)
    # the frame of a lane's outputs is the frame of its rows, the four lanes of a frame hold the four output channels
    lanes = np.arange(64)
    assert np.array_equal(s[0, :, 0, 1], (lanes & 15) >> 2)
    for q in range(16):
        assert set(s[0, 4 * q:4 * q + 4, 0, 0]) == {0, 1, 2, 3}
