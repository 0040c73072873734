// 3x3 / pad 1 convolution of the TFC blocks (uvr_lib_v5/modules.py:11-17, mdxnet.py:97-113) as a DIRECT implicit GEMM on the fp16
// matrix pipe with the fp16 x 3 arithmetic of kernels_gemm3.h (two-part operands, three products, fp32 accumulation) -- no Winograd
// transforms, no cross-wave exchange.  One kernel for 48 -> 48 channels; layers of 96 / 144 channels run as 4 / 9 launches over 48-channel
// slices: for every output slice the input slices one after the other, each launch adding its sum to the partial sum of those before it.  The
// partial sum travels between two consecutive launches through a private scratch buffer in FRAGMENT order (template parameter PS: every lane
// stores and re-loads its own six accumulator quads, 1 KB contiguous per instruction), or -- engine option "conv3h_partial_scratch" = 0 --
// through the output tensor itself in the planar layout (accumulate mode, ACC).  With the scratch, the launches of the output slices that
// share an input slice can be ONE launch (Conv3hArgs::nob, engine option "conv3h_merge_out"): 2 / 3 launches per layer, the output slices side
// by side on groups of workgroups that walk together.  DESIGN.md 6k has the design record and the measurements behind every choice below.
// Fused-input form (template flag FIN, engine option "conv_fuse_input"): for the net's FIRST 3x3 layer, x is relu(b1 + w1 xin), the 4 -> 48 1x1
// input conv of the net -- the producers fetch the four planes of xin (four loads per item instead of eight) and form their eight channels in
// registers in a fixed fma order; pixels outside the plane enter the ring as 0 (the padding is of the 48-channel activation).  The 1x1 conv's
// launch, its 48-channel write and this kernel's read of it are gone.
//
//   y[b, co, t, f] = act(bias[co] + prev[b, co, t, f] + sum_{ci, ky, kx} w[co, ci, ky, kx] x[b, ci, t + ky - 1, f + kx - 1])        [B, C, T, F] fp32, F fastest
//
// GEMM view.  M = output pixels (16 consecutive f per MFMA tile), N = output channels (3 tiles of 16), K = (ky, kx, ci): a kernel row is
// 3 x 48 = 144 = 18 groups of eight channels = 4.5 stages of `v_mfma_f32_16x16x32_f16`.  A stage never mixes rows of different four-row blocks
// (they carry different exponents), but the half stages of two kernel rows of ONE block share a stage, half the lanes each: 14 stages per
// tile (Conv3hCfg::PLAN: 12 full, one merged, one half stage padded with a zero weight fragment), 252 MFMAs and 140 fragment reads per wave.
// A lane's eight K values are eight consecutive input channels of ONE
// tap at ONE pixel, so the x operand is kept channels-LAST in LDS ([ring row][34 pixels][48 halves], 96 bytes per pixel and part).
//
// One persistent 512-thread workgroup per CU (grid 256), two kinds of waves, ONE `s_barrier` per 4 x 32 output tile:
//   * waves 4-7 PRODUCE a block of four input rows x 40 columns x 48 channels per step: 240 (row, 8-channel group, column quad) items, one per
//     lane, eight `buffer_load_dwordx4` each (out-of-image rows / columns through the buffer bounds check = 0).  Four register sets: block
//     s + 4 is fetched, block s + 2's largest |x| reduced (v_max3 + DPP in a wave, a four-entry LDS table across waves, published by the step
//     barrier), block s + 1 scaled by the block's own power of two, split h + l (`v_fma_mixlo / hi_f16`) and written to its slot of a
//     12-row ring (`ds_write_b128`, 2-way at worst);
//   * waves 0-3 CONSUME block s: wave r owns output row r of the tile (two 16-pixel MFMA tiles x three 16-channel tiles = six accumulators);
//     per stage it reads six weight fragments and four x fragments (`ds_read_b128`, a stage ahead) and issues 18 MFMAs (w_l x_h, w_h x_l,
//     w_h x_h); where the exponent moved between the tile's two blocks, the accumulators are rescaled between the last stage of the previous
//     block's rows and the first of this block's.  The finished tile's epilogue and its six whole-line nontemporal stores run among the MFMAs
//     of the next tile.
//   The two-part weight image (432 x 48 x 2 x 2 B = 81 KB, fragment order, one exponent per OUTPUT channel) is copied into LDS once per
//   workgroup and stays for the whole launch.  LDS: 82944 (W) + 78336 (ring) + tables = 161.3 KB of the 160 KiB.
// Bank conflicts: a 16-pixel fragment read at the 96-byte pixel stride puts the sixteen lanes of every `ds_read_b128` service group on
// sixteen distinct 16-byte slots (pixel stride 6 slots: p and p + 8 collide, and a group holds p mod 8 all different for each k group;
// the two k groups of a service group are an odd number of slots apart) -- checked in tests/test_conv3h_host.py.
#pragma once
#include <cstring>
#include <vector>

#include "conv3h_walk_plan.h"
#include "kernels_gemm3.h"

namespace asx {

struct Conv3hArgs {
  const float *x;            // [B, 48, T, F] view (x_bstride floats between batch items)
  float *y;                  // [B, 48, T, F] view
  const u32x4 *wimg;         // conv3h_pack image: fragments, then int32 exponents [48]
  const float *bias;         // [48]
  int B, T, F;
  int64_t x_bstride, y_bstride;
  int act;                   // ACT_NONE / ACT_RELU
  int tilesT, tilesF;        // ceil(T / 4), F / 32
  int bw;                    // walk geometry: strips per band (32, 16 or 8: an XCD's 32 workgroups are 32 / bw groups of bw adjacent strips)
  const u32x4 *walk;         // the walk table (conv3h_walk_plan.h, conv3h_walk_table): row g = {steps, units, 0, 0}, the units {b, band, t0, tiles} of group g, a closing unit
  int walk_stride;           // entries per row
  const float *prev;         // nullptr, or a [B, 48, T, F] view (y's strides) ADDED in front of the activation: the partial sum of another 48-channel slice of the input
  long long *dbg;            // ABL & 32 (timeline build): [64 steps][8] s_memtime stamps of workgroup 0, then [4 workgroups][2048] step starts
  // fused-input form (FIN): x is unused; the 48 input channels are relu(b1 + w1 xin), the net's 1x1 input conv, formed by the producers
  const float *xin;          // [B, 4, T, F] view (xin_bstride floats between batch items)
  const float *w1;           // w1 [48][4], then b1 [48] (BatchNorm folded)
  int64_t xin_bstride;
  // partial-sum scratch (PS): [B][tilesF][tilesT][wave 4][store 6][lane 64] x 16 bytes (Conv3hCfg::ps_off), ps_bstride BYTES between batch items
  void *ps;
  int64_t ps_bstride;
  // merged output slices (the PS forms alone; nob <= 1 elsewhere): the launch runs nob output slices side by side on ONE input slice -- the
  // groups of the grid dealt into walkers of nob groups (conv3h_walk_plan.h, conv3h_walk_wg), group k of a walker on output slice k.  wimg, bias,
  // y and ps above are output slice 0's; slice ob's lie ob strides further
  int nob;
  int64_t wimg_ostride, bias_ostride, y_ostride;   // in 16-byte entries / floats / floats
  int64_t ps_ostride;                              // bytes: one whole scratch (Conv3hCfg::ps_bytes) per output slice
};

struct Conv3hCfg {
  static constexpr int C = 48, CG8 = C / 8;                       // channels, groups of eight
  static constexpr int TH = 4, TW = 32, IW = TW + 2;
  static constexpr int PSTR = C * 2;                              // bytes per pixel and part
  static constexpr int ROWB = IW * PSTR;                          // 3264 bytes per ring row and part
  static constexpr int RING = 12;                                 // ring rows: three blocks of four
  static constexpr int PART = RING * ROWB;                        // 39168 bytes per part
  static constexpr int KGY = 3 * CG8;                             // 18 k groups per kernel row
  static constexpr int SPK = (KGY + 3) / 4;                       // 5 stage groups per kernel row in the weight image, the last one (k groups 16, 17) half a fragment
  static constexpr int NST = (3 * KGY + 3) / 4;                   // 14 stages per tile: 54 k groups = 13.5 stages (stage plan below)
  static constexpr int WKY = (KGY / 4) * 3 * 2 * 1024 + 3 * 2 * 512;   // 27648 bytes of weight fragments per kernel row
  static constexpr int WBYTES = 3 * WKY;                          // 82944
  static constexpr int W_OFF = 0, X_OFF = WBYTES, TAB_OFF = X_OFF + 2 * PART;
  static constexpr int LDS_BYTES = TAB_OFF + 64;                  // maxima [2][4] floats, exponents [3] ints, 16 bytes of zeros at + 48
  static constexpr size_t IMG_U32 = WBYTES / 4 + 48;              // image size in 32-bit words
  static constexpr int EUP = 8;                                   // a block's largest element is never this many bits under the fp16 range ...
  static constexpr int EQ = 8;                                    // ... its exponent is the block's need rounded down to a multiple of this (a power of two, <= EUP)

  // Partial-sum scratch (template parameter PS of the kernel): the sum a launch hands to the next launch of the same output slice, in the order
  // the consumer waves hold it.  Wave r of tile (b, strip, jt) owns six stores of 1 KB -- store k = accumulator (channel tile k / 2, pixel tile
  // k % 2), lane l its own 16 bytes -- so a tile is 4 x 6 x 1024 = 24576 bytes = 48 channels x 4 rows x 32 pixels of fp32, and a batch item
  // tilesF x tilesT tiles (strip major).  The offset inside an item stays a 32-bit number (the launcher checks); the item goes into the base.
  static constexpr int PS_STORE = 1024, PS_WAVE = 6 * PS_STORE, PS_TILE = 4 * PS_WAVE;
  static constexpr int64_t ps_item_bytes(int tilesT, int tilesF) { return (int64_t)tilesF * tilesT * PS_TILE; }
  static constexpr int64_t ps_bytes(int B, int tilesT, int tilesF) { return (int64_t)B * ps_item_bytes(tilesT, tilesF); }   // the whole buffer
  static constexpr unsigned ps_wave_off(int tilesT, int strip, int jt, int r) { return (unsigned)((strip * tilesT + jt) * 4 + r) * (unsigned)PS_WAVE; }   // inside the item
  static constexpr int64_t ps_off(int tilesT, int tilesF, int b, int strip, int jt, int r, int k, int lane) {
    return (int64_t)b * ps_item_bytes(tilesT, tilesF) + ps_wave_off(tilesT, strip, jt, r) + k * PS_STORE + lane * 16;
  }

  // Tile order (template flags XT / YT of the kernel; engine option "conv3h_tiled"): the layout of a 48-channel slice that only this kernel
  // writes AND reads -- the output of conv1 and conv2 of a TFC block.  One 1-KB block per (row t, 16-pixel tile f / 16, 16-channel tile c / 16),
  // row major, the three channel tiles of a pixel tile side by side.  Inside a block the consumer's own lane order: lane g 16 + li (pixels
  // 4 g .. 4 g + 3 of channel li of the tile) at lane 16 -- a consumer store instruction (one accumulator of one wave: sixteen channels x
  // sixteen pixels) is one contiguous 1 KB with no lane swap, and the eight channels of a producer item (one pixel quad, channels 8 h .. 8 h + 7)
  // are ONE aligned 128-byte line, TL_PIECE bytes apart.  A slice takes exactly the planar slice's bytes (T % 4 == 0, F % 32 == 0), so buffers,
  // batch strides and slice offsets stay what they are.  (The other candidates -- the channel-in-group index outermost, eight lanes of a load
  // on one line -- and their times, skeleton and kernel: DESIGN.md 6k, profiles/NOTES.md round 23.)
  static constexpr int TL_BLOCK = 1024, TL_PIECE = 16;           // bytes per block; between the eight channels of a producer item
  static constexpr int64_t tl_item_bytes(int T, int F) { return (int64_t)C * T * F * 4; }
  static constexpr unsigned tl_block_off(int F, int t, int ftile, int n) { return ((unsigned)(t * (F / 16) + ftile) * 3u + (unsigned)n) * (unsigned)TL_BLOCK; }
  static constexpr unsigned tl_in_block(int g, int ch) { return (unsigned)(g * 256 + ch * TL_PIECE); }   // pixel quad g, channel ch of the tile
  static constexpr int64_t tl_off(int T, int F, int t, int f, int c) {   // byte offset of element (c, t, f) inside the slice
    (void)T;
    return (int64_t)tl_block_off(F, t, f / 16, c / 16) + tl_in_block((f % 16) / 4, c % 16) + (f % 4) * 4;
  }
  // consumer: lane (g = lane / 16, li = lane % 16) of store k = (channel tile k / 2, pixel tile k % 2) of the wave that owns row t of the tile at column f0
  static constexpr unsigned tl_store_lane(int lane) { return tl_in_block(lane >> 4, lane & 15); }
  static constexpr unsigned tl_store_off(int F, int t, int f0, int k) { return tl_block_off(F, t, f0 / 16 + k % 2, k / 2); }
  // producer, XT: item (row, 8-channel group cig, aligned quad q = columns f0 - 4 + 4 q ..) of the block at (row t1, column f0): a lane part and
  // a wave-uniform part (unsigned arithmetic: rows and columns outside the image are never dereferenced -- the in-image predicate -- but computed)
  static constexpr unsigned tl_fetch_lane(int F, int row, int cig, int q) {
    const int fq = 4 * q - 4;                                       // -4 .. 32: pixel tile (fq >> 4) = -1 (left neighbour), 0, 1, 2 (right neighbour)
    return ((unsigned)(row * (F / 16) + (fq >> 4)) * 3u + (unsigned)(cig >> 1)) * (unsigned)TL_BLOCK + tl_in_block((fq & 15) >> 2, (cig & 1) * 8);
  }
  static constexpr unsigned tl_fetch_org(int F, int t1, int f0) { return (unsigned)(t1 * (F / 16) + f0 / 16) * 3u * (unsigned)TL_BLOCK; }

  // Stage plan of a consumer wave's tile. A kernel row is four FULL stages (stage group sg: k groups 4 sg .. 4 sg + 3) and half a stage (k groups
  // 16, 17: stage group 4, a half fragment in the weight image).  Two half stages whose input rows lie in the SAME four-row block (one exponent)
  // share one MERGED stage: lanes g < 2 carry row ky's k groups 16, 17 (x fragment and weight half fragment), lanes g >= 2 row kyb's -- the half
  // fragment's lane order puts k group 16 + (g & 1) at (lane & 31) * 16, so lanes 32..63 read kyb's half fragment where lanes 0..31 read ky's.
  // The third row keeps a PADDED half stage (lanes g >= 2: a zero weight fragment).  Wave r reads ring row u = r + ky for kernel row ky; u < 2 is
  // the previous block, u >= 2 the current one: wave 0 (old, old, cur) merges rows 0 and 1, wave 1 (old, cur, cur) rows 1 and 2, waves 2 and 3 (all
  // cur) run wave 0's program.  `rto` >= 0: behind this stage the accumulators go from row rfrom's exponent to row rto's (the only block change
  // of the wave that runs the program) -- the scale moves old -> cur as it did with five stages per kernel row.
  enum { FULL = 0, MERGED = 1, PADDED = 2 };
  struct Stage {
    int kind, ky, kyb, sg;   // kyb: the second row of a merged stage (= ky otherwise)
    int rfrom, rto;
  };
  static constexpr int NPROG = 2;
  static constexpr int PROG_OF_WAVE[4] = {0, 1, 0, 0};
  static constexpr Stage PLAN[NPROG][NST] = {
      {{FULL, 0, 0, 0, -1, -1}, {FULL, 0, 0, 1, -1, -1}, {FULL, 0, 0, 2, -1, -1}, {FULL, 0, 0, 3, -1, -1},
       {FULL, 1, 1, 0, -1, -1}, {FULL, 1, 1, 1, -1, -1}, {FULL, 1, 1, 2, -1, -1}, {FULL, 1, 1, 3, -1, -1},
       {MERGED, 0, 1, 4, 1, 2},
       {FULL, 2, 2, 0, -1, -1}, {FULL, 2, 2, 1, -1, -1}, {FULL, 2, 2, 2, -1, -1}, {FULL, 2, 2, 3, -1, -1},
       {PADDED, 2, 2, 4, -1, -1}},
      {{FULL, 0, 0, 0, -1, -1}, {FULL, 0, 0, 1, -1, -1}, {FULL, 0, 0, 2, -1, -1}, {FULL, 0, 0, 3, -1, -1},
       {PADDED, 0, 0, 4, 0, 1},
       {FULL, 1, 1, 0, -1, -1}, {FULL, 1, 1, 1, -1, -1}, {FULL, 1, 1, 2, -1, -1}, {FULL, 1, 1, 3, -1, -1},
       {FULL, 2, 2, 0, -1, -1}, {FULL, 2, 2, 1, -1, -1}, {FULL, 2, 2, 2, -1, -1}, {FULL, 2, 2, 3, -1, -1},
       {MERGED, 1, 2, 4, -1, -1}}};
  // the stage of kind `kind` of program p (each program has one merged and one padded stage)
  static constexpr Stage plan_find(int p, int kind) {
    for (int s = 0; s < NST; ++s)
      if (PLAN[p][s].kind == kind) return PLAN[p][s];
    return Stage{-1, -1, -1, -1, -1, -1};
  }
};

// host: w [48, 48, 3, 3] fp32 -> the LDS image.  Stage (ky, sg) = k groups 4 sg .. 4 sg + 3 of kernel row ky, k group kk = (kx = kk / 6, eight
// input channels kk % 6); fragment (channel tile n, part p) of a full stage at ky * WKY + sg * 6144 + (n * 2 + p) * 1024 bytes, of the half stage
// (sg = 4, k groups 16 and 17) at ky * WKY + 24576 + (n * 2 + p) * 512; lane l of a fragment: output channel n * 16 + (l & 15), k group 4 sg + (l >> 4).
inline uint16_t conv3h_f16_rne(float f) {
  uint32_t x;
  memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u;
  const int32_t ex = (int32_t)((x >> 23) & 0xffu) - 127 + 15;
  uint32_t mant = x & 0x7fffffu;
  if (((x >> 23) & 0xffu) == 0xffu) return (uint16_t)(sign | 0x7c00u | (mant ? 0x200u : 0u));
  if (ex >= 31) return (uint16_t)(sign | 0x7c00u);
  if (ex <= 0) {
    if (ex < -10) return (uint16_t)sign;
    mant |= 0x800000u;
    const int shift = 14 - ex;
    uint32_t m = mant >> shift;
    const uint32_t rem = mant & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (m & 1u))) ++m;
    return (uint16_t)(sign | m);
  }
  uint32_t m = mant >> 13;
  const uint32_t rem = mant & 0x1fffu;
  uint32_t e2 = (uint32_t)ex;
  if (rem > 0x1000u || (rem == 0x1000u && (m & 1u))) {
    if (++m == 0x400u) {
      m = 0;
      if (++e2 >= 31u) return (uint16_t)(sign | 0x7c00u);
    }
  }
  return (uint16_t)(sign | (e2 << 10) | m);
}
inline float conv3h_f16_f(uint16_t h) {
  const uint32_t sign = ((uint32_t)h & 0x8000u) << 16;
  const uint32_t ex = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t u;
  if (ex == 0) {
    if (m == 0) {
      u = sign;
    } else {
      int sh = 0;
      uint32_t mm = m;
      while (!(mm & 0x400u)) {
        mm <<= 1;
        ++sh;
      }
      u = sign | ((uint32_t)(127 - 15 - sh + 1) << 23) | ((mm & 0x3ffu) << 13);
    }
  } else if (ex == 31) {
    u = sign | 0x7f800000u | (m << 13);
  } else {
    u = sign | ((ex - 15 + 127) << 23) | (m << 13);
  }
  float f;
  memcpy(&f, &u, 4);
  return f;
}

inline void conv3h_pack(const float *w, std::vector<uint32_t> &img) {
  using CFG = Conv3hCfg;
  constexpr int C = CFG::C;
  img.assign(CFG::IMG_U32, 0u);
  int ex[C];
  for (int co = 0; co < C; ++co) {
    float mx = 0.f;
    for (int i = 0; i < C * 9; ++i) {
      const float v = std::fabs(w[(size_t)co * C * 9 + i]);
      if (v <= 3.4028234663852886e38f) mx = std::max(mx, v);
    }
    ex[co] = 0;
    if (mx > 0.f) {
      int fe;
      (void)frexpf(mx, &fe);
      ex[co] = 15 - fe;                                // mx 2^ex in [2^14, 2^15)
    }
    img[CFG::WBYTES / 4 + co] = (uint32_t)ex[co];
  }
  for (int ky = 0; ky < 3; ++ky)
    for (int sg = 0; sg < CFG::SPK; ++sg) {
      const bool half = sg == CFG::SPK - 1;
      const int nl = half ? 32 : 64;
      for (int n = 0; n < 3; ++n)
        for (int lane = 0; lane < nl; ++lane) {
          const int co = n * 16 + (lane & 15);
          const int kk = 4 * sg + (lane >> 4);
          const int tap = ky * 3 + kk / CFG::CG8, c0 = (kk % CFG::CG8) * 8;
          uint16_t hh[8], ll[8];
          for (int e = 0; e < 8; ++e) {
            const float us = ldexpf(w[((size_t)co * C + c0 + e) * 9 + tap], ex[co]);
            hh[e] = conv3h_f16_rne(us);
            ll[e] = conv3h_f16_rne(us - conv3h_f16_f(hh[e]));
          }
          const size_t pstep = half ? 512 : 1024;
          const size_t fb = (size_t)ky * CFG::WKY + (half ? (size_t)(CFG::SPK - 1) * 6144 + (size_t)(n * 2) * 512 : (size_t)sg * 6144 + (size_t)(n * 2) * 1024);
          uint32_t *dh = &img[(fb + (size_t)lane * 16) / 4], *dl = &img[(fb + pstep + (size_t)lane * 16) / 4];
          for (int e = 0; e < 4; ++e) {
            dh[e] = (uint32_t)hh[2 * e] | ((uint32_t)hh[2 * e + 1] << 16);
            dl[e] = (uint32_t)ll[2 * e] | ((uint32_t)ll[2 * e + 1] << 16);
          }
        }
    }
}

// Block walk.  XCD x (block id & 7: where the dispatcher puts the workgroup, for speed only) holds 32 workgroups (block id >> 3): 32 / bw GROUPS
// of bw adjacent strips.  A group walks the UNITS of its row of the walk table (conv3h_walk_plan.h plans them on the host; the reads are
// wave-uniform) one after the other: unit {b, band, t0, tiles} = tile rows t0 .. t0 + tiles - 1 of strips band * bw .. of batch item b, the bw
// workgroups down T together, so the halo columns a strip shares with its neighbours are re-read from that XCD's L2.  A unit is tiles + 1
// blocks of four input rows: block j = rows 4 (t0 + j) + 1 .. + 4, j = -1 .. tiles - 1; output tile j (rows 4 (t0 + j) .. + 3) needs rows
// 4 (t0 + j) - 1 .. 4 (t0 + j) + 4 = the last two rows of block j - 1 and block j.  Where a unit begins changes no result: a block's exponent
// is a function of the block alone (split_store).  Strips past tilesF are all-padding (never stored): they keep the walk in step.  The grid
// is 256 workgroups; the row's closing unit (2^30 tiles) is never left, whatever the producers' look-ahead.
struct Conv3hWalk {
  int u, j, b, strip, t0, tiles;   // u: entry of the current unit in the table
};
__device__ __forceinline__ void conv3h_walk_unit(const Conv3hArgs &a, int wg, Conv3hWalk &w) {
  // (behind the kernel's first store the compiler reads the table through the vector cache: the unit goes back to scalar registers, where the
  // resources and offsets built from it want it)
  const u32x4 un = a.walk[w.u];
  w.b = __builtin_amdgcn_readfirstlane((int)un.x);
  w.strip = __builtin_amdgcn_readfirstlane((int)un.y) * a.bw + ((wg >> 3) & (a.bw - 1));
  w.t0 = __builtin_amdgcn_readfirstlane((int)un.z);
  w.tiles = __builtin_amdgcn_readfirstlane((int)un.w);
}
// MO (the kernel's PS forms): the launch may run a.nob output slices side by side -- the row is the group's WALKER's (conv3h_walk_wg)
template <bool MO>
__device__ __forceinline__ int conv3h_walk_row(const Conv3hArgs &a, int wg) {   // first entry of the group's row (bw is a power of two)
  if constexpr (MO) {
    int row, ob;
    conv3h_walk_wg(wg, a.bw, a.nob, row, ob);
    return row * a.walk_stride;
  }
  const int sh = __builtin_ctz((unsigned)a.bw);
  return ((wg & 7) * (32 >> sh) + ((wg >> 3) >> sh)) * a.walk_stride;
}
__device__ __forceinline__ int conv3h_row0(const Conv3hWalk &w) { return w.t0 * 4; }   // first row of the unit
template <bool MO>
__device__ __forceinline__ int conv3h_nblocks(const Conv3hArgs &a, int wg) { return (int)a.walk[conv3h_walk_row<MO>(a, wg)].x; }
template <bool MO>
__device__ __forceinline__ void conv3h_walk_init(const Conv3hArgs &a, int wg, Conv3hWalk &w) {
  w.u = conv3h_walk_row<MO>(a, wg) + 1;
  w.j = -1;
  conv3h_walk_unit(a, wg, w);
}
__device__ __forceinline__ void conv3h_walk_next(const Conv3hArgs &a, int wg, Conv3hWalk &w) {
  if (++w.j == w.tiles) {
    w.j = -1;
    ++w.u;
    conv3h_walk_unit(a, wg, w);
  }
}

// h + l fp16 parts of x0 s, x1 s (s a power of two): four single-issue VALU instructions for two elements -- `v_fma_mix{lo,hi}_f16` computes
// the fp32 fma and rounds it to a half of the destination: h = RNE_f16(x s + 0), l = RNE_f16(x s - h) (x s and the difference are exact in
// fp32: the same values as kernels_gemm3.h's split2h_pair, which multiplies, converts, converts back, subtracts and converts).
__device__ __forceinline__ void conv3h_split_pair(float x0, float x1, float s, unsigned &h, unsigned &l) {
  unsigned hh = 0, ll = 0;
  asm("v_fma_mixlo_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(hh) : "v"(x0), "v"(s));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0 op_sel_hi:[0,0,0]" : "+v"(hh) : "v"(x1), "v"(s));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel:[0,0,0] op_sel_hi:[0,0,1]" : "+v"(ll) : "v"(x0), "v"(s), "v"(hh));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(ll) : "v"(x1), "v"(s), "v"(hh));
  h = hh;
  l = ll;
}

// `keep` in the lanes outside bank mask BM (bit k: lanes 4 k .. 4 k + 3 of every 16), lane l ^ 8's `from` inside it
template <int BM>
__device__ __forceinline__ float ror8m(float keep, float from) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, keep), __builtin_bit_cast(int, from), 0x128, 0xf, BM, false));   // row_ror:8
}

// the producer registers only the fused-input form has
template <bool FIN>
struct Conv3hFinRegs {};
template <>
struct Conv3hFinRegs<true> {
  f32x4 rin[4][4];           // the four fetched sets (block m in set m % 4): four input planes each
  bool ok[4];                // the item of set m % 4 lies inside the plane
  float w1[8][4], b1[8];     // the 1x1 weights and biases of the lane's eight channels, loaded once
};

// ABL (measurement-only builds, results are garbage): 2 = no global loads, 4 = no stores, 8 = no split / LDS writes, 32 = timeline stamps
// ACC: accumulate mode (a.prev != nullptr): its own instantiation -- a run-time test in front of the six loads ended the MFMA scheduling region
// and cost the plain launches a dozen register moves per tile
// FIN: fused input (never with ACC).  The layer's 48 input channels are a pointwise function of FOUR planes -- the net's 1x1 input conv with
// its folded BatchNorm and ReLU -- so a producer item fetches four lines instead of eight and forms its eight channels in registers,
// v = max(0, fma(w3, in3, fma(w2, in2, fma(w1, in1, fma(w0, in0, b))))) in this fixed order (a halo pixel is computed by two tiles: same bits),
// at the step that first consumes the block (the maximum); a pixel outside the plane enters the ring as 0 -- the 3x3 conv pads the 48-channel
// activation, not the four planes, so relu(b) must not leak in -- through the item's in-image predicate, kept beside the raw set.
// PS: partial sums through the scratch a.ps (never with ACC or FIN; compile-time for the reason given at ACC).  Bit 1 (partial OUT: the launch
// is not the last input slice of its output slice): the epilogue's values -- the ones the planar form would store, computed in the same order
// -- go to the scratch, every lane its own six accumulator quads, no lane swap; bit 0 (partial IN): `prev` is the scratch, six loads at the
// same addresses behind stage 7, each value added where the planar `prev` is added (behind the fma, in front of the activation).
// INVARIANT: a launch with both bits reads and writes the SAME scratch in place, and a launch reads what the one before it wrote.  That is
// safe because a lane only ever touches its own 16 bytes per (tile, store) -- loaded behind stage 7 of the tile, overwritten a step later --
// and because the launches of one output slice walk identically: same B, T, F, tilesT, tilesF, bw and walk table (the launcher builds them from one place).
// Merged output slices (a.nob > 1, engine option "conv3h_merge_out"): ONE launch per input slice runs all output slices side by side, each
// group of workgroups on the slice conv3h_walk_wg gives it, with its own weight image, bias, y slice and scratch -- a layer is n launches
// instead of n x n and an input slice is fetched from memory once, not n times (the n groups of a walker read the same lines at the same
// time).  The invariant holds per output slice: the n launches of a layer share nob and the table, so a group meets its own scratch again.
// XT / YT: the input slice a.x / the final output slice a.y is in TILE ORDER (Conv3hCfg::tl_off) instead of planar -- for the tensors between the
// 3x3 convs of one TFC block, which nothing but this kernel touches (compile-time for the reason given at ACC).  Same accumulators, same lanes,
// same values, another address.  XT changes `fetch` alone: the lane's item is what it was, its eight channels lie TL_PIECE bytes apart (one
// 128-byte line) behind an offset from the map, and the in-image predicate is what it was -- a row outside [0, T) or a quad outside [0, F) enters
// the ring as 0 whatever a neighbouring block holds.  YT changes the final epilogue alone: the values of the planar store (bias, partial in,
// activation, in that order), every lane its own six quads as the partial-out form stores them -- 1 KB contiguous per instruction, no lane
// swap.  XT never with FIN or ACC, YT never with ACC; a partial-out launch (PS & 2) writes no final output: YT means nothing there.
template <int ABL = 0, bool ACC = false, bool FIN = false, int PS = 0, bool XT = false, bool YT = false>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv3h_kernel(Conv3hArgs a) {
  using CFG = Conv3hCfg;
  constexpr bool PIN = (PS & 1) != 0, POUT = (PS & 2) != 0;
  constexpr bool OWNQ = POUT || YT;                    // the epilogue stores the lane's own accumulator quads (no lane swap)
  constexpr bool MO = PS != 0;                         // merged output slices (a.nob): only a layer of several slices has them, and it runs the PS forms
  static_assert(!(PS != 0 && (ACC || FIN)), "partial sums through the scratch: neither the planar accumulate mode nor the fused input");
  static_assert(!(XT && (FIN || ACC)) && !(YT && (ACC || POUT)), "tile order: never the accumulate mode; the fused input has no input slice, a partial-out launch no final output");
  extern __shared__ float lds_f[];
  char *lds = reinterpret_cast<char *>(lds_f);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wg = blockIdx.x;
  float *maxtab = reinterpret_cast<float *>(lds + CFG::TAB_OFF);   // [2][4]: block parity, producer wave
  int *exps = reinterpret_cast<int *>(lds + CFG::TAB_OFF + 32);    // [3]: block % 3
  if constexpr (MO) {
    // the group's output slice: everything that depends on it moves HERE, once -- the rest of the kernel is what it is for one slice
    int row, ob;
    conv3h_walk_wg(wg, a.bw, a.nob, row, ob);
    if (row < 0) return;                               // a group beyond walkers * nob (the whole workgroup, in front of the first barrier)
    a.wimg += ob * a.wimg_ostride;
    if (a.bias) a.bias += ob * a.bias_ostride;
    a.y += ob * a.y_ostride;
    a.ps = static_cast<char *>(a.ps) + ob * a.ps_ostride;
  }

  // ---- weights: global image -> LDS, once
  {
    const u32x4 *src = a.wimg;
    u32x4 *dst = reinterpret_cast<u32x4 *>(lds + CFG::W_OFF);
    for (int i = tid; i < CFG::WBYTES / 16; i += 512) dst[i] = src[i];
  }
  const int64_t TF = (int64_t)a.T * a.F;
  const int NB = __builtin_amdgcn_readfirstlane(conv3h_nblocks<MO>(a, wg));
  const unsigned plane_bytes = (unsigned)(CFG::C * TF * 4);

  if (wave >= 4) {
    // =================================================================== producer ===================================================
    // Items of a block: (row 0..3, 8-channel group 0..5, aligned quad of columns 0..9 = image columns f0 - 4 + 4 q .. + 3; the 34-column
    // window is columns f0 - 1 .. f0 + 32: quad 0 gives its last pixel, quad 9 its first, the others all four) -- 240 items, ONE per
    // producer lane, eight `buffer_load_dwordx4` each (one per channel plane).  Lane order inside an 8-lane group: bit 0 = quad parity
    // (lane pairs fetch 32 contiguous bytes: a vector-memory instruction costs ~45 cycles of the CU's address unit that way against
    // ~70 with every lane on its own line, tools/experimental/micro_ta.hip), bits 1-2 = channel groups 0..3 (items 0..159) or channel
    // group 4 / 5 x row parity (items 160..239): the eight lanes of a `ds_write_b128` service group land on four 16-byte slots twice
    // each (2-way: 16 LDS cycles, the instruction costs 13 anyway) instead of on one slot eight times.
    const int ptid = tid - 256, pw = wave - 4;
    int row, cig, q;
    if (ptid < 160) {
      q = (ptid & 1) + 2 * ((ptid >> 3) % 5);
      cig = (ptid >> 1) & 3;
      row = ptid / 40;
    } else {
      const int u = ptid - 160;
      q = (u & 1) + 2 * ((u >> 3) % 5);
      cig = 4 + ((u >> 1) & 1);
      row = ((u >> 2) & 1) + 2 * (u / 40);
    }
    const bool item_ok = ptid < 240;
    const int loff = (row * CFG::IW + 4 * q - 3) * CFG::PSTR + cig * 16;   // pixel 0 of the quad inside a block slot (window column 4 q - 3: never written for quad 0)
    const int goff = FIN ? (int)((int64_t)row * a.F + 4 * q)              // FIN: the four planes are shared by the channel groups
                         : (int)(((int64_t)cig * 8 * a.T + row) * a.F + 4 * q);  // floats from (channel 0, row 4 j + 1, column f0 - 4); < 2^29 (launcher)
    const unsigned tl_lane = CFG::tl_fetch_lane(a.F, row, cig, q);        // XT: bytes from the block of (row 4 j + 1, pixel tile f0 / 16, channel tile 0)
    // four register sets: block m lives in set m % 4 (fetched in step m - 4, its maximum taken in step m - 2, split in step m - 1).
    // FIN: the four fetched sets are fr.rin; the 48-channel values exist from the maximum to the split: two sets, m % 2
    constexpr int NSET = FIN ? 2 : 4;
    f32x4 raw[NSET][8];
    Conv3hFinRegs<FIN> fr;
    const unsigned in_bytes = (unsigned)(4 * TF * 4);
    if constexpr (FIN) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const f32x4 wv = *reinterpret_cast<const f32x4 *>(a.w1 + (cig * 8 + c) * 4);
        fr.w1[c][0] = wv.x;
        fr.w1[c][1] = wv.y;
        fr.w1[c][2] = wv.z;
        fr.w1[c][3] = wv.w;
        fr.b1[c] = a.w1[CFG::C * 4 + cig * 8 + c];
      }
    }

    Conv3hWalk wk;
    conv3h_walk_init<MO>(a, wg, wk);
    int nf = 0;                                        // blocks fetched so far
    auto fetch = [&](auto setc) {                      // the next block of the walk (nothing past the last one: every offset out of range)
      constexpr int S = decltype(setc)::value;
      const int tb = nf < NB ? wk.b : 0, f0 = wk.strip * 32;
      const int t1 = nf < NB ? conv3h_row0(wk) + wk.j * 4 + 1 : -(1 << 20);
      ++nf;
      conv3h_walk_next(a, wg, wk);
      __amdgpu_buffer_rsrc_t rs = FIN ? __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.xin + (int64_t)tb * a.xin_bstride), 0, in_bytes, 0x00020000)
                                      : __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x + (int64_t)tb * a.x_bstride), 0, plane_bytes, 0x00020000);
      const int org = t1 * a.F + (f0 - 4);
      // F % 4 == 0 and the quad is aligned: inside the row or outside as a whole
      const bool ok = item_ok && (unsigned)(t1 + row) < (unsigned)a.T && (unsigned)(f0 - 4 + 4 * q) < (unsigned)a.F;
      const unsigned vo = !ok ? 0xfffffff0u                                 // past num_records: the load returns 0
                              : (XT ? tl_lane + CFG::tl_fetch_org(a.F, t1, f0) : (unsigned)(goff + org) * 4u);
      if constexpr (FIN) {
        fr.ok[S] = ok;
#pragma unroll
        for (int j = 0; j < 4; ++j) fr.rin[S][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)vo, (int)(j * TF * 4), 0));
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if constexpr ((ABL & 2) != 0) raw[S][j] = (f32x4){0.25f, 0.5f, 0.75f, 1.f};
          else raw[S][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)vo, XT ? j * CFG::TL_PIECE : (int)(j * TF * 4), 0));
        }
      }
    };
    auto tile_max = [&](auto setc, int slot) {         // largest finite |x| of the block held in set S -> maxtab[slot][pw]
      constexpr int S = decltype(setc)::value % NSET;
      if constexpr (FIN) {                             // the block's 48-channel values, first needed here
        constexpr int SI = decltype(setc)::value;
        const bool ok = fr.ok[SI];
        auto px = [&](float i0, float i1, float i2, float i3, int c) {
          const float v = __builtin_fmaf(fr.w1[c][3], i3, __builtin_fmaf(fr.w1[c][2], i2, __builtin_fmaf(fr.w1[c][1], i1, __builtin_fmaf(fr.w1[c][0], i0, fr.b1[c]))));
          return ok ? __builtin_fmaxf(v, 0.f) : 0.f;   // outside the plane: the 3x3 conv's zero padding, not relu(b1)
        };
        const f32x4 i0 = fr.rin[SI][0], i1 = fr.rin[SI][1], i2 = fr.rin[SI][2], i3 = fr.rin[SI][3];
#pragma unroll
        for (int c = 0; c < 8; ++c) raw[S][c] = (f32x4){px(i0.x, i1.x, i2.x, i3.x, c), px(i0.y, i1.y, i2.y, i3.y, c), px(i0.z, i1.z, i2.z, i3.z, c), px(i0.w, i1.w, i2.w, i3.w, c)};
      }
      float m = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(raw[S][j].x)), __builtin_fabsf(raw[S][j].y));   // v_max3_f32 with |.| modifiers
        m = __builtin_fmaxf(__builtin_fmaxf(m, __builtin_fabsf(raw[S][j].z)), __builtin_fabsf(raw[S][j].w));
      }
      m = wave_max64(m);
      if (!(m <= 3.4028234663852886e38f)) {            // an Inf in the block (v_max never returns a NaN): the largest FINITE |x| sets the exponent --
        m = 0.f;                                       // the Inf / NaN elements poison the outputs they reach and nothing else
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          m = fmaxf(m, fmaxf(fmaxf(finite_or_zero(raw[S][j].x), finite_or_zero(raw[S][j].y)), fmaxf(finite_or_zero(raw[S][j].z), finite_or_zero(raw[S][j].w))));
        }
        m = wave_max64(m);
      }
      if (lane == 0) maxtab[slot * 4 + pw] = m;
    };
    int e_prev = 0;                                    // exponent of the block split last
    auto split_store = [&](auto setc, int par, int slot3) {   // set S -> ring rows of block slot `slot3` under the block's exponent
      constexpr int S = decltype(setc)::value % NSET;
      const f32x4 mv = *reinterpret_cast<const f32x4 *>(maxtab + par * 4);
      const float m = fmaxf(fmaxf(mv.x, mv.y), fmaxf(mv.z, mv.w));
      // Block exponent: the block's need (largest |x| 2^need in [2^13, 2^14)) rounded DOWN to a multiple of EQ = 8 -- a function of the block
      // alone, so the bits of a tile do not depend on where the walk that reaches it began (which unit, which batch size).  The block's
      // largest element sits at most EQ - 1 = 7 bits under the range: an element keeps its 22 significand bits down to 2^-12 of such a block
      // maximum, and an absolute error of 2^-34 of that maximum below.  Neighbouring blocks share an exponent unless their maxima lie on
      // either side of a multiple of 2^8: the consumers rescale accumulators only there (rarely).  A block without a finite nonzero element
      // keeps the exponent of the block split before it: whatever that is, every product with the block is 0 (or not finite) and the rescale
      // around it exact, so it changes no bit -- and a block of zeros behind a loud one asks no rise of 2^(100 - e) from the accumulators.
      // Between two blocks with nonzero elements the rise is their needs' difference (at most 2^(100 - need), the clamp below): the
      // accumulators (under 2^39) stay finite unless the two maxima are more than 2^80 apart.
      int need = f16_scale_exp(m) - 1;
      need = need < 100 ? need : 100;                  // 2^e and the epilogue's 2^-(e + weight exponent) stay normal floats
      const int e = m > 0.f ? need & ~(CFG::EQ - 1) : e_prev;
      e_prev = e;
      if (ptid == 0) exps[slot3] = e;
      const float sc = __builtin_ldexpf(1.0f, e);
      char *dst = lds + CFG::X_OFF + slot3 * 4 * CFG::ROWB + loff;
      if constexpr ((ABL & 8) != 0) return;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned hh[4], ll[4];
#pragma unroll
        for (int c2 = 0; c2 < 4; ++c2) conv3h_split_pair(raw[S][2 * c2][i], raw[S][2 * c2 + 1][i], sc, hh[c2], ll[c2]);
        const bool wok = item_ok && (i == 3 ? q <= 8 : (i == 0 ? q >= 1 : (q >= 1 && q <= 8)));   // window column 4 q - 3 + i in 0..33
        if (wok) {
          *reinterpret_cast<u32x4 *>(dst + i * CFG::PSTR) = (u32x4){hh[0], hh[1], hh[2], hh[3]};
          *reinterpret_cast<u32x4 *>(dst + CFG::PART + i * CFG::PSTR) = (u32x4){ll[0], ll[1], ll[2], ll[3]};
        }
      }
    };

    // step s (the consumers work on block s): block s + 4 is FETCHED first (its loads start the step: the memory pipe must not idle while
    // the split runs), then block s + 2's maximum is published (loads of the previous step), then block s + 1 is split into its ring slot
    // (maximum of the previous step).  Steps are identical whatever blocks exist.
    int stepno = 0;
    auto stamp = [&](int slot) {
      if constexpr ((ABL & 32) != 0) {
        if (wg == 0 && pw == 0 && stepno < 64) {
          const long long t = __builtin_amdgcn_s_memtime();
          if (lane == 0) a.dbg[stepno * 8 + slot] = t;
        }
      }
    };
    fetch(IntC<0>{});
    fetch(IntC<1>{});
    fetch(IntC<2>{});
    fetch(IntC<3>{});
    tile_max(IntC<0>{}, 0);
    __syncthreads();                                   // (P0) weights in LDS, maxima of block 0
    tile_max(IntC<1>{}, 1);
    split_store(IntC<0>{}, 0, 0);
    __syncthreads();                                   // (P1) ring slot 0, maxima of block 1
    int s3 = 1;                                        // (s + 1) % 3
    auto step = [&](auto r4, int s) {                  // R = s % 4
      constexpr int R = decltype(r4)::value;
      stamp(0);
      if constexpr ((ABL & 32) != 0) {
        if ((wg == 0 || wg == 9 || wg == 100 || wg == 255) && pw == 0 && stepno < 2048) {
          const long long t = __builtin_amdgcn_s_memtime();
          if (lane == 0) a.dbg[512 + (wg == 0 ? 0 : (wg == 9 ? 1 : (wg == 100 ? 2 : 3))) * 2048 + stepno] = t;
        }
      }
      // the three phases touch different register sets and tables: any order is valid.  Waves 4 / 5 fetch first, waves 6 / 7 last, so
      // that the CU's address unit sees half of the loads at either end of the step instead of all 32 at once
      if ((ABL & 1024) != 0 || pw < 2) {
        fetch(IntC<R>{});                              // block s + 4 (set R: block s was split in step s - 1)
        stamp(1);
        tile_max(IntC<(R + 2) % 4>{}, s & 1);          // block s + 2 (its loads are two steps old)
        stamp(2);
        split_store(IntC<(R + 1) % 4>{}, (s + 1) & 1, s3);   // block s + 1
        stamp(3);
      } else {
        split_store(IntC<(R + 1) % 4>{}, (s + 1) & 1, s3);
        tile_max(IntC<(R + 2) % 4>{}, s & 1);
        fetch(IntC<R>{});
      }
      __syncthreads();
      ++stepno;
      s3 = s3 == 2 ? 0 : s3 + 1;
    };
    for (int s = 0; s < NB; s += 4) {
      step(IntC<0>{}, s);
      if (s + 1 < NB) step(IntC<1>{}, s + 1);
      if (s + 2 < NB) step(IntC<2>{}, s + 2);
      if (s + 3 < NB) step(IntC<3>{}, s + 3);
    }
  } else {
    // =================================================================== consumer ===================================================
    // One body per stage program (Conv3hCfg::PLAN): wave 1 runs program 1, waves 0, 2, 3 program 0 -- one wave-uniform branch per launch
    auto consume = [&](auto progc) {
    constexpr int PROG = decltype(progc)::value;
    constexpr CFG::Stage MST = CFG::plan_find(PROG, CFG::MERGED), PST = CFG::plan_find(PROG, CFG::PADDED);
    const int li = lane & 15, g = lane >> 4;
    int vl[CFG::SPK];                                  // lane part of the x fragment address per stage of a kernel row: (kx + pixel) * 96 + channel group * 16
#pragma unroll
    for (int sg = 0; sg < CFG::SPK; ++sg) {
      int kk = 4 * sg + g;
      kk = kk < CFG::KGY ? kk : CFG::KGY - 2 + (g & 1);   // half stages: lanes g >= 2 re-read groups 16 / 17 (an odd slot distance: no bank conflict) -- of the second row (merged) or against a zero weight fragment (padded)
      vl[sg] = (kk / CFG::CG8 + li) * CFG::PSTR + (kk % CFG::CG8) * 16 + CFG::X_OFF;
    }
    const char *wl = lds + CFG::W_OFF + lane * 16;
    // padded half stage: lanes without a k group behind them (k groups 18, 19) read a 16-byte slot of zeros as their WEIGHT fragment (their x
    // fragment is the real data of k group 17 -- finite whenever the tile's legitimate operands are)
    // merged stage: lanes g < 2 read the half fragment of row MST.ky, lanes g >= 2 that of row MST.kyb (k group 16 + (g & 1) either way)
    const bool pad_lane = g >= (CFG::KGY % 4);
    int whp[3][2], whm[3][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int hf = CFG::W_OFF + (CFG::SPK - 1) * 6144 + (c * 2 + p) * 512 + (lane & 31) * 16;
        whp[c][p] = pad_lane ? CFG::TAB_OFF + 48 : hf + PST.ky * CFG::WKY;
        whm[c][p] = hf + (pad_lane ? MST.kyb : MST.ky) * CFG::WKY;
      }
    if (tid < 4) reinterpret_cast<unsigned *>(lds + CFG::TAB_OFF + 48)[tid] = 0u;   // (published by barrier P0)
    const int *wexp = reinterpret_cast<const int *>(a.wimg) + CFG::WBYTES / 4;
    int ew[3];
    float bz[3], wsc[3];                               // wsc = 2^-ew (the PS forms: one register per channel tile instead of the exponent and its sum with the tile's)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ew[c] = wexp[c * 16 + li];
      wsc[c] = __builtin_ldexpf(1.0f, -ew[c]);
      bz[c] = a.bias ? a.bias[c * 16 + li] : 0.f;
    }
    // finished tile waiting for its stores (issued in the middle of the next step's MFMAs, when the producers' fetch burst has drained:
    // the address unit takes ~45 cycles per 1-KB store, 24 of them per tile in a row held every consumer wave for ~1250 cycles)
    // A store instruction writes eight channels x one whole 128-byte row (lane: channel li & 7 of the eight, 16-byte chunk (li >> 3) * 4 + g)
    // instead of sixteen channels x half a row: the two pixel tiles of a channel sit in ONE lane (acc[0][c], acc[1][c]), so lanes li and
    // li ^ 8 swap one of them (DPP row_ror:8).  Whole lines, nontemporal: the fetch + store skeleton of this kernel (no arithmetic at all,
    // tools/experimental/micro_fetch.hip) runs 3.97 ms per level-0 launch that way against 4.52 with half-line stores.
    f32x4 pend[6];                                     // store k = (channel tile k / 2, channel half k % 2)
    int pend_vo = 0;                                   // byte offset of (channel li & 7, row, column f0 + chunk * 4) in the batch item (partial out: of the wave's 6 KB, wave-uniform)
    __amdgpu_buffer_rsrc_t pend_rs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, 0, 0x00020000);   // num_records 0: every store dropped
    int soff[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) soff[k] = (int)(((k / 2) * 16 + (k % 2) * 8) * TF * 4);
    const unsigned ps_item = (unsigned)CFG::ps_item_bytes(a.tilesT, a.tilesF);
    // (partial out: never an activation -- a constant, no register)
    const float act_lo = !POUT && a.act == ACT_RELU ? 0.f : -__builtin_inff();
    const int tl_lane = (int)CFG::tl_store_lane(lane);  // YT: the lane's 16 bytes inside a store's 1-KB block

    auto flush_one = [&](auto kc) {
      constexpr int K = decltype(kc)::value;
      if constexpr ((ABL & 4) == 0) {
        if constexpr (POUT) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pend[K]), pend_rs, lane * 16, pend_vo + K * CFG::PS_STORE, (ABL & 512) ? 0 : 2);
        else if constexpr (YT) __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pend[K]), pend_rs, tl_lane, pend_vo + ((K % 2) * 3 + K / 2) * CFG::TL_BLOCK, (ABL & 512) ? 0 : 2);
        else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, pend[K]), pend_rs, pend_vo, soff[K], (ABL & 512) ? 0 : 2);
      } else {
        if (pend[K].x == 1.2345e-30f) a.y[0] = pend[K].y;   // keeps the arithmetic alive in the no-store build
      }
    };
    // The finished tile's accumulators wait in `pacc`; its epilogue (scale, bias, activation, lane swap: ~50 VALU instructions per channel
    // tile) runs among the MFMAs of the NEXT tile's stages 1..6 and its six stores behind stages 8..13 (the last one) -- off the wave's critical path.
    f32x4 pacc[2][3];
    int pend_e = 0;
    // accumulate mode (a.prev): the six lines of the other input slice's partial sums, fetched in the stores' own lane arrangement behind stage 7
    // of the tile they belong to (the previous tile's epilogue has used the registers by then) and added in front of the activation
    // partial in (PIN): the same six registers hold the lane's own quads of the scratch, pprev[k] = accumulator (channel tile k / 2, pixel tile k % 2)
    f32x4 pprev[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pprev[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
    auto epi_chunk = [&](auto kc) {                    // store k of the pending tile: channels (k / 2) * 16 + (k % 2) * 8 .. + 7, one whole 128-byte row each
      constexpr int K = decltype(kc)::value, c = K / 2;
      // exact power of two (|exponent| well inside the float range: weights and activations are) -- the same number either way
      const float sc = PS != 0 ? __builtin_ldexpf(wsc[c], -pend_e) : __builtin_ldexpf(1.0f, -(pend_e + ew[c]));
      if constexpr (OWNQ) {
        // partial out: store k is the lane's own accumulator (channel tile c, pixel tile k % 2) -- the planar form's values (the `fmaxf` against
        // -inf included: it is what the planar form's intermediate launch does to a NaN), four fmas instead of eight and no lane swap
        // YT (final output in tile order): the same store of the lane's own quad, with the launch's activation -- element by element the planar
        // final store's fma, partial-in addition and `fmaxf`
        constexpr int qq = K % 2;
        f32x4 o = (f32x4){__builtin_fmaf(pacc[qq][c].x, sc, bz[c]), __builtin_fmaf(pacc[qq][c].y, sc, bz[c]), __builtin_fmaf(pacc[qq][c].z, sc, bz[c]),
                          __builtin_fmaf(pacc[qq][c].w, sc, bz[c])};
        if constexpr (PIN) o += pprev[K];
        pend[K] = (f32x4){fmaxf(o.x, act_lo), fmaxf(o.y, act_lo), fmaxf(o.z, act_lo), fmaxf(o.w, act_lo)};
        return;
      }
      f32x4 v[2];
#pragma unroll
      for (int qq = 0; qq < 2; ++qq) {
        v[qq].x = __builtin_fmaf(pacc[qq][c].x, sc, bz[c]);
        v[qq].y = __builtin_fmaf(pacc[qq][c].y, sc, bz[c]);
        v[qq].z = __builtin_fmaf(pacc[qq][c].z, sc, bz[c]);
        v[qq].w = __builtin_fmaf(pacc[qq][c].w, sc, bz[c]);
        if constexpr (PIN) v[qq] += pprev[c * 2 + qq];   // in front of the lane swap: the element's own partial sum, where the planar form adds it
      }
      // even k: lanes li < 8 keep their own pixel tile 0, lanes li >= 8 take pixel tile 1 of lane li - 8; odd k: lanes li >= 8 keep their own
      // pixel tile 1, lanes li < 8 take pixel tile 0 of lane li + 8 (`v_mov_b32_dpp row_ror:8` written under a bank mask: one instruction per
      // register).  Either half recomputes the eight scaled values it needs: sixteen VALU instructions per store, one store's worth per stage.
      f32x4 o;
      if constexpr (K % 2 == 0) o = (f32x4){ror8m<0xC>(v[0].x, v[1].x), ror8m<0xC>(v[0].y, v[1].y), ror8m<0xC>(v[0].z, v[1].z), ror8m<0xC>(v[0].w, v[1].w)};
      else o = (f32x4){ror8m<0x3>(v[1].x, v[0].x), ror8m<0x3>(v[1].y, v[0].y), ror8m<0x3>(v[1].z, v[0].z), ror8m<0x3>(v[1].w, v[0].w)};
      if constexpr (ACC) o += pprev[K];
      // ReLU or nothing, without a branch (a branch would end the MFMA scheduling region)
      pend[K] = (f32x4){fmaxf(o.x, act_lo), fmaxf(o.y, act_lo), fmaxf(o.z, act_lo), fmaxf(o.w, act_lo)};
    };
    auto flush = [&]() {
      epi_chunk(IntC<0>{});
      epi_chunk(IntC<1>{});
      epi_chunk(IntC<2>{});
      epi_chunk(IntC<3>{});
      epi_chunk(IntC<4>{});
      epi_chunk(IntC<5>{});
      flush_one(IntC<0>{});
      flush_one(IntC<1>{});
      flush_one(IntC<2>{});
      flush_one(IntC<3>{});
      flush_one(IntC<4>{});
      flush_one(IntC<5>{});
      pend_rs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, 0, 0x00020000);
    };

    __syncthreads();                                   // (P0)
    __syncthreads();                                   // (P1)
    Conv3hWalk wk;
    conv3h_walk_init<MO>(a, wg, wk);
    int s3 = 0;                                        // s % 3
    for (int s = 0; s < NB; ++s) {
      const int tb = wk.b, j = wk.j, wk_strip = wk.strip, wk_t0 = wk.t0, f0 = wk_strip * 32;
      conv3h_walk_next(a, wg, wk);
      if constexpr ((ABL & 32) != 0) {
        if (wg == 0 && wave == 0 && s < 64) {
          const long long t = __builtin_amdgcn_s_memtime();
          if (lane == 0) a.dbg[s * 8 + 4] = t;
        }
      }
      if (j >= 0) {
        // F % 32 == 0 (launcher): a strip is inside the image or outside as a whole; rows past T and padding strips get num_records 0
        const int tt = (wk_t0 + j) * 4 + wave;
        const bool cur_ok = tt < a.T && f0 < a.F;
        const int cur_vo = (((li & 7) * a.T + tt) * a.F + f0 + ((li >> 3) * 4 + g) * 4) * 4;
        // the wave's 6 KB of the scratch: wave-uniform (a scalar offset of the loads and stores), the lane adds lane * 16 (cur_ok: strip < tilesF, tile row < tilesT)
        const int cur_ps = (int)CFG::ps_wave_off(a.tilesT, wk_strip, wk_t0 + j, wave);
        const int cur_tl = (int)CFG::tl_store_off(a.F, tt, f0, 0);   // YT: the wave's row of blocks (wave-uniform; cur_ok: inside the slice)
        // rows of the tile: u = 0, 1 = the last two rows of the previous block, u = 2..5 = this block; wave r, kernel row ky reads u = r + ky
        const int sp = s3 == 0 ? 2 : s3 - 1;
        const int e_cur = __builtin_amdgcn_readfirstlane(exps[s3]), e_old = __builtin_amdgcn_readfirstlane(exps[sp]);
        int rowoff[3], eky[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          const int u = wave + ky;
          rowoff[ky] = (u < 2 ? sp * 4 + 2 + u : s3 * 4 + u - 2) * CFG::ROWB;
          eky[ky] = u < 2 ? e_old : e_cur;
        }
        const int xm = (pad_lane ? rowoff[MST.kyb] : rowoff[MST.ky]) + vl[CFG::SPK - 1];   // merged stage: the lane's row (both rows in one block slot)
        f32x4 acc[2][3];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int c = 0; c < 3; ++c) acc[p][c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        constexpr int PF = (ABL & 2048) ? 2 : 1;     // stages of fragment reads in flight ahead of the MFMAs (register sets: PF + 1); 2 measured 2 % slower (224 registers)
        f16x8 wf[PF + 1][3][2], xf[PF + 1][2][2];
        auto load_stage = [&](auto bufc, auto sc) {
          constexpr int BUF = decltype(bufc)::value, S = decltype(sc)::value;
          constexpr CFG::Stage ST = CFG::PLAN[PROG][S];
          constexpr int KY = ST.ky, SG = ST.sg;
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              if constexpr (ST.kind == CFG::MERGED) wf[BUF][c][p] = *reinterpret_cast<const f16x8 *>(lds + whm[c][p]);
              else if constexpr (ST.kind == CFG::PADDED) wf[BUF][c][p] = *reinterpret_cast<const f16x8 *>(lds + whp[c][p]);
              else wf[BUF][c][p] = *reinterpret_cast<const f16x8 *>(wl + KY * CFG::WKY + SG * 6144 + (c * 2 + p) * 1024);
            }
          const char *xs = lds + (ST.kind == CFG::MERGED ? xm : rowoff[KY] + vl[SG]);
#pragma unroll
          for (int qq = 0; qq < 2; ++qq)
#pragma unroll
            for (int p = 0; p < 2; ++p) {
              xf[BUF][qq][p] = *reinterpret_cast<const f16x8 *>(xs + qq * 16 * CFG::PSTR + p * CFG::PART);
            }
        };
        auto mfma_stage = [&](auto bufc) {
          constexpr int BUF = decltype(bufc)::value;
          // smallest terms first; the six accumulators of a product are independent
#pragma unroll
          for (int qq = 0; qq < 2; ++qq)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[qq][c] = ASX_MFMA_F16(xf[BUF][qq][0], wf[BUF][c][1], acc[qq][c]);
#pragma unroll
          for (int qq = 0; qq < 2; ++qq)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[qq][c] = ASX_MFMA_F16(xf[BUF][qq][1], wf[BUF][c][0], acc[qq][c]);
#pragma unroll
          for (int qq = 0; qq < 2; ++qq)
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[qq][c] = ASX_MFMA_F16(xf[BUF][qq][0], wf[BUF][c][0], acc[qq][c]);
        };
        // The fragments of stage s + 1 are read while the MFMAs of stage s issue: one `ds_read_b128` in front of every second MFMA
        // (scheduling groups; left alone, hipcc reads each fragment right before its first use and waits for it)
        __builtin_amdgcn_sched_barrier(0);
        load_stage(IntC<0>{}, IntC<0>{});
        if constexpr (PF == 2) load_stage(IntC<1>{}, IntC<1>{});
        __builtin_amdgcn_sched_barrier(0);
        auto run = [&](auto sc, auto &&self) {
          constexpr int S = decltype(sc)::value;
          if constexpr (S + PF < CFG::NST) load_stage(IntC<(S + PF) % (PF + 1)>{}, IntC<S + PF>{});
          mfma_stage(IntC<S % (PF + 1)>{});
          constexpr bool EPI = (ABL & 128) == 0 && S >= 1 && S <= 6;
          if constexpr (EPI) epi_chunk(IntC<S - 1>{});   // the previous tile's epilogue, one store's worth per stage, among this stage's MFMAs
          if constexpr (S + PF < CFG::NST) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
              __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one DS read
              __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // two MFMA
              if constexpr (EPI) __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);   // two VALU of the epilogue chunk
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (PIN && S == 7) {
            __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(static_cast<char *>(a.ps) + (int64_t)tb * a.ps_bstride, 0, cur_ok ? ps_item : 0u, 0x00020000);
#pragma unroll
            for (int k = 0; k < 6; ++k) pprev[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, lane * 16, cur_ps + k * CFG::PS_STORE, 0));
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr (ACC && S == 7) {
            __amdgpu_buffer_rsrc_t prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.prev + (int64_t)tb * a.y_bstride), 0, cur_ok ? plane_bytes : 0u, 0x00020000);
#pragma unroll
            for (int k = 0; k < 6; ++k) pprev[k] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(prs, cur_vo, soff[k], 0));
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr ((ABL & 128) == 0 && S >= 8 && S <= 13) {
            flush_one(IntC<S - 8>{});                  // the previous tile's stores, one per stage: behind the producers' fetch burst, never two in a row
            if constexpr (S == 13) pend_rs = __builtin_amdgcn_make_buffer_rsrc(a.y, 0, 0, 0x00020000);
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr ((ABL & 256) == 0 && CFG::PLAN[PROG][S].rto >= 0) {
            // the stages that follow read rows of the other block -- bring the accumulators to that block's scale (exact;
            // a rise is the difference of two blocks' needs (split_store), a fall flushes what is negligible against what follows)
            const int d = eky[CFG::PLAN[PROG][S].rto] - eky[CFG::PLAN[PROG][S].rfrom];
            if (d != 0) {
#pragma unroll
              for (int qq = 0; qq < 2; ++qq)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                  acc[qq][c].x = __builtin_ldexpf(acc[qq][c].x, d);
                  acc[qq][c].y = __builtin_ldexpf(acc[qq][c].y, d);
                  acc[qq][c].z = __builtin_ldexpf(acc[qq][c].z, d);
                  acc[qq][c].w = __builtin_ldexpf(acc[qq][c].w, d);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
          }
          if constexpr (S + 1 < CFG::NST) self(IntC<S + 1>{}, self);
        };
        run(IntC<0>{}, run);
        if constexpr ((ABL & 32) != 0) {
          if (wg == 0 && wave == 0 && s < 64) {
            const long long t = __builtin_amdgcn_s_memtime();
            if (lane == 0) a.dbg[s * 8 + 5] = t;
          }
        }
        // ---- the accumulators wait for the next step (epi_chunk)
#pragma unroll
        for (int qq = 0; qq < 2; ++qq)
#pragma unroll
          for (int c = 0; c < 3; ++c) pacc[qq][c] = acc[qq][c];
        pend_e = e_cur;
        if constexpr (POUT) {
          pend_rs = __builtin_amdgcn_make_buffer_rsrc(static_cast<char *>(a.ps) + (int64_t)tb * a.ps_bstride, 0, cur_ok ? ps_item : 0u, 0x00020000);
          pend_vo = cur_ps;
        } else {
          pend_rs = __builtin_amdgcn_make_buffer_rsrc(a.y + (int64_t)tb * a.y_bstride, 0, cur_ok ? plane_bytes : 0u, 0x00020000);
          pend_vo = YT ? cur_tl : cur_vo;
        }
        if constexpr ((ABL & 128) != 0) flush();
      } else {
        flush();                                       // first block of an item: nothing to compute yet
      }
      if constexpr ((ABL & 32) != 0) {
        if (wg == 0 && wave == 0 && s < 64) {
          const long long t = __builtin_amdgcn_s_memtime();
          if (lane == 0) a.dbg[s * 8 + 6] = t;
        }
      }
      __syncthreads();
      s3 = s3 == 2 ? 0 : s3 + 1;
    }
    flush();
    };
    static_assert(CFG::NPROG == 2 && CFG::PROG_OF_WAVE[0] == 0 && CFG::PROG_OF_WAVE[1] == 1 && CFG::PROG_OF_WAVE[2] == 0 && CFG::PROG_OF_WAVE[3] == 0, "the branch below is the table");
    if (wave == 1) consume(IntC<1>{});
    else consume(IntC<0>{});
  }
}

}  // namespace asx
