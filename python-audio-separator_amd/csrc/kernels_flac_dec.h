// FLAC decoder of asx_flac_decode_scan_dev / asx_flac_decode_finish_dev for gfx950: the audio part of a stream (RFC 9639; everything behind
// the last metadata block) in HBM -> the planar float32 mix [2, n] that libsndfile gives for the file (x / 2^(bits - 1)).  1 or 2 channels,
// 8 .. 24 bits per sample, block sizes up to 16384, fixed or variable.
//
// A stream carries no index of its frames, a frame's length is known only once it is parsed, and the sync code also occurs inside frames.
// So every frame that could be one is decoded, and the host keeps those that follow each other from byte 0 (flac_dec_plan.h):
//
// flac_sync_kernel   one thread per byte position: the sync code, every header field (reserved bits and codes, the coded number, the block
//                    size and rate extras), sample rate / bits / channels equal to STREAMINFO's, block size within its maximum, the CRC-8.
//                    Survivors go to a candidate list through an atomic counter, in no particular order.  Two candidates are at least 5
//                    bytes apart (bytes 2, 3 and 4 of a header cannot be 0xff), which bounds the list.
// flac_frame_kernel  one wave per candidate.  The compressed bytes come through a window in LDS that all lanes fill with aligned 32-bit loads;
//                    lane 0 parses from it -- subframe headers, warm-up samples, coefficients, Rice or escape-coded residuals into LDS -- as
//                    a resumable sequence of steps, handing back to the wave whenever the window runs short.  Then one lane per channel
//                    restores the predictor (64-bit sum, arithmetic shift), and all lanes shift in the wasted bits, take the frame's CRC-16
//                    (64 bytes per lane and window, combined as the encoder combines its chunks) and store the two channels, still
//                    decorrelated, into the candidate's slot [2][max_blocksize].  A candidate is arbitrary bits: every read is checked against
//                    the frame's bound (min(end of the data, pos + STREAMINFO's max_framesize, or the worst case when that is 0)), every LDS
//                    index against the block size, and whatever a decoder must refuse clears `ok` in the candidate's record.
// flac_finish_kernel one workgroup per accepted frame: undoes left/side, side/right and mid/side, converts and writes the mix, reduces max |x|.
//
// Written with the phase macros of kernels_flac.h, whose CRC and header-code functions it shares: with ASX_FLAC_HOST the same text runs on
// the host, lanes one after another (tools/flac_host_decode.cpp).
#pragma once
#include "kernels_flac.h"

namespace asx {
namespace flacdec {

constexpr int NT = 64;               // lanes per candidate: one wave
constexpr int MIN_BLOCK = 16;
constexpr int MAX_BLOCK = 16384;     // 2 x 16384 x 4 bytes of samples + window + state fit a CU's 160 KiB of LDS
constexpr int HEADER_MAX = 16;       // sync 2, sizes/rate 1, channels/width 1, coded number <= 7, block size <= 2, rate <= 2, CRC-8 1
constexpr int WIN_WORDS = 1024;      // the window: 4 KiB of the stream
constexpr int WIN_BITS = WIN_WORDS * 32;
constexpr int STAGE_WORDS = WIN_WORDS + 2;
constexpr int MAX_ORDER = 32;
constexpr int REC_WORDS = 5;         // a candidate's record: pos, end, blocksize, assignment, ok
constexpr int SYNC_THREADS = 256;
constexpr int FINISH_THREADS = 256;
static_assert(WIN_WORDS * 4 == NT * flac::CRC_CHUNK, "a window is one CRC chunk per lane");

struct Info {                        // STREAMINFO, as far as the frames must agree with it
  int32_t sample_rate, channels, bps, max_blocksize, max_framesize;
};
struct Header {
  int32_t blocksize, assignment, channels, bytes;    // bytes: the header's length with its CRC-8
};
struct Accept {                      // a frame of the chain: its slot and where its samples go
  int32_t slot, blocksize, assignment, pad;
  int64_t out;
};

// the frame bound when STREAMINFO does not give one: twice a verbatim frame
FLAC_FN int64_t worst_frame_bytes(int nch, int bps, int bs) { return 2 * (32 + (int64_t)nch * (bps + 2) * bs / 8); }

// h: the first `avail` <= HEADER_MAX bytes at a position.  True when they begin a frame header this stream can contain.
FLAC_FN bool parse_header(const uint8_t *h, int avail, const Info &I, Header &H) {
  if (avail < 6 || h[0] != 0xffu || (h[1] & 0xfeu) != 0xf8u) return false;
  const int bs_code = h[2] >> 4, sr_code = h[2] & 15, assign = h[3] >> 4, ss_code = (h[3] >> 1) & 7;
  if ((h[3] & 1) || bs_code == 0 || sr_code == 15 || assign > 10 || ss_code == 3 || ss_code == 7) return false;
  int n = 4;
  const uint32_t lead = h[n++];
  if (lead >= 0x80u) {               // the frame or sample number, coded like UTF-8 with up to 6 continuation bytes
    int extra = 0;
    while (extra < 7 && (lead & (0x40u >> extra))) ++extra;
    if (extra == 0 || extra > 6) return false;
    for (int i = 0; i < extra; ++i) {
      if (n >= avail || (h[n] >> 6) != 2) return false;
      ++n;
    }
  }
  int bs = flac::table_block_size(bs_code);
  if (bs_code == 6) {
    if (n + 1 > avail) return false;
    bs = (int)h[n] + 1;
    n += 1;
  } else if (bs_code == 7) {
    if (n + 2 > avail) return false;
    bs = (((int)h[n] << 8) | (int)h[n + 1]) + 1;
    n += 2;
  }
  int sr = sr_code == 0 ? I.sample_rate : flac::table_sample_rate(sr_code);
  if (sr_code == 12) {
    if (n + 1 > avail) return false;
    sr = (int)h[n] * 1000;
    n += 1;
  } else if (sr_code == 13 || sr_code == 14) {
    if (n + 2 > avail) return false;
    sr = (((int)h[n] << 8) | (int)h[n + 1]) * (sr_code == 14 ? 10 : 1);
    n += 2;
  }
  if (n >= avail) return false;
  const int widths[8] = {0, 8, 12, 0, 16, 20, 24, 0};
  const int bps = ss_code == 0 ? I.bps : widths[ss_code];
  const int nch = assign >= 8 ? 2 : assign + 1;
  if (sr != I.sample_rate || bps != I.bps || nch != I.channels || bs > I.max_blocksize) return false;
  uint32_t crc = 0;
  for (int i = 0; i < n; ++i) crc = flac::crc8_byte(crc, h[i]);
  if (crc != h[n]) return false;
  H.blocksize = bs;
  H.assignment = assign;
  H.channels = nch;
  H.bytes = n + 1;
  return true;
}

// position `pos` of the audio part `a` of `nbytes`: a candidate?
FLAC_FN bool sync_at(const uint8_t *a, int64_t nbytes, int64_t pos, const Info &I) {
  if (pos + 6 > nbytes || a[pos] != 0xffu || (a[pos + 1] & 0xfeu) != 0xf8u) return false;
  uint8_t h[HEADER_MAX];
  const int avail = (int)((nbytes - pos) < HEADER_MAX ? (nbytes - pos) : HEADER_MAX);
  for (int i = 0; i < HEADER_MAX; ++i) h[i] = i < avail ? a[pos + i] : (uint8_t)0;
  Header H;
  return parse_header(h, avail, I, H);
}

// ---- the frame parser ---------------------------------------------------------------------------------------------------------------
enum Step { ST_HEADER, ST_SUB, ST_CONST, ST_VERBATIM, ST_WARMUP, ST_LPC, ST_COEF, ST_RESIDUAL, ST_PARTITION, ST_CODES, ST_NEXT, ST_FOOT };

struct Sub {
  int32_t type;                      // 0 constant, 1 verbatim, 2 predicted
  int32_t order, shift, wasted, bits, precision;
  int32_t coef[MAX_ORDER];
};
struct State {
  Sub sub[2];
  uint32_t pos, nbytes, limit;       // the candidate, the end of the data, the frame's bound (absolute bytes)
  uint32_t wabs, rb;                 // the window's first byte (a multiple of 4) and the parser's bit position in it
  int32_t step, c, i, j;             // channel, sample index, coefficient or partition index
  int32_t method, po, k, part_end;   // k < 0: an escape partition of -1 - k bits per residual
  uint32_t q;                        // zeros of a unary run counted so far
  int32_t done, ok;
  int32_t blocksize, assignment, nch;
  uint32_t end, crc_stored, crc;
  uint32_t crcs[NT];
};

constexpr int OFF_STATE = STAGE_WORDS * 4 + 8;            // 16-byte aligned
static_assert(OFF_STATE % 16 == 0, "state alignment");
FLAC_FN int lds_bytes(int max_blocksize) { return OFF_STATE + (int)((sizeof(State) + 15) / 16 * 16) + 2 * max_blocksize * 4; }
static_assert(OFF_STATE + (sizeof(State) + 15) / 16 * 16 + 2 * MAX_BLOCK * 4 <= 160 * 1024, "a candidate's working set must fit a CU's 160 KiB of LDS");

FLAC_FN uint32_t bswap32(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24); }
// 32 bits of the stream from bit `rb` of the window (rb + 64 <= WIN_BITS keeps both words inside it)
FLAC_FN uint32_t peek32(const uint32_t *stage, uint32_t rb) {
  const uint32_t w = rb >> 5, o = rb & 31u;
  const uint32_t hi = bswap32(stage[w]);
  if (o == 0) return hi;
  return (hi << o) | (bswap32(stage[w + 1]) >> (32u - o));
}
FLAC_FN uint32_t take(const uint32_t *stage, uint32_t &rb, int n) {          // 0 <= n <= 32
  if (n == 0) return 0u;
  const uint32_t v = peek32(stage, rb) >> (32 - n);
  rb += (uint32_t)n;
  return v;
}
FLAC_FN int32_t take_signed(const uint32_t *stage, uint32_t &rb, int n) {    // 1 <= n <= 32
  const uint32_t v = peek32(stage, rb) & ~((n < 32) ? (0xffffffffu >> n) : 0u);
  rb += (uint32_t)n;
  return (int32_t)v >> (32 - n);
}
FLAC_FN int clz32(uint32_t v) {      // v != 0
#ifdef ASX_FLAC_HOST
  return __builtin_clz(v);
#else
  return __clz((int)v);
#endif
}
FLAC_FN uint32_t load32(const uint8_t *p) {   // p is 4-byte aligned
#ifdef ASX_FLAC_HOST
  uint32_t v;
  memcpy(&v, p, 4);
  return v;
#else
  return *reinterpret_cast<const uint32_t *>(p);
#endif
}
FLAC_FN uint32_t stage_byte(const uint32_t *stage, uint32_t b) { return (stage[b >> 2] >> (8u * (b & 3u))) & 255u; }

// all lanes: the STAGE_WORDS words of the data from byte `wabs` (a multiple of 4), zero past the end of the data
#define FLACDEC_LOAD_WINDOW(stage, a, nbytes, wabs)                                                     \
  FLAC_LANES_OF(NT) {                                                                                   \
    for (int w_ = tid; w_ < STAGE_WORDS; w_ += NT) {                                                    \
      const uint64_t b_ = (uint64_t)(wabs) + 4ull * (uint64_t)w_;                                       \
      uint32_t v_ = 0u;                                                                                 \
      if (b_ + 4ull <= (uint64_t)(nbytes)) {                                                            \
        v_ = load32((a) + b_);                                                                          \
      } else {                                                                                          \
        for (int t_ = 0; t_ < 4; ++t_)                                                                  \
          if (b_ + (uint64_t)t_ < (uint64_t)(nbytes)) v_ |= (uint32_t)(a)[b_ + (uint64_t)t_] << (8 * t_); \
      }                                                                                                 \
      (stage)[w_] = v_;                                                                                 \
    }                                                                                                   \
  }

// Lane 0: parse from the window until the frame is done (S.done, with S.ok) or the window runs short; then the window is moved up to the
// parser's position for the wave to fill it again.  x: the two channels [2][xs] in LDS.
FLAC_FN void parse_some(State &S, const uint32_t *stage, int32_t *x, int xs, const Info &I) {
  uint32_t rb = S.rb;
  int i = S.i;
  uint32_t q = S.q;
  // the bound as a bit position of this window (clipped: rb never passes WIN_BITS)
  uint32_t lim = S.limit > S.wabs ? ((S.limit - S.wabs) > (uint32_t)(WIN_WORDS * 8) ? (uint32_t)(WIN_BITS * 2) : (S.limit - S.wabs) * 8u) : 0u;
  bool fail = false, finished = false;
#define NEED_WINDOW() \
  if (rb + 64u > (uint32_t)WIN_BITS) break
#define WITHIN(n) (rb + (uint32_t)(n) <= lim)
  for (;;) {
    bool short_window = true;        // leaving the switch by `break` before this is cleared: the window ran short
    Sub &sub = S.sub[S.c < 2 ? S.c : 1];
    int32_t *xc = x + (S.c < 2 ? S.c : 1) * xs;
    const int bs = S.blocksize;
    switch (S.step) {
      case ST_HEADER: {
        if (rb + 8u * HEADER_MAX + 64u > (uint32_t)WIN_BITS) break;
        uint8_t h[HEADER_MAX];
        uint32_t p = rb;
        for (int t = 0; t < HEADER_MAX; ++t) h[t] = (uint8_t)take(stage, p, 8);
        const uint32_t left = S.nbytes - S.pos;
        Header H;
        if (!parse_header(h, (int)(left < HEADER_MAX ? left : HEADER_MAX), I, H)) {
          fail = true;
          break;
        }
        rb += 8u * (uint32_t)H.bytes;
        S.blocksize = H.blocksize;
        S.assignment = H.assignment;
        S.nch = H.channels;
        const int64_t bound = I.max_framesize > 0 ? (int64_t)I.max_framesize : worst_frame_bytes(H.channels, I.bps, H.blocksize);
        if ((int64_t)S.pos + bound < (int64_t)S.nbytes) S.limit = (uint32_t)((int64_t)S.pos + bound);
        lim = S.limit > S.wabs ? ((S.limit - S.wabs) > (uint32_t)(WIN_WORDS * 8) ? (uint32_t)(WIN_BITS * 2) : (S.limit - S.wabs) * 8u) : 0u;
        S.c = 0;
        S.step = ST_SUB;
        short_window = false;
        break;
      }
      case ST_SUB: {
        NEED_WINDOW();
        short_window = false;
        if (!WITHIN(8)) { fail = true; break; }
        const uint32_t v = take(stage, rb, 8);
        if (v & 0x80u) { fail = true; break; }
        const int kind = (int)((v >> 1) & 63u);
        int wasted = 0;
        if (v & 1u) {                // k wasted bits: k - 1 zeros and a one
          const uint32_t t = peek32(stage, rb);
          if (t == 0u) { fail = true; break; }
          wasted = clz32(t) + 1;
          if (!WITHIN(wasted)) { fail = true; break; }
          rb += (uint32_t)wasted;
        }
        const int a = S.assignment;
        const bool side = (a == 8 && S.c == 1) || (a == 9 && S.c == 0) || (a == 10 && S.c == 1);
        sub.wasted = wasted;
        sub.bits = I.bps + (side ? 1 : 0) - wasted;
        if (sub.bits < 1) { fail = true; break; }
        sub.order = 0;
        sub.shift = 0;
        i = 0;
        if (kind == 0) {
          sub.type = 0;
          S.step = ST_CONST;
        } else if (kind == 1) {
          sub.type = 1;
          S.step = ST_VERBATIM;
        } else if ((kind >= 8 && kind <= 12) || kind >= 32) {
          sub.type = 2;
          sub.order = kind < 32 ? kind - 8 : kind - 31;
          sub.precision = kind < 32 ? 0 : 1;
          if (sub.order > bs) { fail = true; break; }
          S.step = ST_WARMUP;
        } else {
          fail = true;
        }
        break;
      }
      case ST_CONST: {
        NEED_WINDOW();
        short_window = false;
        if (!WITHIN(sub.bits)) { fail = true; break; }
        xc[0] = take_signed(stage, rb, sub.bits);
        S.step = ST_NEXT;
        break;
      }
      case ST_VERBATIM:
      case ST_WARMUP: {
        const int n = S.step == ST_VERBATIM ? bs : sub.order;
        const int bits = sub.bits;
        while (i < n) {
          if (rb + 64u > (uint32_t)WIN_BITS) break;
          if (!WITHIN(bits)) { fail = true; break; }
          xc[i++] = take_signed(stage, rb, bits);
        }
        if (fail || i < n) break;
        short_window = false;
        if (S.step == ST_VERBATIM) {
          S.step = ST_NEXT;
        } else if (sub.precision == 0) {                 // a fixed predictor as coefficients
          const int fixed[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};
          for (int t = 0; t < sub.order; ++t) sub.coef[t] = fixed[sub.order][t];
          S.step = ST_RESIDUAL;
        } else {
          S.step = ST_LPC;
        }
        break;
      }
      case ST_LPC: {
        NEED_WINDOW();
        short_window = false;
        if (!WITHIN(9)) { fail = true; break; }
        sub.precision = (int)take(stage, rb, 4) + 1;
        sub.shift = take_signed(stage, rb, 5);
        if (sub.precision == 16 || sub.shift < 0) { fail = true; break; }
        S.j = 0;
        S.step = ST_COEF;
        break;
      }
      case ST_COEF: {
        int j = S.j;
        while (j < sub.order) {
          if (rb + 64u > (uint32_t)WIN_BITS) break;
          if (!WITHIN(sub.precision)) { fail = true; break; }
          sub.coef[j++] = take_signed(stage, rb, sub.precision);
        }
        S.j = j;
        if (fail || j < sub.order) break;
        short_window = false;
        S.step = ST_RESIDUAL;
        break;
      }
      case ST_RESIDUAL: {
        NEED_WINDOW();
        short_window = false;
        if (!WITHIN(6)) { fail = true; break; }
        S.method = (int)take(stage, rb, 2);
        S.po = (int)take(stage, rb, 4);
        if (S.method > 1 || (bs & ((1 << S.po) - 1)) != 0 || (bs >> S.po) < sub.order) { fail = true; break; }
        S.j = 0;
        i = sub.order;
        S.step = ST_PARTITION;
        break;
      }
      case ST_PARTITION: {
        if (S.j == (1 << S.po)) {
          short_window = false;
          S.step = ST_NEXT;
          break;
        }
        NEED_WINDOW();
        short_window = false;
        const int pbits = S.method ? 5 : 4;
        if (!WITHIN(pbits + 5)) { fail = true; break; }
        S.k = (int)take(stage, rb, pbits);
        if (S.k == (1 << pbits) - 1) S.k = -1 - (int)take(stage, rb, 5);
        S.part_end = (S.j + 1) * (bs >> S.po);
        q = 0u;
        S.step = ST_CODES;
        break;
      }
      case ST_CODES: {
        const int end = S.part_end, k = S.k;
        if (k < 0) {                 // escape: the residuals verbatim
          const int width = -1 - k;
          while (i < end) {
            if (rb + 64u > (uint32_t)WIN_BITS) break;
            if (!WITHIN(width)) { fail = true; break; }
            xc[i++] = width ? take_signed(stage, rb, width) : 0;
          }
        } else {
          while (i < end) {
            if (rb + 64u > (uint32_t)WIN_BITS) break;
            const uint32_t t = peek32(stage, rb);
            if (t == 0u) {           // 32 more zeros of the unary part
              if (!WITHIN(32)) { fail = true; break; }
              q += 32u;
              rb += 32u;
              continue;
            }
            const int z = clz32(t);
            if (!WITHIN(z + 1 + k)) { fail = true; break; }
            rb += (uint32_t)z + 1u;
            const uint64_t u = ((uint64_t)(q + (uint32_t)z) << k) | (uint64_t)take(stage, rb, k);
            if (u >> 32) { fail = true; break; }         // a residual is a 32-bit number
            xc[i++] = (int32_t)((uint32_t)u >> 1) ^ -(int32_t)((uint32_t)u & 1u);
            q = 0u;
          }
        }
        if (fail || i < end) break;
        short_window = false;
        ++S.j;
        S.step = ST_PARTITION;
        break;
      }
      case ST_NEXT: {
        short_window = false;
        ++S.c;
        S.step = S.c < S.nch ? ST_SUB : ST_FOOT;
        break;
      }
      default: {                     // ST_FOOT: padding to a byte, then the CRC-16
        rb = (rb + 7u) & ~7u;
        NEED_WINDOW();
        short_window = false;
        if (!WITHIN(16)) { fail = true; break; }
        S.crc_stored = take(stage, rb, 16);
        S.end = S.wabs + (rb >> 3);
        finished = true;
        break;
      }
    }
    if (fail || finished || short_window) break;
  }
#undef NEED_WINDOW
#undef WITHIN
  if (fail) S.ok = 0;
  if (fail || finished) S.done = 1;
  // the next window begins at the parser's position
  const uint32_t adv = (rb >> 5) * 4u;
  S.wabs += adv;
  S.rb = rb - adv * 8u;
  S.i = i;
  S.q = q;
}

// x[i] = residual[i] + (sum_j coef[j] x[i - 1 - j] >> shift), the sum in 64 bits
FLAC_FN void restore(int32_t *x, int bs, const Sub &sub) {
  const int order = sub.order, shift = sub.shift;
  for (int i = order; i < bs; ++i) {
    int64_t acc = 0;
    for (int j = 0; j < order; ++j) acc += (int64_t)sub.coef[j] * (int64_t)x[i - 1 - j];
    x[i] = (int32_t)(uint32_t)(uint64_t)((int64_t)x[i] + (acc >> shift));
  }
}

// One candidate.  `lds`: lds_bytes(max_blocksize) of 16-byte aligned workgroup memory.  a: the audio part, 4-byte aligned.
#ifdef ASX_FLAC_HOST
static void decode_candidate(const uint8_t *a, uint32_t nbytes, const Info &I, const uint32_t *cand, uint32_t index, int32_t *slots, int32_t *recs,
                             unsigned char *lds)
#else
static __device__ __forceinline__ void decode_candidate(const uint8_t *a, uint32_t nbytes, const Info &I, const uint32_t *cand, uint32_t index,
                                                        int32_t *slots, int32_t *recs, unsigned char *lds)
#endif
{
  uint32_t *stage = reinterpret_cast<uint32_t *>(lds);
  State &S = *reinterpret_cast<State *>(lds + OFF_STATE);
  const int xs = I.max_blocksize;
  int32_t *x = reinterpret_cast<int32_t *>(lds + OFF_STATE + (sizeof(State) + 15) / 16 * 16);

  FLAC_LANES_OF(NT) {
    if (tid == 0) {
      const uint32_t pos = cand[index];
      S.pos = pos;
      S.nbytes = nbytes;
      S.limit = nbytes;
      S.wabs = pos & ~3u;
      S.rb = (pos & 3u) * 8u;
      S.step = ST_HEADER;
      S.c = 0, S.i = 0, S.j = 0, S.q = 0u;
      S.method = 0, S.po = 0, S.k = 0, S.part_end = 0;
      S.done = 0, S.ok = 1;
      S.blocksize = 0, S.assignment = 0, S.nch = 0;
      S.end = pos, S.crc_stored = 0u, S.crc = 0u;
    }
  }
  FLAC_SYNC();

  // ---- parse: the wave fills the window, lane 0 reads it
  for (;;) {
    FLACDEC_LOAD_WINDOW(stage, a, nbytes, S.wabs)
    FLAC_SYNC();
    FLAC_LANES_OF(NT) {
      if (tid == 0) parse_some(S, stage, x, xs, I);
    }
    FLAC_SYNC();
    if (S.done) break;
  }

  if (S.ok) {
    // ---- constants, predictors, wasted bits
    FLAC_LANES_OF(NT) {
      for (int c = 0; c < S.nch; ++c)
        if (S.sub[c].type == 0) {
          const int32_t v = x[c * xs];
          for (int i = tid; i < S.blocksize; i += NT) x[c * xs + i] = v;
        }
    }
    FLAC_SYNC();
    FLAC_LANES_OF(NT) {
      if (tid < S.nch && S.sub[tid].type == 2) restore(x + tid * xs, S.blocksize, S.sub[tid]);
    }
    FLAC_SYNC();

    // ---- CRC-16 of the frame's bytes before it: a window at a time, one chunk per lane
    const uint32_t nbody = S.end - S.pos - 2u;
    for (uint32_t done = 0; done < nbody; done += (uint32_t)(WIN_WORDS * 4)) {
      const uint32_t first = S.pos + done, wabs = first & ~3u;
      const int nb = (int)((nbody - done) < (uint32_t)(WIN_WORDS * 4) ? (nbody - done) : (uint32_t)(WIN_WORDS * 4));
      const int nchunks = (nb + flac::CRC_CHUNK - 1) / flac::CRC_CHUNK;
      FLACDEC_LOAD_WINDOW(stage, a, nbytes, wabs)
      FLAC_SYNC();
      FLAC_LANES_OF(NT) {
        if (tid < nchunks) {
          const int b0 = tid * flac::CRC_CHUNK, b1 = (b0 + flac::CRC_CHUNK) < nb ? (b0 + flac::CRC_CHUNK) : nb;
          uint32_t crc = 0;
          for (int b = b0; b < b1; ++b) crc = flac::crc16_byte(crc, stage_byte(stage, (first - wabs) + (uint32_t)b));
          S.crcs[tid] = crc;
        }
      }
      FLAC_SYNC();
      FLAC_LANES_OF(NT) {
        if (tid == 0) S.crc = flac::crc16_combine(S.crc, S.crcs, nchunks, nb);
      }
      FLAC_SYNC();
    }
    FLAC_LANES_OF(NT) {
      if (tid == 0 && S.crc != S.crc_stored) S.ok = 0;
    }
    FLAC_SYNC();
  }

  // ---- the slot and the record
  if (S.ok) {
    FLAC_LANES_OF(NT) {
      int32_t *slot = slots + (int64_t)index * 2 * xs;
      for (int c = 0; c < S.nch; ++c) {
        const int w = S.sub[c].wasted;
        for (int i = tid; i < S.blocksize; i += NT) slot[c * xs + i] = (int32_t)((uint32_t)x[c * xs + i] << w);
      }
    }
  }
  FLAC_LANES_OF(NT) {
    if (tid == 0) {
      int32_t *r = recs + (int64_t)index * REC_WORDS;
      r[0] = (int32_t)S.pos;
      r[1] = (int32_t)S.end;
      r[2] = S.blocksize;
      r[3] = S.assignment;
      r[4] = S.ok;
    }
  }
}

// the two subframe channels of a sample -> left and right
FLAC_FN void undo_stereo(int assignment, int64_t a, int64_t b, int64_t &l, int64_t &r) {
  l = a, r = b;
  if (assignment == 8) {             // left / side
    r = a - b;
  } else if (assignment == 9) {      // side / right
    l = a + b;
  } else if (assignment == 10) {     // mid / side
    const int64_t mid = (a * 2) | (b & 1);
    l = (mid + b) >> 1;
    r = (mid - b) >> 1;
  }
}

#ifndef ASX_FLAC_HOST
__global__ __launch_bounds__(SYNC_THREADS) void flac_sync_kernel(const uint8_t *__restrict__ a, int64_t nbytes, Info I, uint32_t *__restrict__ count,
                                                                 uint32_t *__restrict__ cand, uint32_t capacity) {
  for (int64_t pos = (int64_t)blockIdx.x * SYNC_THREADS + threadIdx.x; pos < nbytes; pos += (int64_t)gridDim.x * SYNC_THREADS)
    if (sync_at(a, nbytes, pos, I)) {
      const uint32_t at = atomicAdd(count, 1u);
      if (at < capacity) cand[at] = (uint32_t)pos;
    }
}

__global__ __launch_bounds__(NT) void flac_frame_kernel(const uint8_t *__restrict__ a, uint32_t nbytes, Info I, const uint32_t *__restrict__ cand,
                                                        int32_t *__restrict__ slots, int32_t *__restrict__ recs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char flacdec_lds[];
  decode_candidate(a, nbytes, I, cand, blockIdx.x, slots, recs, flacdec_lds);
}

__global__ __launch_bounds__(FINISH_THREADS) void flac_finish_kernel(const int32_t *__restrict__ slots, const Accept *__restrict__ accept, int max_blocksize,
                                                                     int channels, float scale, int64_t n, float *__restrict__ mix,
                                                                     unsigned int *peak_bits) {
  const Accept A = accept[blockIdx.x];
  const int32_t *s0 = slots + (int64_t)A.slot * 2 * max_blocksize;
  const int32_t *s1 = channels == 2 ? s0 + max_blocksize : s0;       // a mono stream feeds both rows
  float m = 0.f;
  for (int i = (int)threadIdx.x; i < A.blocksize; i += FINISH_THREADS) {
    int64_t l, r;
    undo_stereo(A.assignment, (int64_t)s0[i], (int64_t)s1[i], l, r);
    const float fl = (float)l * scale, fr = (float)r * scale;
    mix[A.out + i] = fl;
    mix[n + A.out + i] = fr;
    m = fmaxf(m, fmaxf(fabsf(fl), fabsf(fr)));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
  __shared__ float wm[FINISH_THREADS / 64];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < FINISH_THREADS / 64; ++w) m = fmaxf(m, wm[w]);
    atomicMax(peak_bits, __float_as_uint(m));
  }
}
#endif

}  // namespace flacdec
}  // namespace asx
