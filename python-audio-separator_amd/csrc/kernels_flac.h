// FLAC encoder of asx_flac_encode_dev for gfx950: interleaved int16 [n, 2] -> the audio frames of a fixed-blocksize, 2-channel stream
// (RFC 9639), 16 bits per sample or 24 (the same values shifted left by 8, every subframe flagging its wasted bits).
//
// The same text with PCM = true is the encoder of asx_flac_encode_pcm_dev: int32 [n, 2] samples of 16 or 24 real bits, no wasted bits,
// S = L - R at bps + 1 bits and M = (L + R) >> 1.  What differs there: exact Rice bits for the parameters 0..23 and partition orders 0..5 (the
// table of a pass must fit the union region), a second minimum per partition over the parameters 0..14 only, so that a subframe takes
// Rice method 0 (4-bit parameters) wherever that is not larger than method 1 (5-bit), and a predictor is dropped when a residual leaves
// the 32 bits the format gives it.  The PCM = false instantiation writes the bytes it always wrote.
//
// flac_encode_kernel: one workgroup per block of `block_size` inter-channel samples (the last block is shorter).  The block's four candidate
// channels L, R, M = (L + R) >> 1 and S = L - R sit in LDS as int32 (24-bit streams: M = L + R with 7 wasted bits, so that M/S still
// restores v << 8 exactly).  Per candidate channel 13 predictors are tried in 13 passes over all four channels: the fixed predictors of
// orders 0..4 and LPC orders 1..8 (Welch-windowed autocorrelation and Levinson-Durbin in float64, coefficients quantised to 15 bits with the
// shift of the stream; the float part only chooses coefficients).  A pass computes the residuals in integers exactly as a decoder restores
// them (64-bit sum, arithmetic right shift), adds (zigzag >> k) for k = 0..14 into a table per finest Rice partition, and from the table
// takes the exact Rice bits (method 0, no escapes) of every admissible partition order 0..6.  The cheapest predictor per channel -- or a
// CONSTANT / VERBATIM subframe when nothing coded is smaller -- then the cheapest of L/R, L/S, S/R, M/S.
//
// Bit packing: the frame is an image of big-endian 32-bit words in LDS, zeroed first.  Code lengths per sample, a scan over the block
// (per-lane sums, one serial pass over the lanes' totals), then every lane ORs its codes into the image (LDS atomics; unary runs are the
// zeros already there).  CRC-8 of the header by one lane; CRC-16 as per-64-byte CRCs by all lanes, combined by one lane through
// multiplications by x^512 mod P.  The frame leaves with 16-byte stores into its slot of `stride` bytes; flac_scan_kernel and
// flac_compact_kernel then pack the slots into one contiguous buffer.
//
// The body is written as phases: inside FLAC_LANES a lane works alone (only LDS atomics cross lanes), FLAC_SYNC separates phases, and no
// local variable that differs between lanes lives across a phase.  With ASX_FLAC_HOST defined the same text compiles for the host with the
// lanes of a phase run one after another (tools/flac_host_encode.cpp; tests/test_host_flac_kernel.py decodes what it writes).
#pragma once
#include <stdint.h>

#ifdef ASX_FLAC_HOST
#include <algorithm>
#include <cmath>
#include <cstring>
#define FLAC_FN static inline
#define FLAC_LANES_OF(N) for (int tid = 0; tid < (N); ++tid)
#define FLAC_SYNC() ((void)0)
#define FLAC_ADD64(p, v) (*(p) += (v))
#define FLAC_OR32(p, v) (*(p) |= (v))
#define FLAC_MIN64(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define FLAC_CLOCK(P) 0ll
#else
#include <hip/hip_runtime.h>
#define FLAC_FN static __host__ __device__ inline
#define FLAC_LANES_OF(N) for (int tid = (int)threadIdx.x, once_ = 0; once_ < 1; ++once_)
#define FLAC_SYNC() __syncthreads()
#define FLAC_ADD64(p, v) atomicAdd((p), (v))
#define FLAC_OR32(p, v) atomicOr((p), (v))
#define FLAC_MIN64(p, v) atomicMin((p), (v))
#define FLAC_CLOCK(P) (((P).cycles != nullptr && threadIdx.x == 0) ? (long long)clock64() : 0ll)   // lane 0's stamps, for the profile only
#endif
#define FLAC_LANES FLAC_LANES_OF(asx::flac::NT)   // the encoder's workgroup; the decoder (kernels_flac_dec.h) names its own lane count

namespace asx {
namespace flac {

constexpr int NT = 512;              // lanes per block
constexpr int MIN_BLOCK = 16;        // the format's smallest block size of a stream
constexpr int MAX_BLOCK = 4608;      // the subset's largest block size at rates up to 48 kHz; the LDS layout is sized for it
constexpr int MAX_ORDER = 8;
constexpr int NPRED = 13;            // passes: fixed orders 0..4, then LPC orders 1..8
constexpr int QLP_BITS = 15;         // coefficient precision in the stream
constexpr int MAX_PO = 6;            // Rice partition orders 0..6
constexpr int NK = 15;               // Rice parameters 0..14 (15 is method 0's escape code)
constexpr int MAX_PO_PCM = 5;        // the int32-sample form: orders 0..5, so that the table of its 24 parameters fits the union region
constexpr int NK_PCM = 24;           // ... parameters 0..23; method 1 above 14 (31 is its escape code)
constexpr int SIDE_BITS = 17;        // the widest subframe sample of the int16 form (also of its shifted 24-bit stream: 8 or 7 bits are wasted)
constexpr int SIDE_BITS_MAX = 25;    // ... and of the int32 form at 24 bits per sample
constexpr int HEADER_MAX = 15;       // sync 2, sizes/rate 1, channels/width 1, frame number <= 6, block size <= 2, rate <= 2, CRC-8 1
constexpr int CRC_CHUNK = 64;

// worst case of one frame: header + 2 x (16 + side_bits * block) bits + padding to a byte + CRC-16 (side_bits: the side channel's sample size)
FLAC_FN int64_t worst_frame_bytes(int64_t bs, int side_bits = SIDE_BITS) { return HEADER_MAX + (2 * (16 + side_bits * bs) + 7) / 8 + 2; }
FLAC_FN int frame_stride(int block_size, int side_bits = SIDE_BITS) { return (int)((worst_frame_bytes(block_size, side_bits) + 15) / 16 * 16); }

// the header's block-size code: a table entry, else 6 / 7 = (size - 1) in 8 / 16 bits behind the frame number
// the block size of a table code 1 .. 5 and 8 .. 15 (0 for the reserved code and for 6 / 7, whose size follows the frame number)
FLAC_FN int table_block_size(int code) {
  return code == 1 ? 192 : (code >= 2 && code <= 5) ? (576 << (code - 2)) : (code >= 8 && code <= 15) ? (256 << (code - 8)) : 0;
}
FLAC_FN int block_size_code(int bs, bool table) {
  if (table)
    for (int c = 1; c <= 15; ++c)
      if (bs == table_block_size(c)) return c;
  return bs <= 256 ? 6 : 7;
}
// the sample rate of a table code 1 .. 11 (0 for every other code)
FLAC_FN int table_sample_rate(int code) {
  const int tab[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  return code >= 1 && code <= 11 ? tab[code] : 0;
}

struct Stream {
  const int32_t *pcm;        // [n] samples, L in the low and R in the high half; the int32 form: [n, 2]
  int64_t n;
  int32_t block_size;
  int32_t bps;               // 16 or 24 (the int16 form at 24: the values shifted left by 8)
  int32_t sr_code;           // the header's sample-rate code ...
  int32_t sr_extra_bits;     // ... and the 0, 8 or 16 bits it puts behind the block size
  uint32_t sr_extra;
  int32_t stride;            // bytes per frame slot, a multiple of 16
  uint8_t *frames;           // [n_blocks, stride]
  int32_t *frame_bytes;      // [n_blocks]
  unsigned long long *cycles;  // NULL, or two sums over the blocks of lane 0's shader clocks: the whole block, its CRC-16 phases
};

// the header's sample-rate fields for a rate the format can carry (1 .. 1048575 Hz)
FLAC_FN void sample_rate_code(int sr, int32_t *code, int32_t *extra_bits, uint32_t *extra) {
  *extra_bits = 0;
  *extra = 0;
  for (int c = 1; c < 12; ++c)
    if (sr == table_sample_rate(c)) {
      *code = c;
      return;
    }
  if (sr <= 65535) {
    *code = 13, *extra_bits = 16, *extra = (uint32_t)sr;
  } else if (sr % 10 == 0 && sr / 10 <= 65535) {
    *code = 14, *extra_bits = 16, *extra = (uint32_t)(sr / 10);
  } else if (sr % 1000 == 0 && sr / 1000 <= 255) {
    *code = 12, *extra_bits = 8, *extra = (uint32_t)(sr / 1000);
  } else {
    *code = 0;               // "see STREAMINFO"
  }
}

struct Small {
  double ac[4][MAX_ORDER + 1];
  unsigned long long cost[4][MAX_PO + 1];
  unsigned long long best_bits[4];
  unsigned long long cost1[4][MAX_PO + 1];             // the int32 form: the same with method 1's parameters
  unsigned long long pk[4][128];                        // per partition [(1 << po) - 1 + j]: min over k <= 14 of (Rice bits << 4 | k) (int32 form: << 5)
  unsigned long long pk1[4][128];                       // the int32 form: min over every k
  int32_t coef[4][NPRED][MAX_ORDER];
  int32_t shift[4][NPRED];
  int32_t valid[4][NPRED];
  int32_t noteq[4], bad[4], sub_bps[4], hdr_bits[4];
  int32_t best_type[4], best_pred[4], best_po[4];      // type: 0 constant, 1 verbatim, 2 predicted (fixed or LPC by best_pred)
  int32_t best_method[4];                               // Rice method of the best predictor: 0 = 4-bit, 1 = 5-bit parameters
  uint32_t csum[2][NT];
  int32_t sel[2];
  uint32_t sub_start[2], res_start[2];
  int32_t frame_len;
  uint32_t crcs[(HEADER_MAX + (2 * (16 + SIDE_BITS_MAX * MAX_BLOCK) + 7) / 8 + 2) / CRC_CHUNK + 2];
  uint8_t kb[4][128];                                   // best parameter of partition j at order po: [(1 << po) - 1 + j]
  uint8_t kb1[4][128];                                  // the int32 form: the same of pk1
  uint8_t best_k[4][64];
};

constexpr int img_words(int side_bits) { return (int)(((HEADER_MAX + (2 * (16 + side_bits * (int64_t)MAX_BLOCK) + 7) / 8 + 2 + 15) / 16 * 16) / 4); }
constexpr int IMG_WORDS = img_words(SIDE_BITS_MAX);     // the int32 form's image; the int16 form's is img_words(SIDE_BITS), and its layout ends sooner
constexpr int UNION_BYTES = 2 * MAX_BLOCK * 4;          // acp [NT][9] doubles = sums [4][64][15] or [4][32][24] u64 (smaller) = res [2][MAX_BLOCK] u32
static_assert(NT % 16 == 0 && (NT / 16) * (MAX_ORDER + 1) <= NT && NT * (MAX_ORDER + 1) * 8 <= UNION_BYTES && 4 * 64 * NK * 8 <= UNION_BYTES &&
                  4 * (1 << MAX_PO_PCM) * NK_PCM * 8 <= UNION_BYTES && MAX_PO_PCM <= MAX_PO && NK_PCM <= 31,
              "union region");
constexpr int OFF_UNION = 4 * MAX_BLOCK * 4;
constexpr int OFF_IMG = OFF_UNION + UNION_BYTES;
constexpr int off_small(bool pcm) { return OFF_IMG + (pcm ? IMG_WORDS : img_words(SIDE_BITS)) * 4; }
constexpr int lds_bytes(bool pcm) { return off_small(pcm) + (int)((sizeof(Small) + 15) / 16 * 16); }
constexpr int LDS_BYTES = lds_bytes(true);              // the larger of the two forms
static_assert(off_small(false) % 16 == 0 && off_small(true) % 16 == 0 && lds_bytes(false) <= LDS_BYTES && LDS_BYTES <= 160 * 1024,
              "one block's working set must fit a CU's 160 KiB of LDS");

// n <= 32 bits of v at bit `pos` of the big-endian image (the image is zero where nothing was written yet)
FLAC_FN void put_bits(uint32_t *img, uint32_t pos, int n, uint32_t v) {
  if (n <= 0) return;
  if (n < 32) v &= (1u << n) - 1u;
  const uint32_t w = pos >> 5;
  const int off = (int)(pos & 31u);
  if (off + n <= 32) {
    FLAC_OR32(&img[w], v << (32 - off - n));
  } else {
    const int r = off + n - 32;
    FLAC_OR32(&img[w], v >> r);
    FLAC_OR32(&img[w + 1], v << (32 - r));
  }
}
FLAC_FN uint32_t img_byte(const uint32_t *img, int i) { return (img[i >> 2] >> (24 - 8 * (i & 3))) & 255u; }
FLAC_FN uint32_t crc16_byte(uint32_t crc, uint32_t b) {
  crc ^= b << 8;
  for (int i = 0; i < 8; ++i) crc = (crc & 0x8000u) ? ((crc << 1) ^ 0x8005u) & 0xffffu : (crc << 1) & 0xffffu;
  return crc;
}
// a * b mod P over GF(2), P = x^16 + x^15 + x^2 + 1
FLAC_FN uint32_t crc16_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 15; i >= 0; --i) {
    r = (r & 0x8000u) ? ((r << 1) ^ 0x8005u) & 0xffffu : (r << 1) & 0xffffu;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// `crc` (the CRC-16 of everything before) continued over `nbytes` more bytes whose CRCs per CRC_CHUNK bytes (the last chunk may be shorter)
// are crcs[0 .. nchunks): one multiplication by x^(8 * chunk bytes) mod P per chunk
FLAC_FN uint32_t crc16_combine(uint32_t crc, const uint32_t *crcs, int nchunks, int nbytes) {
  uint32_t x512 = 1;                            // x^(8 * CRC_CHUNK) mod P: a CRC state moved past one chunk of zero bytes
  for (int b = 0; b < CRC_CHUNK; ++b) x512 = crc16_byte(x512, 0);
  for (int j = 0; j < nchunks; ++j) {
    uint32_t mul = x512;
    if (j == nchunks - 1) {
      mul = 1;
      for (int b = j * CRC_CHUNK; b < nbytes; ++b) mul = crc16_byte(mul, 0);
    }
    crc = crc16_mul(crc, mul) ^ crcs[j];
  }
  return crc;
}
FLAC_FN uint32_t crc8_byte(uint32_t crc, uint32_t b) {
  crc ^= b;
  for (int i = 0; i < 8; ++i) crc = (crc & 0x80u) ? ((crc << 1) ^ 0x07u) & 0xffu : (crc << 1) & 0xffu;
  return crc;
}
FLAC_FN double welch(int i, int bs) {
  const double t = ((double)i - 0.5 * (double)(bs - 1)) / (0.5 * (double)(bs + 1));
  return 1.0 - t * t;
}
// the residual of sample i >= order as the decoder undoes it: x[i] - (sum_j coef[j] x[i - 1 - j] >> shift), the sum in 64 bits (8 taps of
// 2^14 times samples of 2^16 pass 2^32)
FLAC_FN int64_t residual(const int32_t *x, int i, const int32_t *cf, int order, int shift) {
  int64_t acc = 0;
  for (int j = 0; j < order; ++j) acc += (int64_t)cf[j] * (int64_t)x[i - 1 - j];
  return (int64_t)x[i] - (acc >> shift);
}
FLAC_FN int pred_order(int p) { return p < 5 ? p : p - 4; }
// the largest admissible partition order: it divides the block and leaves more than `order` samples to the first partition
FLAC_FN int max_partition_order(int bs, int order, int cap = MAX_PO) {
  int mp = 0;
  while (mp < cap && ((bs >> mp) & 1) == 0) ++mp;
  while (mp > 0 && (bs >> mp) <= order) --mp;
  return mp;
}

// One block.  `lds` is lds_bytes(PCM) of 16-byte aligned workgroup memory.  PCM: the int32 form (above).
template <bool PCM>
#ifdef ASX_FLAC_HOST
static void encode_block(const Stream &P, int64_t blk, unsigned char *lds)
#else
static __device__ __forceinline__ void encode_block(const Stream &P, int64_t blk, unsigned char *lds)
#endif
{
  constexpr int NK = PCM ? NK_PCM : flac::NK;                 // parameters with exact bit counts
  constexpr int KSH = PCM ? 5 : 4;                            // the parameter's field under the bits in pk / pk1
  constexpr int PO_CAP = PCM ? MAX_PO_PCM : MAX_PO;
  constexpr int MY_IMG_WORDS = PCM ? IMG_WORDS : img_words(SIDE_BITS);
  constexpr long long RES_LIMIT = PCM ? 0x7fffffffll : (1ll << 30);   // |residual| below it, or the predictor is no candidate
  int32_t(*ch)[MAX_BLOCK] = reinterpret_cast<int32_t(*)[MAX_BLOCK]>(lds);
  double(*acp)[MAX_ORDER + 1] = reinterpret_cast<double(*)[MAX_ORDER + 1]>(lds + OFF_UNION);
  unsigned long long *sums = reinterpret_cast<unsigned long long *>(lds + OFF_UNION);   // [4][F][NK]
  uint32_t(*res)[MAX_BLOCK] = reinterpret_cast<uint32_t(*)[MAX_BLOCK]>(lds + OFF_UNION);
  uint32_t *img = reinterpret_cast<uint32_t *>(lds + OFF_IMG);
  Small &S = *reinterpret_cast<Small *>(lds + off_small(PCM));

  const int64_t first = blk * (int64_t)P.block_size;
  const int bs = (int)((P.n - first) < (int64_t)P.block_size ? (P.n - first) : (int64_t)P.block_size);
  const int chunk = (bs + NT - 1) / NT;
  const bool wide = !PCM && P.bps == 24;                      // the shifted stream of the int16 form
  const long long clk_begin = FLAC_CLOCK(P);

  // ---- load the four candidate channels, clear the image
  FLAC_LANES {
    for (int i = tid; i < bs; i += NT) {
      int32_t l, r;
      if (PCM) {
        l = P.pcm[2 * (first + i)];
        r = P.pcm[2 * (first + i) + 1];
      } else {
        const int32_t v = P.pcm[first + i];
        l = (int32_t)(int16_t)(v & 0xffff), r = v >> 16;
      }
      ch[0][i] = l;
      ch[1][i] = r;
      ch[2][i] = wide ? l + r : (l + r) >> 1;
      ch[3][i] = l - r;
    }
    for (int w = tid; w < MY_IMG_WORDS; w += NT) img[w] = 0u;
    if (tid < 4) {
      S.noteq[tid] = 0;
      S.sub_bps[tid] = PCM ? P.bps + (tid == 3 ? 1 : 0) : (tid == 3 || (tid == 2 && wide)) ? 17 : 16;
      S.hdr_bits[tid] = 8 + (wide ? (tid == 2 ? 7 : 8) : 0);
      for (int p = 0; p < NPRED; ++p) {
        S.valid[tid][p] = p < 5 ? 1 : 0;
        S.shift[tid][p] = 0;
        for (int j = 0; j < MAX_ORDER; ++j) S.coef[tid][p][j] = 0;
      }
      S.coef[tid][1][0] = 1;
      S.coef[tid][2][0] = 2, S.coef[tid][2][1] = -1;
      S.coef[tid][3][0] = 3, S.coef[tid][3][1] = -3, S.coef[tid][3][2] = 1;
      S.coef[tid][4][0] = 4, S.coef[tid][4][1] = -6, S.coef[tid][4][2] = 4, S.coef[tid][4][3] = -1;
    }
  }
  FLAC_SYNC();

  // ---- constant channels
  FLAC_LANES {
    for (int c = 0; c < 4; ++c) {
      bool ne = false;
      for (int i = tid; i < bs; i += NT) ne = ne || ch[c][i] != ch[c][0];
      if (ne) S.noteq[c] = 1;
    }
  }
  FLAC_SYNC();

  // ---- windowed autocorrelation, lags 0..8: per-lane partial sums, then a sum over the lanes in lane order (deterministic)
  for (int c = 0; c < 4; ++c) {
    FLAC_LANES {
      double a[MAX_ORDER + 1];
      for (int l = 0; l <= MAX_ORDER; ++l) a[l] = 0.0;
      const int i0 = tid * chunk, i1 = (i0 + chunk) < bs ? (i0 + chunk) : bs;
      for (int i = i0; i < i1; ++i) {
        const double xi = welch(i, bs) * (double)ch[c][i];
        for (int l = 0; l <= MAX_ORDER && l <= i; ++l) a[l] += xi * (welch(i - l, bs) * (double)ch[c][i - l]);
      }
      for (int l = 0; l <= MAX_ORDER; ++l) acp[tid][l] = a[l];
    }
    FLAC_SYNC();
    FLAC_LANES {                                // runs of 16 lanes, in place: a work item only touches its own run and lag
      if (tid < (NT / 16) * (MAX_ORDER + 1)) {
        const int l = tid % (MAX_ORDER + 1), g = tid / (MAX_ORDER + 1);
        double s = 0.0;
        for (int t = 0; t < 16; ++t) s += acp[g * 16 + t][l];
        acp[g * 16][l] = s;
      }
    }
    FLAC_SYNC();
    FLAC_LANES {
      if (tid <= MAX_ORDER) {
        double s = 0.0;
        for (int g = 0; g < NT / 16; ++g) s += acp[g * 16][tid];
        S.ac[c][tid] = s;
      }
    }
    FLAC_SYNC();
  }

  // ---- Levinson-Durbin and quantisation, one lane per channel; the first verdict per channel (constant or verbatim)
  FLAC_LANES {
    if (tid < 4) {
      const int c = tid;
      double a[MAX_ORDER], t[MAX_ORDER];
      double err = S.ac[c][0];
      for (int i = 0; i < MAX_ORDER && err > 0.0; ++i) {
        double acc = S.ac[c][i + 1];
        for (int j = 0; j < i; ++j) acc -= a[j] * S.ac[c][i - j];
        const double k = acc / err;
        for (int j = 0; j < i; ++j) t[j] = a[j] - k * a[i - 1 - j];
        for (int j = 0; j < i; ++j) a[j] = t[j];
        a[i] = k;
        err *= 1.0 - k * k;
        double cmax = 0.0;
        bool finite = true;
        for (int j = 0; j <= i; ++j) {
          const double m = fabs(a[j]);
          finite = finite && m < 1e30;          // false for NaN too
          cmax = m > cmax ? m : cmax;
        }
        if (!finite) break;
        if (cmax <= 0.0) continue;
        int e2 = 0;
        (void)frexp(cmax, &e2);                 // cmax = m * 2^e2, 0.5 <= m < 1
        int sh = QLP_BITS - 1 - e2;
        if (sh > 15) sh = 15;
        if (sh < 0) continue;
        const int p = 5 + i;
        const double scale = (double)(1 << sh);
        double carry = 0.0;
        for (int j = 0; j <= i; ++j) {
          carry += a[j] * scale;
          double q = floor(carry + 0.5);
          if (q > 16383.0) q = 16383.0;
          if (q < -16384.0) q = -16384.0;
          S.coef[c][p][j] = (int32_t)q;
          carry -= q;
        }
        S.shift[c][p] = sh;
        S.valid[c][p] = 1;
      }
      if (S.noteq[c]) {
        S.best_type[c] = 1;
        S.best_bits[c] = (unsigned long long)S.hdr_bits[c] + (unsigned long long)S.sub_bps[c] * (unsigned long long)bs;
      } else {
        S.best_type[c] = 0;
        S.best_bits[c] = (unsigned long long)(S.hdr_bits[c] + S.sub_bps[c]);
      }
      S.best_pred[c] = 0;
      S.best_po[c] = 0;
      S.best_method[c] = 0;
    }
  }
  FLAC_SYNC();

  // ---- the predictor passes
  for (int p = 0; p < NPRED; ++p) {
    const int order = pred_order(p);
    if (order >= bs) continue;
    const int mp = max_partition_order(bs, order, PO_CAP);
    const int F = 1 << mp, plen = bs >> mp;
    FLAC_LANES {
      for (int q = tid; q < 4 * F * NK; q += NT) sums[q] = 0ull;
      for (int q = tid; q < 4 * 128; q += NT) {
        S.pk[q >> 7][q & 127] = ~0ull;
        if (PCM) S.pk1[q >> 7][q & 127] = ~0ull;
      }
      if (tid < 4) {
        S.bad[tid] = 0;
        for (int o = 0; o <= MAX_PO; ++o) {
          S.cost[tid][o] = 0ull;
          if (PCM) S.cost1[tid][o] = 0ull;
        }
      }
    }
    FLAC_SYNC();
    FLAC_LANES {
      int i0 = tid * chunk;
      const int i1 = (i0 + chunk) < bs ? (i0 + chunk) : bs;
      if (i0 < order) i0 = order;
      for (int c = 0; c < 4 && i0 < i1; ++c) {
        if (!S.valid[c][p]) continue;
        int32_t cf[MAX_ORDER];
        for (int j = 0; j < MAX_ORDER; ++j) cf[j] = S.coef[c][p][j];
        const int sh = S.shift[c][p];
        unsigned long long acc[NK];
        for (int k = 0; k < NK; ++k) acc[k] = 0ull;
        int part = i0 / plen;
        int next = (part + 1) * plen;
        bool bad = false;
        for (int i = i0; i < i1; ++i) {
          if (i == next) {
            for (int k = 0; k < NK; ++k) {
              FLAC_ADD64(&sums[(c * F + part) * NK + k], acc[k]);
              acc[k] = 0ull;
            }
            ++part;
            next += plen;
          }
          int64_t r = residual(ch[c], i, cf, order, sh);
          if (PCM ? (r >= RES_LIMIT || r <= -RES_LIMIT) : (r >= RES_LIMIT || r < -RES_LIMIT)) {
            bad = true;
            r = 0;
          }
          const uint32_t u = (uint32_t)(((uint64_t)r << 1) ^ (uint64_t)(r >> 63));
          for (int k = 0; k < NK; ++k) acc[k] += (unsigned long long)(u >> k);
        }
        for (int k = 0; k < NK; ++k) FLAC_ADD64(&sums[(c * F + part) * NK + k], acc[k]);
        if (bad) S.bad[c] = 1;
      }
    }
    FLAC_SYNC();
    // exact Rice bits of every partition of every admissible order: one work item per (channel, partition, parameter) sums the finest
    // partitions under it; the cheapest parameter of a partition is the minimum of (bits << 4 | k), so equal costs take the smaller k
    FLAC_LANES {
      const int per = 2 * F - 1;
      for (int q = tid; q < 4 * per * NK; q += NT) {
        const int k = q % NK, cq = q / NK;
        const int c = cq / per, qq = cq % per;
        int po = 0;
        while ((2 << po) - 1 <= qq) ++po;
        const int j = qq - ((1 << po) - 1);
        const int span = F >> po;
        unsigned long long bits = (unsigned long long)(k + 1) * (unsigned long long)((bs >> po) - (j == 0 ? order : 0));
        for (int f = 0; f < span; ++f) bits += sums[(c * F + j * span + f) * NK + k];
        if (!PCM || k < flac::NK) FLAC_MIN64(&S.pk[c][qq], (bits << KSH) | (unsigned long long)k);
        if (PCM) FLAC_MIN64(&S.pk1[c][qq], (bits << KSH) | (unsigned long long)k);
      }
    }
    FLAC_SYNC();
    FLAC_LANES {
      const int per = 2 * F - 1;
      for (int q = tid; q < 4 * per; q += NT) {
        const int c = q / per, qq = q % per;
        int po = 0;
        while ((2 << po) - 1 <= qq) ++po;
        const unsigned long long v = S.pk[c][qq];
        S.kb[c][qq] = (uint8_t)(v & ((1ull << KSH) - 1ull));
        FLAC_ADD64(&S.cost[c][po], (v >> KSH) + 4ull);
        if (PCM) {
          const unsigned long long v1 = S.pk1[c][qq];
          S.kb1[c][qq] = (uint8_t)(v1 & ((1ull << KSH) - 1ull));
          FLAC_ADD64(&S.cost1[c][po], (v1 >> KSH) + 5ull);
        }
      }
    }
    FLAC_SYNC();
    FLAC_LANES {
      if (tid < 4 && S.valid[tid][p] && !S.bad[tid]) {
        const int c = tid;
        int po = 0, method = 0;                  // equal costs: the lower order, and method 0 before method 1
        unsigned long long least = S.cost[c][0];
        for (int o = 0; o <= mp; ++o) {
          if (S.cost[c][o] < least) least = S.cost[c][o], po = o, method = 0;
          if (PCM && S.cost1[c][o] < least) least = S.cost1[c][o], po = o, method = 1;
        }
        const unsigned long long bits = (unsigned long long)(S.hdr_bits[c] + order * S.sub_bps[c] + (p >= 5 ? 4 + 5 + order * QLP_BITS : 0) + 2 + 4) +
                                        least;
        if (bits < S.best_bits[c]) {
          S.best_bits[c] = bits;
          S.best_type[c] = 2;
          S.best_pred[c] = p;
          S.best_po[c] = po;
          S.best_method[c] = method;
          for (int j = 0; j < (1 << po); ++j) S.best_k[c][j] = method ? S.kb1[c][(1 << po) - 1 + j] : S.kb[c][(1 << po) - 1 + j];
        }
      }
    }
    FLAC_SYNC();
  }

  // ---- stereo mode, frame header, subframe headers
  FLAC_LANES {
    if (tid == 0) {
      const unsigned long long m[4] = {S.best_bits[0] + S.best_bits[1], S.best_bits[0] + S.best_bits[3], S.best_bits[3] + S.best_bits[1],
                                       S.best_bits[2] + S.best_bits[3]};
      int mode = 0;
      for (int i = 1; i < 4; ++i)
        if (m[i] < m[mode]) mode = i;
      const int sel0[4] = {0, 0, 3, 2}, sel1[4] = {1, 3, 1, 3}, assign[4] = {1, 8, 9, 10};
      S.sel[0] = sel0[mode];
      S.sel[1] = sel1[mode];
      uint32_t hb[HEADER_MAX];
      int nh = 0;
      const int bcode = block_size_code(bs, bs == P.block_size);
      hb[nh++] = 0xffu;
      hb[nh++] = 0xf8u;
      hb[nh++] = (uint32_t)((bcode << 4) | P.sr_code);
      hb[nh++] = (uint32_t)((assign[mode] << 4) | ((P.bps == 24 ? 6 : 4) << 1));
      const uint32_t fn = (uint32_t)blk;
      if (fn < 0x80u) {
        hb[nh++] = fn;
      } else {
        int extra = fn < 0x800u ? 1 : fn < 0x10000u ? 2 : fn < 0x200000u ? 3 : fn < 0x4000000u ? 4 : 5;
        hb[nh++] = ((0xfeu << (6 - extra)) & 0xffu) | (fn >> (6 * extra));
        for (int i = extra - 1; i >= 0; --i) hb[nh++] = 0x80u | ((fn >> (6 * i)) & 0x3fu);
      }
      if (bcode == 6) hb[nh++] = (uint32_t)(bs - 1);
      if (bcode == 7) hb[nh++] = (uint32_t)((bs - 1) >> 8), hb[nh++] = (uint32_t)((bs - 1) & 255);
      if (P.sr_extra_bits == 16) hb[nh++] = (P.sr_extra >> 8) & 255u;
      if (P.sr_extra_bits >= 8) hb[nh++] = P.sr_extra & 255u;
      uint32_t crc = 0;
      for (int i = 0; i < nh; ++i) crc = crc8_byte(crc, hb[i]);
      hb[nh++] = crc;
      for (int i = 0; i < nh; ++i) put_bits(img, (uint32_t)(8 * i), 8, hb[i]);
      S.sub_start[0] = (uint32_t)(8 * nh);
      S.sub_start[1] = S.sub_start[0] + (uint32_t)S.best_bits[S.sel[0]];
      const uint32_t total = S.sub_start[1] + (uint32_t)S.best_bits[S.sel[1]];
      S.frame_len = (int32_t)((total + 7u) / 8u + 2u);
    }
  }
  FLAC_SYNC();
  FLAC_LANES {
    if (tid < 2) {
      const int c = S.sel[tid];
      const int type = S.best_type[c], p = S.best_pred[c], order = type == 2 ? pred_order(p) : 0;
      const int sb = S.sub_bps[c];
      uint32_t pos = S.sub_start[tid];
      const int code = type == 0 ? 0 : type == 1 ? 1 : p < 5 ? (8 | order) : (32 | (order - 1));
      put_bits(img, pos, 8, (uint32_t)((code << 1) | (wide ? 1 : 0)));
      pos += 8;
      if (wide) {
        const int wb = S.hdr_bits[c] - 8;         // wasted bits k as k - 1 zeros and a one
        put_bits(img, pos, wb, 1u);
        pos += (uint32_t)wb;
      }
      if (type == 0) put_bits(img, pos, sb, (uint32_t)ch[c][0]);
      if (type == 2) {
        for (int i = 0; i < order; ++i, pos += (uint32_t)sb) put_bits(img, pos, sb, (uint32_t)ch[c][i]);
        if (p >= 5) {
          put_bits(img, pos, 4, (uint32_t)(QLP_BITS - 1));
          put_bits(img, pos + 4, 5, (uint32_t)S.shift[c][p]);
          pos += 9;
          for (int j = 0; j < order; ++j, pos += QLP_BITS) put_bits(img, pos, QLP_BITS, (uint32_t)S.coef[c][p][j]);
        }
        put_bits(img, pos, 6, (uint32_t)((S.best_method[c] << 4) | S.best_po[c]));   // the method in two bits, then the partition order
        pos += 6;
      }
      S.res_start[tid] = pos;
    }
  }
  FLAC_SYNC();

  // ---- residuals of the two chosen channels and their code lengths per lane
  FLAC_LANES {
    for (int s = 0; s < 2; ++s) {
      const int c = S.sel[s];
      uint32_t total = 0;
      if (S.best_type[c] == 2) {
        const int p = S.best_pred[c], order = pred_order(p), sh = S.shift[c][p];
        const int plen = bs >> S.best_po[c];
        int32_t cf[MAX_ORDER];
        for (int j = 0; j < MAX_ORDER; ++j) cf[j] = S.coef[c][p][j];
        int i0 = tid * chunk;
        const int i1 = (i0 + chunk) < bs ? (i0 + chunk) : bs;
        if (i0 < order) i0 = order;
        for (int i = i0; i < i1; ++i) {
          const int64_t r = residual(ch[c], i, cf, order, sh);
          const uint32_t u = (uint32_t)(((uint64_t)r << 1) ^ (uint64_t)(r >> 63));
          const int k = S.best_k[c][i / plen];
          res[s][i] = u;
          total += (u >> k) + 1u + (uint32_t)k;
        }
      }
      S.csum[s][tid] = total;
    }
  }
  FLAC_SYNC();
  FLAC_LANES {
    if (tid < 2) {
      uint32_t run = 0;
      for (int t = 0; t < NT; ++t) {
        const uint32_t v = S.csum[tid][t];
        S.csum[tid][t] = run;
        run += v;
      }
    }
  }
  FLAC_SYNC();

  // ---- every lane deposits its codes
  FLAC_LANES {
    for (int s = 0; s < 2; ++s) {
      const int c = S.sel[s];
      const int sb = S.sub_bps[c];
      if (S.best_type[c] == 1) {
        const uint32_t base = S.sub_start[s] + (uint32_t)S.hdr_bits[c];
        for (int i = tid; i < bs; i += NT) put_bits(img, base + (uint32_t)i * (uint32_t)sb, sb, (uint32_t)ch[c][i]);
      } else if (S.best_type[c] == 2) {
        const int order = pred_order(S.best_pred[c]);
        const int plen = bs >> S.best_po[c];
        int i0 = tid * chunk;
        const int i1 = (i0 + chunk) < bs ? (i0 + chunk) : bs;
        if (i0 < order) i0 = order;
        if (i0 < i1) {
          int part = i0 / plen;
          const uint32_t pb = S.best_method[c] ? 5u : 4u;   // bits of a partition's parameter
          uint32_t pos = S.res_start[s] + S.csum[s][tid] + pb * (uint32_t)(part + 1);
          for (int i = i0; i < i1; ++i) {
            if (i == (part + 1) * plen) {
              ++part;
              pos += pb;
            }
            const int k = S.best_k[c][part];
            if (i == (part == 0 ? order : part * plen)) put_bits(img, pos - pb, (int)pb, (uint32_t)k);
            const uint32_t u = res[s][i];
            const uint32_t q = u >> k;
            put_bits(img, pos + q, k + 1, (1u << k) | (u & ((1u << k) - 1u)));
            pos += q + 1u + (uint32_t)k;
          }
        }
      }
    }
  }
  FLAC_SYNC();

  // ---- CRC-16 over everything before it
  const long long clk_crc = FLAC_CLOCK(P);
  const int nbytes = S.frame_len - 2;
  const int nchunks = (nbytes + CRC_CHUNK - 1) / CRC_CHUNK;
  FLAC_LANES {
    for (int j = tid; j < nchunks; j += NT) {
      const int b0 = j * CRC_CHUNK, b1 = (b0 + CRC_CHUNK) < nbytes ? (b0 + CRC_CHUNK) : nbytes;
      uint32_t crc = 0;
      for (int b = b0; b < b1; ++b) crc = crc16_byte(crc, img_byte(img, b));
      S.crcs[j] = crc;
    }
  }
  FLAC_SYNC();
  FLAC_LANES {
    if (tid == 0) {
      const uint32_t crc = crc16_combine(0u, S.crcs, nchunks, nbytes);
      put_bits(img, (uint32_t)nbytes * 8u, 16, crc);
      P.frame_bytes[blk] = S.frame_len;
    }
  }
  FLAC_SYNC();
  const long long clk_crc_end = FLAC_CLOCK(P);

  // ---- the frame, 16 bytes per store
  FLAC_LANES {
    uint8_t *slot = P.frames + blk * (int64_t)P.stride;
    const int n16 = (S.frame_len + 15) / 16;
    for (int q = tid; q < n16; q += NT) {
      uint32_t w[4];
      for (int i = 0; i < 4; ++i) {
        const uint32_t v = img[4 * q + i];
        w[i] = (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
      }
#ifdef ASX_FLAC_HOST
      memcpy(slot + 16 * q, w, 16);
#else
      *reinterpret_cast<uint4 *>(slot + 16 * q) = make_uint4(w[0], w[1], w[2], w[3]);
#endif
    }
  }
#ifndef ASX_FLAC_HOST
  if (P.cycles != nullptr && threadIdx.x == 0) {
    atomicAdd(&P.cycles[0], (unsigned long long)(clock64() - clk_begin));
    atomicAdd(&P.cycles[1], (unsigned long long)(clk_crc_end - clk_crc));
  }
#else
  (void)clk_begin, (void)clk_crc, (void)clk_crc_end;
#endif
}

#ifndef ASX_FLAC_HOST
template <bool PCM>
__global__ __launch_bounds__(NT) void flac_encode_kernel(Stream P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char flac_lds[];
  encode_block<PCM>(P, (int64_t)blockIdx.x, flac_lds);
}

// offsets[b] = sum of frame_bytes[0 .. b), offsets[nb] = the stream's audio bytes: one workgroup, a run of blocks per lane
constexpr int SCAN_THREADS = 1024;
__global__ __launch_bounds__(SCAN_THREADS) void flac_scan_kernel(const int32_t *__restrict__ frame_bytes, int64_t nb, int64_t *__restrict__ offsets) {
  __shared__ int64_t part[SCAN_THREADS];
  const int tid = (int)threadIdx.x;
  const int64_t per = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
  const int64_t b0 = (int64_t)tid * per < nb ? (int64_t)tid * per : nb, b1 = (b0 + per) < nb ? (b0 + per) : nb;
  int64_t s = 0;
  for (int64_t b = b0; b < b1; ++b) s += frame_bytes[b];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int64_t run = 0;
    for (int t = 0; t < SCAN_THREADS; ++t) {
      const int64_t v = part[t];
      part[t] = run;
      run += v;
    }
    offsets[nb] = run;
  }
  __syncthreads();
  int64_t run = part[tid];
  for (int64_t b = b0; b < b1; ++b) {
    offsets[b] = run;
    run += frame_bytes[b];
  }
}

// frame b: frame_bytes[b] bytes from its slot to out + offsets[b]
constexpr int COMPACT_THREADS = 256;
__global__ __launch_bounds__(COMPACT_THREADS) void flac_compact_kernel(const uint8_t *__restrict__ frames, int stride, const int32_t *__restrict__ frame_bytes,
                                                                        const int64_t *__restrict__ offsets, uint8_t *__restrict__ out) {
  const int64_t b = (int64_t)blockIdx.x;
  const uint8_t *src = frames + b * (int64_t)stride;
  uint8_t *dst = out + offsets[b];
  const int n = frame_bytes[b];
  // destination words where both ends allow, bytes at the edges
  const int head = (int)((4 - ((uintptr_t)dst & 3)) & 3) < n ? (int)((4 - ((uintptr_t)dst & 3)) & 3) : n;
  const int words = (n - head) / 4;
  for (int i = (int)threadIdx.x; i < head; i += COMPACT_THREADS) dst[i] = src[i];
  for (int w = (int)threadIdx.x; w < words; w += COMPACT_THREADS) {
    const uint8_t *s = src + head + 4 * w;
    *reinterpret_cast<uint32_t *>(dst + head + 4 * w) = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
  }
  for (int i = head + 4 * words + (int)threadIdx.x; i < n; i += COMPACT_THREADS) dst[i] = src[i];
}
#endif

}  // namespace flac
}  // namespace asx
