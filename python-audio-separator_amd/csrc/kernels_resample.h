// The rational polyphase converter of asx_resample_rational for gfx950 (the definition, the filter design and the table layout are in
// resample_plan.h): planar x [channels, n_in] -> y [channels, n_out], y[m] = sum_t tab[t][m mod L] * x[floor(m M / L) + P - t].
//
// One launch per call, grid (tiles, channels).  A workgroup owns the J * K consecutive outputs from tile * J * K (J a multiple of L) and
// stages their whole input span -- (J / L) K M + T floats, zero outside [0, n_in) -- in LDS once.  A thread takes one j in [0, J) per pass
// and walks the K outputs m = first + j + k J: (m mod L) is the same for all of them and the input base moves by (J / L) M per step, so
// every coefficient, loaded once from the table in L2 (consecutive lanes read consecutive floats of row t), feeds K FMAs whose inputs come
// from LDS.  For every k the lanes of a pass write consecutive outputs.  Lanes run along m, never along k: the LDS addresses of a wave then
// advance by M / L per lane (about 1.09 floats for 48 kHz -> 44.1 kHz: at most two lanes per bank; upsampling: broadcasts), where lanes along
// k would be M floats apart.  Tables of a few phases (L = 1, 2, 4: every lane of a wave wants the same one or two coefficients) are copied
// to LDS first and read from there (TAPS_LDS).
//
// The T products of an output are summed from both ends of the filter towards its centre in two float32 FMA chains, joined with the centre
// tap at the end: the partial sums stay as small as the tails of the filter until the last steps, which keeps the rounding of a 200 .. 800
// term sum near that of its few large terms.  The order is fixed, so a result does not depend on the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asx {

constexpr int RS_THREADS = 256;   // RESAMPLE_THREADS of resample_plan.h

// the outputs of one tile from its staged span: xs[u] = x[i0 + u] (0 outside the input), cs the table in LDS when TAPS_LDS
// COMP (the complement form, below): r goes to yc when that is not null, and cc[m] = fl(fl(ms mixc[m]) - fl(ss r))
template <int K, bool TAPS_LDS, bool COMP = false>
__device__ __forceinline__ void rs_tile_outputs(const float *xs, const float *cs, const float *__restrict__ tab, int L, int M, int P, int J, int64_t first,
                                                float *__restrict__ yc, int64_t n_out, const float *__restrict__ mixc = nullptr,
                                                float *__restrict__ cc = nullptr, float ms = 1.f, float ss = 1.f) {
  const int tid = (int)threadIdx.x;
  const int step = J / L * M;   // the input base of period k + 1 over that of period k
  for (int j = tid; j < J; j += RS_THREADS) {
    const int64_t m = first + j;
    if (m >= n_out) break;
    const float *c = (TAPS_LDS ? cs : tab) + j % L;
    const float *xb = xs + (int)(((int64_t)j * M) / L);   // tap t of period k reads xb[2 P - t + k step]
    float lo[K], hi[K];
#pragma unroll
    for (int k = 0; k < K; ++k) lo[k] = hi[k] = 0.f;
    for (int s = 0; s < P; ++s) {
      const float c_lo = c[(int64_t)s * L], c_hi = c[(int64_t)(2 * P - s) * L];
      const float *x_lo = xb + (2 * P - s), *x_hi = xb + s;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        lo[k] = fmaf(c_lo, x_lo[k * step], lo[k]);
        hi[k] = fmaf(c_hi, x_hi[k * step], hi[k]);
      }
    }
    const float c_mid = c[(int64_t)P * L];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int64_t mk = m + (int64_t)k * J;
      if (mk >= n_out) continue;
      const float r = fmaf(c_mid, xb[P + k * step], lo[k] + hi[k]);
      if (COMP) {
        const float w = mixc[mk];   // (the lanes of a pass: consecutive mk, like the stores)
        if (yc) yc[mk] = r;
        cc[mk] = __fsub_rn(__fmul_rn(ms, w), __fmul_rn(ss, r));   // two roundings and a third: hipcc would contract a*b - c*d
      } else {
        yc[mk] = r;
      }
    }
  }
}

template <int K, bool TAPS_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_rational_kernel(const float *__restrict__ x, int64_t n_in, const float *__restrict__ tab,
                                                                        int L, int M, int P, int J, int span, float *__restrict__ y,
                                                                        int64_t n_out) {
  extern __shared__ float rs_lds[];
  float *xs = rs_lds;          // [span]: x[q0 - P + u]
  float *cs = rs_lds + span;   // TAPS_LDS: the table [2 P + 1][L]
  const int tid = (int)threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * J * K;   // a multiple of L
  const int64_t i0 = first / L * M - P;                // the input sample behind xs[0]
  const float *xc = x + (int64_t)blockIdx.y * n_in;
  for (int u = tid; u < span; u += RS_THREADS) {
    const int64_t i = i0 + u;
    xs[u] = (i >= 0 && i < n_in) ? xc[i] : 0.f;
  }
  if (TAPS_LDS)
    for (int u = tid; u < (2 * P + 1) * L; u += RS_THREADS) cs[u] = tab[u];
  __syncthreads();
  rs_tile_outputs<K, TAPS_LDS>(xs, cs, tab, L, M, P, J, first, y + (int64_t)blockIdx.y * n_out, n_out);
}

// The writer-side form (asx_resample_rational_stem): the same tile, taps and FMA chains, so y[c][m] carries the bits of the kernel above wherever both
// compute it, with two freedoms.  ROWS: x is [n_in, channels] (the MDX stem layout) and channel blockIdx.y is staged with a stride of `channels`
// floats -- for stereo the two workgroups of a tile read the same lines, one from HBM and one from L2; the staging is span loads against
// T J K LDS reads and FMAs of the tile, which is why the channels are not folded into one workgroup (that would double the span in LDS, past
// 64 KiB for 44.1 -> 32 kHz, to save under 1 % of the tile's work).  n_out is the caller's: the grid covers it, and a tile whose span starts at or
// past n_in -- the filter has left the input -- stores zeros without staging or reading anything.
//
// COMP, the complement form (asx_resample_rational_complement): with r the output above, the epilogue also loads the file-rate mix
// mix[ch mix_stride + m] and stores c[ch][m] = fl(fl(mix_scale mix) - fl(stem_scale r)) -- three float32 roundings, no FMA -- beside r
// (y may be null: only c is stored).  No LDS and no barrier of its own; a tile past the input stores c = fl(mix_scale mix) - fl(stem_scale 0).
template <int K, bool TAPS_LDS, bool ROWS, bool COMP = false>
__global__ __launch_bounds__(RS_THREADS) void resample_rational_stem_kernel(const float *__restrict__ x, int channels, int64_t n_in,
                                                                             const float *__restrict__ tab, int L, int M, int P, int J, int span,
                                                                             float *__restrict__ y, int64_t n_out,
                                                                             const float *__restrict__ mix = nullptr, int64_t mix_stride = 0,
                                                                             float mix_scale = 1.f, float stem_scale = 1.f,
                                                                             float *__restrict__ c = nullptr) {
  extern __shared__ float rs_lds[];
  float *xs = rs_lds;          // [span]: x[i0 + u]
  float *cs = rs_lds + span;   // TAPS_LDS: the table [2 P + 1][L]
  const int tid = (int)threadIdx.x;
  const int64_t first = (int64_t)blockIdx.x * J * K;   // a multiple of L
  const int64_t i0 = first / L * M - P;                // the input sample behind xs[0]
  float *yc = (COMP && !y) ? nullptr : y + (int64_t)blockIdx.y * n_out;
  const float *mixc = COMP ? mix + (int64_t)blockIdx.y * mix_stride : nullptr;
  float *cc = COMP ? c + (int64_t)blockIdx.y * n_out : nullptr;
  if (i0 >= n_in) {   // (the same for every thread of the workgroup)
    const int64_t end = first + (int64_t)J * K < n_out ? first + (int64_t)J * K : n_out;
    for (int64_t m = first + tid; m < end; m += RS_THREADS) {
      if (!COMP || yc) yc[m] = 0.f;
      if (COMP) cc[m] = __fsub_rn(__fmul_rn(mix_scale, mixc[m]), __fmul_rn(stem_scale, 0.f));
    }
    return;
  }
  const float *xc = ROWS ? x + blockIdx.y : x + (int64_t)blockIdx.y * n_in;
  const int64_t stride = ROWS ? channels : 1;
  for (int u = tid; u < span; u += RS_THREADS) {
    const int64_t i = i0 + u;
    xs[u] = (i >= 0 && i < n_in) ? xc[i * stride] : 0.f;
  }
  if (TAPS_LDS)
    for (int u = tid; u < (2 * P + 1) * L; u += RS_THREADS) cs[u] = tab[u];
  __syncthreads();
  rs_tile_outputs<K, TAPS_LDS, COMP>(xs, cs, tab, L, M, P, J, first, yc, n_out, mixc, cc, mix_scale, stem_scale);
}

}  // namespace asx
