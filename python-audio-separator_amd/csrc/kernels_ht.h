// Demucs v4 (HTDemucs) kernels for gfx950 (uvr_lib_v5/demucs/htdemucs.py, hdemucs.py, demucs.py,
// transformer.py, spec.py).
//
// Every activation is CHANNELS-LAST: the spectrogram branch is [B, T, F, C] (time frames outer,
// frequency rows inner -- which is also the `b (t1 fr) c` token order of the cross transformer,
// transformer.py:524), the waveform branch is [B, 1, L, C].  In that layout every convolution of the
// network is a row GEMM whose A rows are GATHERED from KO x KI taps of C contiguous floats:
//   Conv2d (8,1)/(4,1)  and Conv1d 8/4          : taps along the inner axis, stride 4
//   ConvTranspose 8/4                           : two taps (j-1, j) -> 4*Cout columns scattered to 4 positions
//   3x3 / k3 rewrite, DConv dilated k3, 1x1     : taps along inner and/or outer axis
// (gg_kernel).  The A tile is fetched by LDS-DMA exactly like tdf_dma_kernel (kernels_net.h); only the
// source address of each 16-byte chunk differs.
#pragma once
#include "kernels_gemm3.h"   // split3_pair / split3_oct, bf16x8, ASX_MFMA_BF16 (the bf16 x 6 attention kernels)
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asx {

// sigmoid on the hardware exp / rcp units (2 ulp each; the GLU gates sit far inside the 1e-4 parity bar)
__device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }

enum { GG_DENSE = 0, GG_GLU = 1, GG_CONVT = 2, GG_STATS = 3, GG_GNGLU = 4 };

struct GgArgs {
  const float *x, *w, *bias, *res, *zeros;
  float *y;
  int64_t M;                    // rows = (B*O) * IR
  int N, K;                     // K = KO*KI*Cin; w is [N, K] dense
  int O, I, Cin, ldc;           // input [B, O, I, ldc], Cin (% 4 == 0) channels used
  int KO, KI, DO, DI, PO, PI, SI;
  int SO, OR;                   // outer-axis stride and output rows on the outer axis (OR = O when SO = 1)
  int64_t x_bs, y_bs;           // floats between batch items of x / y (views into larger tensors)
  int IR;                       // rows per (b, o) line
  float inv_cin;
  int mode, act;
  int Iout, Cout, crop, So;     // GG_CONVT: column (r, co) of row j -> position So*j - crop + r, r < N/Cout
  int64_t ldy, ldr;
  int res_mod;                  // > 0: residual row = row % res_mod (frequency embedding table)
  // GroupNorm(1, N) fusion (DConv, demucs.py:146-157): group of a row = (row / g_outer) * g_mod + row % g_mod
  float2 *row_stat;             // GG_DENSE / GG_STATS: [N tiles][M] (sum, sum of squares) of each row's act-less outputs; may be null
  const float2 *stat_in;        // GG_GNGLU: (mean, rstd) per group (rowstat_reduce_kernel)
  int64_t g_outer;
  int g_mod;
  const float *gamma, *beta, *ls;   // GG_GNGLU: GroupNorm affine (row order of w) and the LayerScale of the GLU outputs
  int lowai;                    // != 0: HBM-bound launch (ht_gg): prefer the small-tile variants
  int glu_rows;                 // != 0: w's rows are in GLU order (ht_glu_perm) -- GG_GLU / GG_GNGLU and the GG_STATS pass of the same GEMM
};

// Wave layout: MS = false -- the four waves split the N tile (wave w owns columns [16*NREP*w, +16*NREP) of all BM = 16*MREP
// rows): wide outputs.  MS = true -- the waves split the rows (wave w owns rows [16*MREP*w, +16*MREP) of all BN = 16*NREP
// columns; BM = 64*MREP): narrow outputs (N = 8 .. 96) without padding N up to a multiple of 64.
template <int NREP, int MREP, bool MS = false>
__global__ __launch_bounds__(256, 2) void gg_kernel(GgArgs a) {
  constexpr int BK = 32, CPR = 8, RPI = 8;
  constexpr int BM = MS ? 64 * MREP : 16 * MREP, BN = MS ? 16 * NREP : 64 * NREP, BUF = (BM + BN) * BK;
  constexpr int MG = MREP < 4 ? MREP : 4;   // activation fragments are loaded in groups of MG
  constexpr int NXI = BM / RPI, NWI = BN / RPI, NXL = (NXI + 3) / 4;
  extern __shared__ float lds_f[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;

  const int nbn = (a.N + BN - 1) / BN;
  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int bn = lid % nbn;
  const int64_t m0 = (int64_t)(lid / nbn) * BM;
  const int n0 = bn * BN;

  const int xrow0 = MS ? wave * 16 * MREP : 0;   // first tile row / column this wave owns
  const int wcol0 = MS ? 0 : wave * 16 * NREP;

  const int lr = lane / CPR, lp = lane % CPR;
  // swizzle g(row) = (row >> 1) & 7 with row = q*8 + lr, q = wave + 4i: depends on (wave & 1, lr) only
  const int cl = lp ^ ((((wave & 1) << 2) + (lr >> 1)) & 7);   // logical chunk this lane fetches

  // row -> (batch b, outer row oo, inner position j): one 64-bit division per lane, then incremental carries
  // (64-bit divisions cost thousands of cycles per lane -- they dominated the small-K, memory-bound launches)
  auto split = [&](int64_t row, int64_t &b, int &oo, int &j) {
    const int64_t bo = row / a.IR;
    j = (int)(row - bo * a.IR);
    b = bo / a.OR;
    oo = (int)(bo - b * a.OR);
  };
  auto advance = [&](int step, int64_t &b, int &oo, int &j) {
    j += step;
    while (j >= a.IR) {
      j -= a.IR;
      if (++oo >= a.OR) {
        oo = 0;
        ++b;
      }
    }
  };
  int64_t xb[NXL];
  int xo[NXL], xi[NXL];
  {
    int64_t b;
    int oo, j;
    split(m0 + wave * RPI + lr, b, oo, j);
#pragma unroll
    for (int i = 0; i < NXL; ++i) {
      const int q = wave + 4 * i;
      const int64_t row = m0 + q * RPI + lr;
      if (q < NXI && row < a.M) {
        xb[i] = b * a.x_bs;
        xo[i] = oo * a.SO - a.PO;
        xi[i] = j * a.SI - a.PI;
      } else {
        xb[i] = 0;
        xo[i] = -(1 << 29);
        xi[i] = 0;
      }
      advance(4 * RPI, b, oo, j);
    }
  }

  auto issue = [&](int k0, int buf) {
    float *xs = lds_f + buf * BUF;
    float *ws = xs + BM * BK;
    const int k = k0 + cl * 4;
    const int tap = (int)(((float)k + 0.5f) * a.inv_cin);
    const int ci = k - tap * a.Cin;
    const int to = (tap >= a.KI) + (tap >= 2 * a.KI);
    const int ti = tap - to * a.KI;
    const int od = to * a.DO, id = ti * a.DI;
    const bool kok = k < a.K;
#pragma unroll
    for (int i = 0; i < NXL; ++i) {
      const int q = wave + 4 * i;
      if (q < NXI) {
        const int o = xo[i] + od, ii = xi[i] + id;
        const bool ok = kok && ((unsigned)o < (unsigned)a.O) && ((unsigned)ii < (unsigned)a.I);
        const float *src = ok ? a.x + xb[i] + ((int64_t)o * a.I + ii) * a.ldc + ci : a.zeros;
        ASX_GLDS16(src, xs + q * 256);
      }
    }
#pragma unroll
    for (int i = 0; i < (NWI + 3) / 4; ++i) {
      const int q = wave + 4 * i;
      if (q < NWI) {
        const int row = q * RPI + lr;
        const bool ok = (n0 + row < a.N) && kok;
        const float *src = ok ? a.w + (int64_t)(n0 + row) * a.K + k : a.zeros;
        ASX_GLDS16(src, ws + q * 256);
      }
    }
  };

  f32x4 acc[NREP][MREP];
#pragma unroll
  for (int n = 0; n < NREP; ++n)
#pragma unroll
    for (int m = 0; m < MREP; ++m) acc[n][m] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (a.K + BK - 1) / BK;
  const int sw = (li >> 1) & 7;
  issue(0, 0);
  for (int ks = 0; ks < nk; ++ks) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (ks + 1 < nk) issue((ks + 1) * BK, (ks + 1) & 1);
    const float *xs = lds_f + (ks & 1) * BUF;
    const float *ws = xs + BM * BK;
#pragma unroll
    for (int kk = 0; kk < BK / 16; ++kk) {
      if (ks * BK + kk * 16 >= a.K) break;   // the tail of the last stage is zero padding (K = 8 .. 48 for the DConv 1x1)
      const int pc = ((kk * 4 + lk) ^ sw) * 4;
      f32x4 wa[NREP];
#pragma unroll
      for (int n = 0; n < NREP; ++n)
        wa[n] = *reinterpret_cast<const f32x4 *>(&ws[(wcol0 + n * 16 + li) * BK + pc]);
#pragma unroll
      for (int mg = 0; mg < MREP; mg += MG) {
        f32x4 xf[MG];
#pragma unroll
        for (int m = 0; m < MG; ++m) xf[m] = *reinterpret_cast<const f32x4 *>(&xs[(xrow0 + (mg + m) * 16 + li) * BK + pc]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int n = 0; n < NREP; ++n)
#pragma unroll
            for (int m = 0; m < MG; ++m) acc[n][mg + m] = ASX_MFMA(wa[n][j], xf[m][j], acc[n][mg + m]);
      }
    }
  }

  // epilogue: lane (li, lk) holds 4 consecutive columns of row m*16 + li
  const bool want_stats = a.row_stat != nullptr;
  if (a.mode == GG_GNGLU) {
    // y[row, c] += ls[c] * glu(groupnorm(z))[c].  GLU row order (engine_ht.h: ht_glu_perm): fragment 2 j holds 16 values, fragment
    // 2 j + 1 their gates, so this lane owns FOUR consecutive output channels per fragment pair: 16-byte read-modify-write.
    // All loads are issued before the first store.
    constexpr int NP = NREP / 2;
    f32x4 old[MREP][NP > 0 ? NP : 1];
    float2 mr[MREP];
    int64_t gb = (m0 + xrow0 + li) / a.g_outer;
    int64_t gr = (m0 + xrow0 + li) - gb * a.g_outer;     // row inside the batch item
    int gm = (int)(gr % a.g_mod);
#pragma unroll
    for (int m = 0; m < MREP; ++m) {
      const int64_t row = m0 + xrow0 + m * 16 + li;
      mr[m] = make_float2(0.f, 1.f);
      if (row < a.M) mr[m] = a.stat_in[gb * a.g_mod + gm];
      gr += 16;
      gm += 16;
      while (gm >= a.g_mod) gm -= a.g_mod;
      if (gr >= a.g_outer) {
        gr -= a.g_outer;
        ++gb;
      }
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const int oc = ((n0 + wcol0 + j * 32) >> 1) + lk * 4;      // output channel of this lane's four values
        old[m][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (row < a.M && oc < a.Cout) old[m][j] = *reinterpret_cast<const f32x4 *>(a.y + row * a.ldy + oc);
      }
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int ca = n0 + wcol0 + j * 32 + lk * 4, cg = ca + 16;   // value / gate columns of the GEMM
      const int oc = ((n0 + wcol0 + j * 32) >> 1) + lk * 4;
      if (oc >= a.Cout) continue;
      const f32x4 bza = *reinterpret_cast<const f32x4 *>(a.bias + ca), bzg = *reinterpret_cast<const f32x4 *>(a.bias + cg);
      const f32x4 gaa = *reinterpret_cast<const f32x4 *>(a.gamma + ca), gag = *reinterpret_cast<const f32x4 *>(a.gamma + cg);
      const f32x4 bea = *reinterpret_cast<const f32x4 *>(a.beta + ca), beg = *reinterpret_cast<const f32x4 *>(a.beta + cg);
      const f32x4 l4 = *reinterpret_cast<const f32x4 *>(a.ls + oc);
#pragma unroll
      for (int m = 0; m < MREP; ++m) {
        const int64_t row = m0 + xrow0 + m * 16 + li;
        if (row >= a.M) continue;
        const f32x4 va = acc[2 * j][m] + bza, vg = acc[2 * j + 1][m] + bzg;
        const float gmn = mr[m].x, grs = mr[m].y;
        f32x4 o = old[m][j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float nv = (va[r] - gmn) * grs * gaa[r] + bea[r];
          const float ng = (vg[r] - gmn) * grs * gag[r] + beg[r];
          o[r] += l4[r] * (nv * fast_sigmoid(ng));
        }
        *reinterpret_cast<f32x4 *>(a.y + row * a.ldy + oc) = o;
      }
    }
    return;
  }
  float rs[MREP], rss[MREP];
  int64_t eb;
  int eoo, ej;
  split(m0 + xrow0 + li, eb, eoo, ej);
  int rmod = a.res_mod > 0 ? (int)((m0 + xrow0 + li) % a.res_mod) : 0;
#pragma unroll
  for (int m = 0; m < MREP; ++m) {
    rs[m] = 0.f;
    rss[m] = 0.f;
    const int64_t row = m0 + xrow0 + m * 16 + li;
    const int64_t rrow = a.res_mod > 0 ? rmod : row;
    const int64_t bo = eb * a.OR + eoo;
    const int j = ej;
    const int64_t yrow = eb * a.y_bs + ((int64_t)eoo * a.IR + ej) * a.ldy;   // DENSE / GLU destination row
    advance(16, eb, eoo, ej);
    if (a.res_mod > 0) {
      rmod += 16;
      while (rmod >= a.res_mod) rmod -= a.res_mod;
    }
    if (row >= a.M) continue;
#pragma unroll
    for (int n = 0; n < NREP; ++n) {
      const int col = n0 + wcol0 + n * 16 + lk * 4;
      if (col >= a.N) continue;
      f32x4 v = acc[n][m];
      if (a.bias != nullptr) v += *reinterpret_cast<const f32x4 *>(a.bias + col);
      if (want_stats) {
        rs[m] += (v.x + v.y) + (v.z + v.w);
        rss[m] += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
      }
      if (a.mode == GG_STATS) continue;
      if (a.mode == GG_GLU) {
        // fragment pairs (values, gates): four consecutive GLU outputs per lane, one 16-byte store (ht_glu_perm)
        if (n & 1) continue;                         // handled together with its value fragment
        const int oc = ((n0 + wcol0 + n * 16) >> 1) + lk * 4;
        if (oc >= a.Cout) continue;
        f32x4 g4 = acc[n + 1 < NREP ? n + 1 : n][m];
        if (a.bias != nullptr) g4 += *reinterpret_cast<const f32x4 *>(a.bias + col + 16);
        f32x4 o;
        o.x = v.x * fast_sigmoid(g4.x);
        o.y = v.y * fast_sigmoid(g4.y);
        o.z = v.z * fast_sigmoid(g4.z);
        o.w = v.w * fast_sigmoid(g4.w);
        if (a.res != nullptr) o += *reinterpret_cast<const f32x4 *>(a.res + rrow * a.ldr + oc);
        *reinterpret_cast<f32x4 *>(a.y + yrow + oc) = o;
      } else {
        f32x4 o;
        o.x = tdf_act(v.x, a.act);
        o.y = tdf_act(v.y, a.act);
        o.z = tdf_act(v.z, a.act);
        o.w = tdf_act(v.w, a.act);
        int64_t off, roff;
        if (a.mode == GG_CONVT) {
          const int r = col / a.Cout;
          const int co = col - r * a.Cout;
          const int pos = j * a.So - a.crop + r;
          if ((unsigned)pos >= (unsigned)a.Iout) continue;
          off = (bo * a.Iout + pos) * a.ldy + co;
          roff = (bo * a.Iout + pos) * a.ldr + co;
        } else {
          off = yrow + col;
          roff = rrow * a.ldr + col;
        }
        if (a.res != nullptr) o += *reinterpret_cast<const f32x4 *>(a.res + roff);
        *reinterpret_cast<f32x4 *>(a.y + off) = o;
      }
    }
  }
  if (want_stats) {
    // per-row sums: over the 4 column groups of a wave (lk), then (N-split layout) over the 4 waves through LDS; one
    // float2 per (N tile, row) goes to row_stat and rowstat_reduce_kernel folds rows into groups (no atomics, reproducible)
    if (MS) {
#pragma unroll
      for (int m = 0; m < MREP; ++m) {
        float s1 = rs[m], s2 = rss[m];
        s1 += __shfl_xor(s1, 16);
        s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        const int64_t row = m0 + xrow0 + m * 16 + li;
        if (lk == 0 && row < a.M) a.row_stat[(int64_t)bn * a.M + row] = make_float2(s1, s2);
      }
    } else {
      __syncthreads();   // the K loop's LDS tiles are dead
      float *sh = lds_f;                 // [4 waves][BM][2]
#pragma unroll
      for (int m = 0; m < MREP; ++m) {
        float s1 = rs[m], s2 = rss[m];
        s1 += __shfl_xor(s1, 16);
        s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 32);
        if (lk == 0) {
          sh[(wave * BM + m * 16 + li) * 2] = s1;
          sh[(wave * BM + m * 16 + li) * 2 + 1] = s2;
        }
      }
      __syncthreads();
      if (tid < BM && m0 + tid < a.M) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          s1 += sh[(w * BM + tid) * 2];
          s2 += sh[(w * BM + tid) * 2 + 1];
        }
        a.row_stat[(int64_t)bn * a.M + m0 + tid] = make_float2(s1, s2);
      }
    }
  }
}

// fold the per-row sums of gg_kernel into GroupNorm statistics: group g = (b, g2) owns rows b*g_outer + r*g_mod + g2,
// r < R, of every N tile.  acc[g] = (sum, sum of squares) in float64 (for gn_apply_kernel), mr[g] = (mean, rstd).
// g_mod > 1: grid = (ceil(G2 / 16), B), a workgroup folds 16 adjacent groups over 16 row slices;
// g_mod == 1: grid = (slices, B), the slices stride over the rows of the single group (ticket: one zeroed counter per item).
__global__ __launch_bounds__(256) void rowstat_reduce_kernel(const float2 *__restrict__ row_stat, int64_t M, int ntile,
                                                             int64_t g_outer, int g_mod, int64_t R, double count, float eps,
                                                             double *__restrict__ acc, float2 *__restrict__ mr,
                                                             unsigned *__restrict__ ticket) {
  const int64_t b = blockIdx.y;
  __shared__ double sh[16][16][2];
  const int lane = threadIdx.x & 63, sl = threadIdx.x >> 6;
  double s1 = 0.0, s2 = 0.0;
  if (g_mod > 1) {
    // 16 adjacent groups (128-byte row segments) x 16 row slices per workgroup: 4x the workgroups of a 64 x 4 split --
    // with 1895 frames per group (Demucs v3's 44 s chunks) the fold was 11 % of the forward at 32 workgroups
    const int gl = threadIdx.x & 15, rs = threadIdx.x >> 4;
    const int g2 = blockIdx.x * 16 + gl;
    if (g2 < g_mod)
      for (int t = 0; t < ntile; ++t) {
        const float2 *p = row_stat + (int64_t)t * M + b * g_outer + g2;
        for (int64_t r = rs; r < R; r += 16) {
          const float2 v = p[r * g_mod];
          s1 += (double)v.x;
          s2 += (double)v.y;
        }
      }
    sh[rs][gl][0] = s1;
    sh[rs][gl][1] = s2;
    __syncthreads();
    if (rs == 0 && g2 < g_mod) {
      s1 = 0.0;
      s2 = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        s1 += sh[i][gl][0];
        s2 += sh[i][gl][1];
      }
      const int64_t g = b * g_mod + g2;
      acc[g * 2] = s1;
      acc[g * 2 + 1] = s2;
      const double mu = s1 / count;
      double var = s2 / count - mu * mu;
      if (var < 0.0) var = 0.0;
      mr[g] = make_float2((float)mu, (float)(1.0 / sqrt(var + (double)eps)));
    }
    return;
  }
  // one group per item: gridDim.x workgroups share the rows; partial sums meet in acc (zeroed by the caller) through
  // float64 atomics and the last workgroup to arrive publishes (mean, rstd)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int t = 0; t < ntile; ++t) {
    const float2 *p = row_stat + (int64_t)t * M + b * g_outer;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += stride) {
      const float2 v = p[r];
      s1 += (double)v.x;
      s2 += (double)v.y;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_xor(s1, off);
    s2 += __shfl_xor(s2, off);
  }
  if (lane == 0) {
    sh[sl][0][0] = s1;
    sh[sl][0][1] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    s1 = (sh[0][0][0] + sh[1][0][0]) + (sh[2][0][0] + sh[3][0][0]);
    s2 = (sh[0][0][1] + sh[1][0][1]) + (sh[2][0][1] + sh[3][0][1]);
    if (gridDim.x > 1) {
      atomicAdd(&acc[b * 2], s1);
      atomicAdd(&acc[b * 2 + 1], s2);
      __threadfence();
      if (atomicAdd(&ticket[b], 1u) != gridDim.x - 1) return;
      __threadfence();
      s1 = atomicAdd(&acc[b * 2], 0.0);
      s2 = atomicAdd(&acc[b * 2 + 1], 0.0);
      ticket[b] = 0;
    } else {
      acc[b * 2] = s1;
      acc[b * 2 + 1] = s2;
    }
    const double mu = s1 / count;
    double var = s2 / count - mu * mu;
    if (var < 0.0) var = 0.0;
    mr[b] = make_float2((float)mu, (float)(1.0 / sqrt(var + (double)eps)));
  }
}

template <int NREP, int MREP, bool MS = false>
static void ht_launch_gg(const GgArgs &a, hipStream_t s) {
  constexpr int BM = MS ? 64 * MREP : 16 * MREP, BN = MS ? 16 * NREP : 64 * NREP;
  constexpr int lds = 2 * (BM + BN) * 32 * 4;
  grant_lds(&gg_kernel<NREP, MREP, MS>, lds);
  const int64_t nbm = (a.M + BM - 1) / BM;
  const int nbn = (a.N + BN - 1) / BN;
  // a single-stage K loop (K <= 32: the DConv 1x1 -> 2C GEMMs of the outer levels) only ever touches LDS buffer 0: ask for half
  // the LDS, so that four workgroups instead of two share a CU -- these launches are HBM-bound and want loads in flight
  const int lds_launch = a.K <= 32 ? lds / 2 : lds;
  hipLaunchKernelGGL((gg_kernel<NREP, MREP, MS>), dim3((unsigned)(nbm * nbn)), dim3(256), lds_launch, s, a);
}

// N tile width ht_gg_dispatch will use for an output of n columns (rowstat_reduce_kernel needs the tile count)
// glu: the launch runs a GLU epilogue (value / gate fragment pairs must sit in ONE wave: no 16- or 48-column tiles, and not
// the 64-column tile whose four waves own 16 columns each)
static inline int gg_tile_n(int n, bool glu = false) {
  if (knobs().gg_legacy && !glu) return n > 64 ? 128 : 64;
  if (glu) {
    if (n <= 32) return 32;
    if (n <= 64) return 32;
  }
  if (n <= 16) return 16;
  if (n <= 32) return 32;
  if (n <= 48) return 48;
  if (n <= 64) return 64;
  const int p96 = (n + 95) / 96 * 96, p128 = (n + 127) / 128 * 128;
  return p96 < p128 ? 96 : 128;
}

static void ht_gg_dispatch(const GgArgs &a, hipStream_t s) {
  // narrow outputs (N <= 48: DConv k3 -> C/8, small VR / encoder layers) are HBM-bound: 128-row tiles (37-45 KB of LDS, three to
  // four workgroups per CU) instead of 256-row tiles (70-78 KB, two) keep more loads in flight (ASX_GG_M128=0: the 256-row tiles)
  const bool m128 = knobs().gg_m128;
  switch (gg_tile_n(a.N, a.glu_rows != 0)) {
    case 16: m128 ? ht_launch_gg<1, 2, true>(a, s) : ht_launch_gg<1, 4, true>(a, s); break;
    case 32: m128 ? ht_launch_gg<2, 2, true>(a, s) : ht_launch_gg<2, 4, true>(a, s); break;
    case 48: m128 ? ht_launch_gg<3, 2, true>(a, s) : ht_launch_gg<3, 4, true>(a, s); break;
    // HBM-bound launches (a.lowai: algorithmic flop / byte under the threshold of ht_gg) take 64-row tiles: 41-49 KB of LDS, three
    // workgroups per CU instead of two -- loads in flight, not operand reuse, is what they lack
    case 64: a.lowai ? ht_launch_gg<1, 4>(a, s) : ht_launch_gg<1, 8>(a, s); break;
    case 96: a.lowai ? ht_launch_gg<6, 1, true>(a, s) : ht_launch_gg<6, 2, true>(a, s); break;
    default: a.lowai ? ht_launch_gg<2, 4>(a, s) : ht_launch_gg<2, 8>(a, s); break;
  }
}

// ---------------------------------------------------------------------------
// Multi-head softmax attention (torch.nn.MultiheadAttention, transformer.py:213,305), head dim
// DH = 16*DT (48 for htdemucs: 384 / 8).  q / k / v are separate row matrices (slices of the packed
// in_proj output), queries and keys may differ in count (cross attention).  Same register scheme as
// kernels_rof.h::attention_kernel: S^T = K Q^T, online softmax per query column, O^T += V^T P^T.
// grid = (ceil(nq / 64), heads, B).
// ---------------------------------------------------------------------------
struct MhaArgs {
  const float *q, *k, *v;
  float *out;
  int64_t ldq, ldk, ldv, ldo;
  int nq, nk;
  float scale;
  int exact;   // 1: libm expf in the softmax; 0: hardware exp
  // LocalState of Demucs v3 (demucs.py:197-221; nq == nk): decay logits [B*nq, ldd] (4 per head) give every query a
  // slope D = 1/4 * sum_f (f + 1) * sigmoid(logit_f); score -= |key - query| * D, and the diagonal is set to -100
  const float *decay;
  int64_t ldd;
  int nqt, heads;   // query tiles and heads: the 1-D grid is nqt * heads * batch workgroups
};

// DB (double-buffered key / value tiles, head dims up to 48): tile t + 1 is written into the other LDS buffer while tile t is
// consumed, so ONE workgroup barrier per key tile remains instead of two (the barriers between the three co-resident
// workgroups, not the fragment reads or the K / V stream, are what held this kernel at ~57 % of the MFMA peak -- kernels_rof.h);
// 52 KB of LDS at DH = 48 keeps three workgroups per CU, and the global loads run two tiles ahead.
// (the single-buffered build of head dims <= 48 is compiled for FOUR workgroups per CU: <= 128 registers, 26 KB of LDS)
template <int DT, bool DECAY = false, bool DB = false>
__global__ __launch_bounds__(256, (DT <= 3 && !DB) ? 4 : 1) void mha_kernel(MhaArgs a) {
  constexpr int DH = 16 * DT, QS = DH + 2, VS = DH + 4, C4 = DH / 4;
  constexpr int TILE = 64 * QS + 64 * VS;
  // Q is staged through a K tile's space (its fragments move to registers before that tile is written):
  // head dim 96 fits the 64 KB of static LDS
  __shared__ float lds[(DB ? 2 : 1) * TILE];
  float *Qs = DB ? lds + TILE : lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  // 1-D grid, XCD-aware: the query tiles of one (batch item, head) get consecutive logical ids, i.e. run on ONE XCD and share
  // its L2 copy of that head's K / V (1 MB at 2688 tokens).  With the (q tile, head, batch) grid the dispatcher dealt the
  // query tiles of a head round-robin over the eight XCDs and every L2 had to hold every head: 6.8x the algorithmic bytes
  // came from HBM (rocprofv3 FETCH_SIZE, profiles/r03_pmc_halo.txt).
  int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = lid % a.nqt;
  lid /= a.nqt;
  const int h = lid % a.heads, b = lid / a.heads;
  const int q0 = qt * 64;
  const float *qp = a.q + (int64_t)b * a.nq * a.ldq + h * DH;
  const float *kp = a.k + (int64_t)b * a.nk * a.ldk + h * DH;
  const float *vp = a.v + (int64_t)b * a.nk * a.ldv + h * DH;

  for (int e = tid; e < 64 * C4; e += 256) {
    const int r = e / C4, c4 = e - r * C4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (q0 + r < a.nq) v = *reinterpret_cast<const float4 *>(qp + (int64_t)(q0 + r) * a.ldq + c4 * 4);
    float *d = &Qs[r * QS + c4 * 4];
    d[0] = v.x;
    d[1] = v.y;
    d[2] = v.z;
    d[3] = v.w;
  }

  f32x4 acc_o[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc_o[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  const int nkt = (a.nk + 63) / 64;
  // K / V tiles are prefetched into registers one tile ahead (the global latency hides behind the MFMAs of the current
  // tile); the wave's Q fragments are loop invariant and live in registers
  constexpr int NLD = (64 * C4 + 255) / 256;
  float4 kreg[NLD], vreg[NLD];
  auto fetch = [&](int kt) {
    const int k0 = kt * 64;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + i * 256;
      const int r = e / C4, c4 = e - r * C4;
      kreg[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      vreg[i] = kreg[i];
      if (e < 64 * C4 && k0 + r < a.nk) {
        kreg[i] = *reinterpret_cast<const float4 *>(kp + (int64_t)(k0 + r) * a.ldk + c4 * 4);
        vreg[i] = *reinterpret_cast<const float4 *>(vp + (int64_t)(k0 + r) * a.ldv + c4 * 4);
      }
    }
  };
  auto stage = [&](int buf) {          // registers -> LDS tile `buf`
    float *Kb = lds + buf * TILE, *Vb = Kb + 64 * QS;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = tid + i * 256;
      if (e < 64 * C4) {
        const int r = e / C4, c4 = e - r * C4;
        float *dk = &Kb[r * QS + c4 * 4];
        dk[0] = kreg[i].x;
        dk[1] = kreg[i].y;
        dk[2] = kreg[i].z;
        dk[3] = kreg[i].w;
        *reinterpret_cast<float4 *>(&Vb[r * VS + c4 * 4]) = vreg[i];
      }
    }
  };
  fetch(0);
  __syncthreads();   // Q staged
  float bqr[DH / 4];
#pragma unroll
  for (int kk = 0; kk < DH / 4; ++kk) bqr[kk] = Qs[(wave * 16 + li) * QS + 4 * kk + lk];
  const int qi = q0 + wave * 16 + li;
  float slope = 0.f;
  if (DECAY && qi < a.nq) {
    const float *dr = a.decay + ((int64_t)b * a.nq + qi) * a.ldd + h * 4;
#pragma unroll
    for (int f = 0; f < 4; ++f) slope += (float)(f + 1) * (1.0f / (1.0f + expf(-dr[f])));
    slope *= 0.25f;
  }
  if (DB) {
    stage(0);                          // buffer 0 is untouched so far (Q sits in buffer 1)
    if (nkt > 1) fetch(1);
  }
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * 64;
    const float *Ks, *Vs;
    if (DB) {
      // tile kt is visible in buffer kt & 1; everyone has finished with buffer (kt + 1) & 1 (tile kt - 1, or the Q stage)
      __syncthreads();
      if (kt + 1 < nkt) {
        stage((kt + 1) & 1);
        if (kt + 2 < nkt) fetch(kt + 2);
      }
      Ks = lds + (kt & 1) * TILE;
      Vs = Ks + 64 * QS;
    } else {
      __syncthreads();   // previous tile fully consumed
      stage(0);
      __syncthreads();
      if (kt + 1 < nkt) fetch(kt + 1);
      Ks = lds;
      Vs = lds + 64 * QS;
    }

    f32x4 st[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) st[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < DH / 4; ++kk) {
      const float bq = bqr[kk];
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const float av = Ks[(mt * 16 + li) * QS + 4 * kk + lk];
        st[mt] = ASX_MFMA(av, bq, st[mt]);
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + mt * 16 + 4 * lk + r;
        float s = (key < a.nk) ? st[mt][r] * a.scale : -INFINITY;
        if (DECAY && key < a.nk) {
          const int d = key > qi ? key - qi : qi - key;
          s = d == 0 ? -100.0f : s - (float)d * slope;
        }
        st[mt][r] = s;
        mx = fmaxf(mx, s);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float corr = (m_run == -INFINITY) ? 0.f : (a.exact ? expf(m_run - m_new) : __expf(m_run - m_new));
    float psum = 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = (st[mt][r] == -INFINITY) ? 0.f : (a.exact ? expf(st[mt][r] - m_new) : __expf(st[mt][r] - m_new));
        st[mt][r] = p;
        psum += p;
      }
    }
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    l_run = l_run * corr + psum;
    m_run = m_new;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) acc_o[dt] *= corr;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pb = st[mt][r];
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const float av = Vs[(mt * 16 + 4 * lk + r) * VS + dt * 16 + li];
          acc_o[dt] = ASX_MFMA(av, pb, acc_o[dt]);
        }
      }
    }
  }

  const int q = q0 + wave * 16 + li;
  if (q < a.nq) {
    const float inv = 1.0f / l_run;
    float *op = a.out + ((int64_t)b * a.nq + q) * a.ldo + h * DH;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      f32x4 o = acc_o[dt];
      o *= inv;
      *reinterpret_cast<f32x4 *>(op + dt * 16 + 4 * lk) = o;
    }
  }
}

// ---------------------------------------------------------------------------
// LayerNorm over the channel axis of a row matrix (+ optional positional table added after the affine,
// transformer.py:528,536): y = (x - mean) * rsqrt(var + eps) * g + b (+ pos[row % pos_mod]).
// One wave per row.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layernorm_kernel(const float *__restrict__ x, int64_t lda, int C,
                                                        const float *__restrict__ g, const float *__restrict__ bta,
                                                        const float *__restrict__ pos, int64_t pos_mod,
                                                        float *__restrict__ y, int64_t ldy, int64_t M, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float *xp = x + row * lda;
  float s = 0.f;
  for (int i = lane; i < C; i += 64) s += xp[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  const float mean = s / (float)C;
  float ss = 0.f;
  for (int i = lane; i < C; i += 64) {
    const float d = xp[i] - mean;
    ss += d * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
  const float rstd = 1.0f / sqrtf(ss / (float)C + eps);
  float *yp = y + row * ldy;
  const float *pp = pos != nullptr ? pos + (row % pos_mod) * C : nullptr;
  for (int i = lane; i < C; i += 64) {
    float v = (xp[i] - mean) * rstd * g[i] + bta[i];
    if (pp != nullptr) v += pp[i];
    yp[i] = v;
  }
}

// ---------------------------------------------------------------------------
// Group statistics.  x is viewed as [G1, R, P] (P = contiguous plane of G2 groups x ld floats, of which
// the first Cn of every ld are data); group (g1, e / gdiv) accumulates sum and sum of squares in
// float64: acc[(g1*G2 + g2)*2 + {0,1}].  grid = (ceil(P/256) or 1, rsplit, G1).
//   GroupNorm(1, C) of DConv on the spectrogram branch: G1 = B, R = T, P = F*ld, gdiv = ld   (per (b, f))
//   GroupNorm(1, C) over a whole sample / the mean-std of htdemucs.py:511,518: P = row, gdiv >= P
// Two launches, no atomics, every sum in a fixed order, so that two runs give the same bits: gstats_kernel leaves the sums of
// workgroup (bx, by, g1) over its nslot <= 66 local groups in part[((g1 * rsplit + by) * gx + bx) * nslot + slot] (slot = the group's
// index minus the workgroup's first group), gstats_finish_kernel adds a group's partial sums over (by, bx) with one wave per group.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gstats_kernel(const float *__restrict__ x, int64_t R, int64_t P, int64_t gdiv,
                                                     int ld, int Cn, int nslot, double2 *__restrict__ part) {
  __shared__ double ts[256], tq[256];
  __shared__ int tg[256];
  const int tid = threadIdx.x;
  int64_t e;
  int rr = 0, rpb = 1;
  if (P >= 256) {
    e = (int64_t)blockIdx.x * 256 + tid;
  } else {
    rpb = (int)(256 / P);
    rr = tid / (int)P;
    e = tid - rr * (int)P;
    if (rr >= rpb) e = P;   // idle
  }
  const int64_t g1 = blockIdx.z;
  const int64_t rows_per = (R + gridDim.y - 1) / gridDim.y;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per;
  const int64_t r1 = (r0 + rows_per < R) ? r0 + rows_per : R;
  const int64_t gfirst = ((int64_t)blockIdx.x * 256) / gdiv;
  double s = 0.0, ss = 0.0;
  int lg = -1;
  if (e < P && (int)(e % ld) < Cn) {
    const float *xp = x + g1 * R * P + e;
    for (int64_t r = r0 + rr; r < r1; r += rpb) {
      const double v = (double)xp[r * P];
      s += v;
      ss += v * v;
    }
    lg = (int)(e / gdiv - (P >= 256 ? gfirst : 0));
  }
  ts[tid] = s;
  tq[tid] = ss;
  tg[tid] = lg;
  __syncthreads();
  if (tid < nslot) {           // the threads of local group tid, in thread order
    double a = 0.0, q = 0.0;
    for (int t = 0; t < 256; ++t)
      if (tg[t] == tid) {
        a += ts[t];
        q += tq[t];
      }
    const int64_t wg = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[wg * nslot + tid] = make_double2(a, q);
  }
}

// grid = (G2, G1), one wave each: lane l adds the group's partial sums l, l + 64, ... in (by, bx) order, then the lanes fold in a fixed tree
__global__ __launch_bounds__(64) void gstats_finish_kernel(const double2 *__restrict__ part, int64_t P, int64_t gdiv, int G2, int gx,
                                                           int rsplit, int nslot, double *__restrict__ acc) {
  const int64_t g2 = blockIdx.x, g1 = blockIdx.y;
  double a = 0.0, q = 0.0;
  const int64_t first = g2 * gdiv;                      // the group's plane elements [first, last]
  if (first < P) {
    const int64_t last = (first + gdiv < P ? first + gdiv : P) - 1;
    const int bx0 = P >= 256 ? (int)(first / 256) : 0, bx1 = P >= 256 ? (int)(last / 256) : 0;
    const int nb = bx1 - bx0 + 1;
    for (int k = threadIdx.x; k < rsplit * nb; k += 64) {
      const int by = k / nb, bx = bx0 + k % nb;
      const int64_t gfirst = P >= 256 ? ((int64_t)bx * 256) / gdiv : 0;
      const double2 v = part[(((int64_t)g1 * rsplit + by) * gx + bx) * nslot + (g2 - gfirst)];
      a += v.x;
      q += v.y;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_xor(a, off);
    q += __shfl_xor(q, off);
  }
  if (threadIdx.x == 0) {
    acc[(g1 * G2 + g2) * 2] = a;
    acc[(g1 * G2 + g2) * 2 + 1] = q;
  }
}

__device__ __forceinline__ void group_mean_rstd(const double *acc, int64_t g, double n, float eps, float &mean,
                                                float &rstd) {
  const double m = acc[g * 2] / n;
  double var = acc[g * 2 + 1] / n - m * m;
  if (var < 0.0) var = 0.0;
  mean = (float)m;
  rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// GroupNorm(1, Cn) apply over [G1, R, G2, ld] with the statistics of gstats_kernel.
//   mode 0: y = gelu(norm(x))                         in place on x       (DConv, demucs.py:150-157)
//   mode 1: dst[.., c] += ls[c] * glu(norm(x))[c]     x has 2*Ch channels (DConv + LayerScale, demucs.py:178)
//   mode 2: y = norm(x)                               in place            (MyGroupNorm norm_out, transformer.py:181)
__global__ __launch_bounds__(256) void gn_apply_kernel(float *__restrict__ x, int64_t R, int G2, int ld, int Cn,
                                                       const double *__restrict__ acc, const float *__restrict__ gam,
                                                       const float *__restrict__ bet, float eps, int mode,
                                                       float *__restrict__ dst, int dst_ld,
                                                       const float *__restrict__ ls, int64_t total) {
  const int Ce = (mode == 1) ? Cn / 2 : Cn;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;          // total = G1*R*G2*Ce
  const int c = (int)(idx % Ce);
  const int64_t pos = idx / Ce;       // (g1, r, g2)
  const int g2 = (int)(pos % G2);
  const int64_t g1 = pos / G2 / R;
  float mean, rstd;
  group_mean_rstd(acc, g1 * G2 + g2, (double)R * Cn, eps, mean, rstd);
  float *xp = x + pos * ld;
  if (mode == 1) {
    const float na = (xp[c] - mean) * rstd * gam[c] + bet[c];
    const float ng = (xp[c + Ce] - mean) * rstd * gam[c + Ce] + bet[c + Ce];
    dst[pos * dst_ld + c] += ls[c] * (na * (1.0f / (1.0f + expf(-ng))));
  } else {
    float v = (xp[c] - mean) * rstd * gam[c] + bet[c];
    if (mode == 0) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
    xp[c] = v;
  }
}

// x = (x - mean) / (1e-5 + std), std unbiased (htdemucs.py:511-513), in place over [G1, n] with per-g1 stats.
__device__ __forceinline__ void sample_mean_std(const double *acc, int64_t g, double n, float &mean, float &stdv) {
  const double m = acc[g * 2] / n;
  double var = (acc[g * 2 + 1] - n * m * m) / (n - 1.0);
  if (var < 0.0) var = 0.0;
  mean = (float)m;
  stdv = (float)sqrt(var);
}

__global__ __launch_bounds__(256) void std_norm_kernel(float *__restrict__ x, int64_t n, const double *__restrict__ acc) {
  const int64_t g = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float mean, stdv;
  sample_mean_std(acc, g, (double)n, mean, stdv);
  x[g * n + i] = (x[g * n + i] - mean) / (1e-5f + stdv);
}

// waveform branch input (htdemucs.py:516-519): seg [B, 2, L] -> xt [B, L, 2] = (seg - mean) / (1e-5 + std), channels
// last; the first encoder layer reads it as [B, L/2, 4] (pairs of samples) so that its taps are 16-byte chunks.
__global__ __launch_bounds__(256) void time_norm_kernel(const float *__restrict__ seg, int64_t L,
                                                        const double *__restrict__ acc, float *__restrict__ xt) {
  const int64_t b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  float mean, stdv;
  sample_mean_std(acc, b, (double)(2 * L), mean, stdv);
  const float d = 1e-5f + stdv;
  const float l = (seg[(b * 2) * L + i] - mean) / d, r = (seg[(b * 2 + 1) * L + i] - mean) / d;
  reinterpret_cast<float2 *>(xt)[b * L + i] = make_float2(l, r);
}

__global__ __launch_bounds__(256) void add_kernel(float *__restrict__ y, const float *__restrict__ a, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] += a[i];
}

// ---------------------------------------------------------------------------
// HTDemucs._spec (htdemucs.py:383-403) -> [B, T, F, 4] with channel = ch*2 + {re, im}.
// Frame t covers samples [t*hop - 3*hop/2, ... + n_fft) of the segment, reflected at both ends (pad1d reflect
// then the centre padding of torch.stft, which frames 2 .. 2+le never touch), window = periodic Hann,
// normalized=True (x n_fft^-0.5); the Nyquist bin is dropped.  grid = (T, 2, B).
// ---------------------------------------------------------------------------
// Inputs no longer than the right pad are first zero-extended by pad1d (hdemucs.py:21-34: el zeros on the left, up to
// Lv samples in all) and the reflection runs on that; el = 0, Lv = L otherwise.
__global__ __launch_bounds__(256) void ht_stft_kernel(const float *__restrict__ seg, int64_t L, int64_t el, int64_t Lv, int hop, int T,
                                                      float *__restrict__ spec, const float *__restrict__ window,
                                                      const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  float2 *bufA = lds;
  float2 *bufB = lds + p.nh;
  const int t = blockIdx.x, ch = blockIdx.y, b = blockIdx.z;
  const float *src = seg + ((int64_t)b * 2 + ch) * L;
  const int pad = hop / 2 * 3;
  float *fa = reinterpret_cast<float *>(bufA);
  for (int e = threadIdx.x; e < p.n_fft; e += blockDim.x) {
    int64_t q = (int64_t)t * hop + e - pad + el;
    if (q < 0) q = -q;
    if (q >= Lv) q = 2 * (Lv - 1) - q;
    q -= el;
    fa[e] = (q >= 0 && q < L) ? src[q] * window[e] : 0.f;
  }
  float2 *Z = fft_lds<-1>(bufA, bufB, p, tw);
  const int nh = p.nh;
  const float sc = 1.0f / sqrtf((float)p.n_fft);
  for (int k = threadIdx.x; k < nh; k += blockDim.x) {
    const float2 zk = Z[k];
    float2 zc = Z[k == 0 ? 0 : nh - k];
    zc.y = -zc.y;
    const float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
    const float2 D = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
    const float2 O = make_float2(D.y, -D.x);
    const float2 X = cadd(E, cmul(tw[k], O));
    reinterpret_cast<float2 *>(spec)[(((int64_t)b * T + t) * nh + k) * 2 + ch] = make_float2(X.x * sc, X.y * sc);
  }
}

// HTDemucs._ispec frames (htdemucs.py:405-413, 600-606): spectrum of (b, source s, channel c) = CaC output
// x[b, t, f, s*4 + c*2 + {re, im}] * std + mean (htdemucs.py:590), Nyquist = 0; windowed inverse frames
// [B, S*2, T, n_fft] scaled by sqrt(n_fft) (normalized=True).  grid = (T, S*2, B).
__global__ __launch_bounds__(256) void ht_istft_kernel(const float *__restrict__ x, int T, int CH,
                                                       const double *__restrict__ acc, double n_stat,
                                                       float *__restrict__ frames, const float *__restrict__ window,
                                                       const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  // the staged spectrum X[0 .. nh] lives in bufB's space (+ 1 element): it is dead once the merge loop has written bufA, and
  // fft_lds starts with a barrier before its first stage writes bufB -- 32 KB instead of 48 KB, five workgroups per CU
  float2 *bufA = lds;
  float2 *bufB = lds + p.nh;
  float2 *bufX = bufB;
  const int t = blockIdx.x, sc_ = blockIdx.y, b = blockIdx.z;
  const int nh = p.nh;
  float mean, stdv;
  sample_mean_std(acc, b, n_stat, mean, stdv);
  for (int k = threadIdx.x; k <= nh; k += blockDim.x) {
    float2 v = make_float2(0.f, 0.f);
    if (k < nh) {
      const float2 r = *reinterpret_cast<const float2 *>(x + (((int64_t)b * T + t) * nh + k) * CH + sc_ * 2);
      v = make_float2(r.x * stdv + mean, r.y * stdv + mean);
    }
    if (k == 0) v.y = 0.f;
    bufX[k] = v;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nh; k += blockDim.x) {
    const float2 xk = bufX[k];
    float2 xc = bufX[nh - k];
    xc.y = -xc.y;
    const float2 E = make_float2(0.5f * (xk.x + xc.x), 0.5f * (xk.y + xc.y));
    const float2 D = make_float2(0.5f * (xk.x - xc.x), 0.5f * (xk.y - xc.y));
    float2 w = tw[k];
    w.y = -w.y;
    const float2 O = cmul(w, D);
    bufA[k] = make_float2(E.x - O.y, E.y + O.x);
  }
  float2 *z = fft_lds<+1>(bufA, bufB, p, tw);
  const float scale = sqrtf((float)p.n_fft) / (float)nh;
  float2 *dst = reinterpret_cast<float2 *>(frames + (((int64_t)b * gridDim.y + sc_) * T + t) * p.n_fft);
  const float2 *w2 = reinterpret_cast<const float2 *>(window);
  for (int m = threadIdx.x; m < nh; m += blockDim.x) {
    const float2 v = z[m];
    const float2 w = w2[m];
    dst[m] = make_float2((v.x * scale) * w.x, (v.y * scale) * w.y);
  }
}

// Overlap-add of the frames (torch.istft with two zero frames either side, / window envelope, htdemucs.py:405-413)
// plus the waveform branch: out[b, s, c, n] = xt[b, n, s*2 + c] * stdt + meant + ispec (htdemucs.py:608-612).
// env_hop[r] = sum_i w^2[r + i*hop] (every output sample is covered by n_fft/hop real-or-zero frames).
__global__ __launch_bounds__(256) void ht_ola_kernel(const float *__restrict__ frames, const float *__restrict__ env_hop,
                                                     int n_fft, int hop, int T, int64_t L,
                                                     const float *__restrict__ xt, int xt_ld,
                                                     const double *__restrict__ acc_t, float *__restrict__ out) {
  const int b = blockIdx.z, sc_ = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= L) return;
  const int64_t m = n + hop / 2 * 3;           // offset inside the run of real frames
  int64_t t_hi = m / hop;
  int64_t t_lo = (m - n_fft + hop) / hop;
  if (m - n_fft + 1 <= 0) t_lo = 0;
  if (t_hi > T - 1) t_hi = T - 1;
  const float *fr = frames + ((int64_t)b * gridDim.y + sc_) * T * n_fft;
  float a = 0.f;
  for (int64_t t = t_lo; t <= t_hi; ++t) a += fr[t * n_fft + (m - t * hop)];
  const float y = a / env_hop[m % hop];
  float mean, stdv;
  sample_mean_std(acc_t, b, (double)(2 * L), mean, stdv);
  const float tv = xt[((int64_t)b * L + n) * xt_ld + sc_] * stdv + mean;
  out[((int64_t)b * gridDim.y + sc_) * L + n] = tv + y;
}

// ---------------------------------------------------------------------------
// apply_model (apply.py:124-260) around the model.
// gather: seg[b, ch, i] = song[ch, start[b] + i] standardised ((x - mean) / std, demucs_separator.py:171-173),
//         0 outside the song (TensorChunk.padded, apply.py:96-107).
// ---------------------------------------------------------------------------
// The segment starts travel BY VALUE in the kernel arguments (up to 32 per launch): no table upload, no host synchronisation,
// so asx_ht_*_dev / asx_hd_*_dev only enqueue work (capturable, overlappable with a gather -- VERDICT r2 weak #11).
struct HtStarts {
  int64_t v[32];
};
__global__ __launch_bounds__(256) void ht_gather_kernel(const float *__restrict__ song, int64_t N, HtStarts start, int64_t L,
                                                        const double *__restrict__ ref_acc, int standardize,
                                                        float *__restrict__ seg) {
  const int b = blockIdx.z, ch = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const int64_t j = start.v[b] + i;
  float v = 0.f;
  if (j >= 0 && j < N) {
    v = song[(int64_t)ch * N + j];
    if (standardize) {
      float mean, stdv;
      sample_mean_std(ref_acc, 0, (double)N, mean, stdv);
      v = (v - mean) / stdv;
    }
  }
  seg[((int64_t)b * 2 + ch) * L + i] = v;
}

static inline void ht_gather_launch(const float *song, int64_t N, const int64_t *host_starts, int B, int64_t L, const double *ref_acc,
                                    int standardize, float *seg, hipStream_t s) {
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int nb = B - b0 < 32 ? B - b0 : 32;
    HtStarts st{};
    for (int i = 0; i < nb; ++i) st.v[i] = host_starts[b0 + i];
    hipLaunchKernelGGL(ht_gather_kernel, dim3((unsigned)((L + 255) / 256), 2, nb), dim3(256), 0, s, song, N, st, L, ref_acc, standardize,
                       seg + (size_t)b0 * 2 * L);
  }
}

// ---- BagOfModels on the device (apply.py:169-196, demucs_separator.py:171-189) --------------------------------------------
// mix -> (mix - ref.mean()) / ref.std()  (the standardised mix every bag member demixes)
__global__ __launch_bounds__(256) void ht_standardize_kernel(const float *__restrict__ mix, int64_t n2, int64_t N,
                                                             const double *__restrict__ ref_acc, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n2) return;
  float mean, stdv;
  sample_mean_std(ref_acc, 0, (double)N, mean, stdv);
  out[i] = (mix[i] - mean) / stdv;
}
struct BagWeights {
  float v[16];
};
// estimates += out * weight (per source; the first member initialises): float32, product rounded before the sum
__global__ __launch_bounds__(256) void ht_bag_accumulate_kernel(float *__restrict__ est, const float *__restrict__ member, int64_t per_source,
                                                                BagWeights w, int first) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per_source) return;
  const float m = member[s * per_source + i] * w.v[s];
  est[s * per_source + i] = first ? m : est[s * per_source + i] + m;
}
// estimates[:, k] /= totals[k]; sources * ref.std() + ref.mean(); sources[[0, 1]] = sources[[1, 0]] -- est [S, 2, N] -> out [S, 2, N]
__global__ __launch_bounds__(256) void ht_bag_finish_kernel(const float *__restrict__ est, int64_t per_source, int64_t N, BagWeights totals,
                                                            const double *__restrict__ ref_acc, int standardize, int swap01,
                                                            float *__restrict__ out) {
#pragma clang fp contract(off)
  const int s = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= per_source) return;
  float v = est[s * per_source + i] / totals.v[s];
  if (standardize) {
    float mean, stdv;
    sample_mean_std(ref_acc, 0, (double)N, mean, stdv);
    v = v * stdv + mean;
  }
  const int so = (swap01 && s < 2) ? 1 - s : s;
  out[so * per_source + i] = v;
}

// mono reference: ref[i] = mean over channels (demucs_separator.py:171)
__global__ __launch_bounds__(256) void ht_mono_kernel(const float *__restrict__ song, int64_t N, float *__restrict__ ref) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) ref[i] = (song[i] + song[N + i]) / 2.0f;
}

// fold of one shift (apply.py:215-250 then :207-213): view sample u = n + lead is covered by chunks k with
// view offset k*stride; so = sum_k w[u - k*stride] * y_k[trim_k + u - k*stride] / sum_k w[..];
// out = (first ? 0 : out) + so; the last shift divides by `shifts` and de-standardises (* std + mean).
__global__ __launch_bounds__(256) void ht_fold_kernel(const float *__restrict__ chunk_out, int n_chunks, int SC,
                                                      int64_t TL, int64_t stride, int64_t segment, int64_t VL,
                                                      int64_t lead, const float *__restrict__ weight, int first,
                                                      int last, int shifts, const double *__restrict__ ref_acc,
                                                      int standardize, int swap01, int center, int64_t N,
                                                      float *__restrict__ out) {
  const int sc_ = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int64_t u = n + lead;
  int64_t k_hi = u / stride;
  if (k_hi > n_chunks - 1) k_hi = n_chunks - 1;
  int64_t k_lo = (u - segment + stride) / stride;
  if (u - segment + 1 <= 0) k_lo = 0;
  float num = 0.f, den = 0.f;
  for (int64_t k = k_lo; k <= k_hi; ++k) {
    const int64_t off = k * stride;
    const int64_t clen = (VL - off < segment) ? VL - off : segment;
    const int64_t j = u - off;
    if (j < 0 || j >= clen) continue;
    const int64_t trim = center ? (TL - clen) / 2 : 0;   // Demucs v3 chunks run unpadded (engine_hd.h)
    const float w = weight[j];
    num += w * chunk_out[((int64_t)k * SC + sc_) * TL + trim + j];
    den += w;
  }
  int so_ = sc_;
  if (swap01 && (sc_ >> 1) < 2) so_ = ((1 - (sc_ >> 1)) << 1) | (sc_ & 1);
  float *op = out + (int64_t)so_ * N + n;
  float v = num / den;
  if (!first) v = *op + v;
  if (last) {
    v = v / (float)shifts;
    if (standardize) {
      float mean, stdv;
      sample_mean_std(ref_acc, 0, (double)N, mean, stdv);
      v = v * stdv + mean;
    }
  }
  *op = v;
}

// ---- a pool of songs (asx_ht_demix_batch_dev / asx_hd_demix_batch_dev): twins of ht_gather_kernel and ht_fold_kernel ----------
// Every row of a forward batch may come from another song: song pointer, length, start and the song's slot of ref_acc travel BY
// VALUE like HtStarts (up to 32 rows per launch, 32 bytes each).  Per element the arithmetic of ht_gather_kernel.
struct HtPoolRow {
  const float *song;   // [2, N]
  int64_t N, start;
  int slot, pad_;
};
struct HtPoolRows {
  HtPoolRow v[32];
};
__global__ __launch_bounds__(256) void ht_gather_pool_kernel(HtPoolRows rows, int64_t L, const double *__restrict__ ref_acc, int standardize,
                                                             float *__restrict__ seg) {
  const int b = blockIdx.z, ch = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L) return;
  const float *__restrict__ song = rows.v[b].song;
  const int64_t N = rows.v[b].N;
  const int64_t j = rows.v[b].start + i;
  float v = 0.f;
  if (j >= 0 && j < N) {
    v = song[(int64_t)ch * N + j];
    if (standardize) {
      float mean, stdv;
      sample_mean_std(ref_acc, rows.v[b].slot, (double)N, mean, stdv);
      v = (v - mean) / stdv;
    }
  }
  seg[((int64_t)b * 2 + ch) * L + i] = v;
}

static inline void ht_gather_pool_launch(const HtPoolRow *host_rows, int B, int64_t L, const double *ref_acc, int standardize, float *seg,
                                         hipStream_t s) {
  for (int b0 = 0; b0 < B; b0 += 32) {
    const int nb = B - b0 < 32 ? B - b0 : 32;
    HtPoolRows r{};
    for (int i = 0; i < nb; ++i) r.v[i] = host_rows[b0 + i];
    hipLaunchKernelGGL(ht_gather_pool_kernel, dim3((unsigned)((L + 255) / 256), 2, nb), dim3(256), 0, s, r, L, ref_acc, standardize,
                       seg + (size_t)b0 * 2 * L);
  }
}

// The fold of ONE shift index for up to 32 songs in one launch.  blockIdx.x runs over the songs' sample ranges laid end to end,
// each rounded up to whole blocks (`block0` = the song's first block; songs past `n` are never reached), so a block belongs to
// one song and finds it with a scan of launch arguments.  From there on it is ht_fold_kernel per sample: the same k loop, first /
// last / shifts handling, de-standardisation (the song's own ref_acc slot), swap01 and centre trim, on that song's rows of the
// pooled chunk slab and that song's out [S, 2, N].
struct HtFoldSong {
  float *out;                    // [S, 2, N]
  int64_t N, VL, lead;
  int first, nk, slot, block0;   // rows [first, first + nk) of the pooled slab
};
struct HtFoldSongs {
  HtFoldSong v[32];
  int n, blocks;                 // songs in this launch, blocks they take together
};
__global__ __launch_bounds__(256) void ht_fold_pool_kernel(const float *__restrict__ chunk_all, HtFoldSongs songs, int SC, int64_t TL,
                                                           int64_t stride, int64_t segment, const float *__restrict__ weight, int first,
                                                           int last, int shifts, const double *__restrict__ ref_acc, int standardize,
                                                           int swap01, int center) {
  const int sc_ = blockIdx.y;
  int si = 0;
  while (si + 1 < songs.n && (int)blockIdx.x >= songs.v[si + 1].block0) ++si;
  const int64_t N = songs.v[si].N, VL = songs.v[si].VL;
  const int n_chunks = songs.v[si].nk;
  const float *__restrict__ chunk_out = chunk_all + (int64_t)songs.v[si].first * SC * TL;
  const int64_t n = (int64_t)((int)blockIdx.x - songs.v[si].block0) * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int64_t u = n + songs.v[si].lead;
  int64_t k_hi = u / stride;
  if (k_hi > n_chunks - 1) k_hi = n_chunks - 1;
  int64_t k_lo = (u - segment + stride) / stride;
  if (u - segment + 1 <= 0) k_lo = 0;
  float num = 0.f, den = 0.f;
  for (int64_t k = k_lo; k <= k_hi; ++k) {
    const int64_t off = k * stride;
    const int64_t clen = (VL - off < segment) ? VL - off : segment;
    const int64_t j = u - off;
    if (j < 0 || j >= clen) continue;
    const int64_t trim = center ? (TL - clen) / 2 : 0;
    const float w = weight[j];
    num += w * chunk_out[((int64_t)k * SC + sc_) * TL + trim + j];
    den += w;
  }
  int so_ = sc_;
  if (swap01 && (sc_ >> 1) < 2) so_ = ((1 - (sc_ >> 1)) << 1) | (sc_ & 1);
  float *op = songs.v[si].out + (int64_t)so_ * N + n;
  float v = num / den;
  if (!first) v = *op + v;
  if (last) {
    v = v / (float)shifts;
    if (standardize) {
      float mean, stdv;
      sample_mean_std(ref_acc, songs.v[si].slot, (double)N, mean, stdv);
      v = v * stdv + mean;
    }
  }
  *op = v;
}

// ---------------------------------------------------------------------------
// mha6_kernel: mha_kernel on the bf16 matrix pipe with fp32 results (kernels_rof.h: attention6_kernel has the scheme -- six bf16
// MFMA products on exactly split operands, Q split in registers, K and the transposed V split by the staging threads, P split
// from the S accumulators in place).  Head dims 16 DT <= 64: the K image and the Q fragments are 64 dims wide (dims >= DH are
// zero on the Q side, so whatever the K image holds there contributes nothing -- it is zeroed once all the same), the V^T
// image has DH rows.  No decay variant (Demucs v3's LocalState keeps mha_kernel).  QW = 16-query groups per wave.
// ---------------------------------------------------------------------------
// H: the fp16 x 3 arithmetic, block exponents as in attention6_kernel<QW, true> (per query, per K tile, running per V tile, none for P).
template <int DT, int QW, bool H = false>
__global__ __launch_bounds__(256, (QW == 1 ? 3 : 2)) void mha6_kernel(MhaArgs a) {
  constexpr int DH = 16 * DT, C4 = DH / 4;
  constexpr int NP = H ? 2 : 3;
  constexpr int PARTB = 64 * 128;
  static_assert(DT >= 1 && DT <= 4, "head dim");
  __shared__ __attribute__((aligned(16))) char lds6[2 * NP * PARTB];
  __shared__ __attribute__((aligned(16))) float tile_mx[8];
  char *Kp = lds6, *Vp = lds6 + NP * PARTB;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int qt = lid % a.nqt;
  lid /= a.nqt;
  const int h = lid % a.heads, b = lid / a.heads;
  const int q0 = qt * 64 * QW;
  const float *qp = a.q + (int64_t)b * a.nq * a.ldq + h * DH;
  const float *kp = a.k + (int64_t)b * a.nk * a.ldk + h * DH;
  const float *vp = a.v + (int64_t)b * a.nk * a.ldv + h * DH;

  if constexpr (DH < 64) {                             // dims DH .. 63 of the K image are never written below
    for (int e = tid; e < NP * PARTB / 16; e += 256) reinterpret_cast<u32x4 *>(Kp)[e] = (u32x4){0u, 0u, 0u, 0u};
    __syncthreads();
  }

  // ---- Q operand of this lane: query q0 + 16 (wave QW + g) + li, dims 32 ks + 8 lk .. + 7 (zero past DH) ----
  u32x4 qf[QW][2][NP];
  int eq[QW];                                          // H: exponent of this lane's query
#pragma unroll
  for (int g = 0; g < QW; ++g) {
    const int q = q0 + (wave * QW + g) * 16 + li;
    const bool ok = q < a.nq;
    const float *qr = qp + (int64_t)(ok ? q : 0) * a.ldq + 8 * lk;
    f32x4 qv[2][2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qv[ks][0] = (f32x4){0.f, 0.f, 0.f, 0.f};
      qv[ks][1] = qv[ks][0];
      if (ok && 32 * ks + 8 * lk < DH) {               // DH % 8 == 0: an 8-dim group is inside the head or past it as a whole
        qv[ks][0] = *reinterpret_cast<const f32x4 *>(qr + 32 * ks);
        qv[ks][1] = *reinterpret_cast<const f32x4 *>(qr + 32 * ks + 4);
      }
    }
    eq[g] = 0;
    if constexpr (H) {
      float m = fmaxf(absmax_oct(qv[0][0], qv[0][1]), absmax_oct(qv[1][0], qv[1][1]));
      m = fmaxf(m, __shfl_xor(m, 16));
      m = fmaxf(m, __shfl_xor(m, 32));
      eq[g] = f16_scale_exp(m);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      if constexpr (H) split2h_oct(qv[ks][0], qv[ks][1], eq[g], qf[g][ks][0], qf[g][ks][1]);
      else split3_oct(qv[ks][0], qv[ks][1], qf[g][ks][0], qf[g][ks][1], qf[g][ks][NP - 1]);
    }
  }

  f32x4 acc_o[QW][DT];
  float m_run[QW], l_run[QW];
#pragma unroll
  for (int g = 0; g < QW; ++g) {
#pragma unroll
    for (int i = 0; i < DT; ++i) acc_o[g][i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    m_run[g] = -INFINITY;
    l_run[g] = 0.f;
  }

  // ---- staging: thread (kb = tid >> 4, c4 = tid & 15) owns keys 4 kb .. + 3 x dims 4 c4 .. + 3 (idle for c4 >= DH / 4) ----
  const int kb = tid >> 4, c4 = tid & 15;
  const bool stg = c4 < C4;
  const int nkt = (a.nk + 63) / 64;
  f32x4 kreg[4], vreg[4];
  auto fetch = [&](int kt) {
    const int k0 = kt * 64 + 4 * kb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      kreg[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
      vreg[j] = kreg[j];
      if (stg && k0 + j < a.nk) {
        kreg[j] = *reinterpret_cast<const f32x4 *>(kp + (int64_t)(k0 + j) * a.ldk + c4 * 4);
        vreg[j] = *reinterpret_cast<const f32x4 *>(vp + (int64_t)(k0 + j) * a.ldv + c4 * 4);
      }
    }
  };
  const int vslot = ((kb >> 3) << 2) | (kb & 3), vhalf = (kb >> 2) & 1;
  int ek = 0, ev_run = 200;                            // H: exponent of the K tile in LDS; running exponent of V (and of the O accumulators)
  float fdev = 1.0f;                                   // H: 2^(drop of ev_run at this tile), applied with the softmax correction
  auto publish_tile_max = [&]() {                      // H: largest |K|, |V| of the fetched tile, per wave (idle staging lanes hold zeros)
    float mk = 0.f, mv = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      mk = fmaxf(mk, fmaxf(fmaxf(fabsf(kreg[j].x), fabsf(kreg[j].y)), fmaxf(fabsf(kreg[j].z), fabsf(kreg[j].w))));
      mv = fmaxf(mv, fmaxf(fmaxf(fabsf(vreg[j].x), fabsf(vreg[j].y)), fmaxf(fabsf(vreg[j].z), fabsf(vreg[j].w))));
    }
    mk = wave_max64(mk);
    mv = wave_max64(mv);
    if (lane == 0) {
      tile_mx[wave] = mk;
      tile_mx[4 + wave] = mv;
    }
  };
  auto stage = [&]() {
    if constexpr (H) {
      const f32x4 a4 = *reinterpret_cast<const f32x4 *>(tile_mx), b4 = *reinterpret_cast<const f32x4 *>(tile_mx + 4);
      ek = __builtin_amdgcn_readfirstlane(f16_scale_exp(fmaxf(fmaxf(a4.x, a4.y), fmaxf(a4.z, a4.w))));
      const int need = __builtin_amdgcn_readfirstlane(f16_scale_exp(fmaxf(fmaxf(b4.x, b4.y), fmaxf(b4.z, b4.w))));
      const int ev_new = need < ev_run ? need - 2 : ev_run;
      fdev = __builtin_ldexpf(1.0f, ev_new - ev_run);
      ev_run = ev_new;
    }
    if (!stg) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = 4 * kb + j;
      unsigned hh[2], mm[2], ll[2];
      if constexpr (H) {
        split2h_pair(kreg[j].x, kreg[j].y, ek, hh[0], ll[0]);
        split2h_pair(kreg[j].z, kreg[j].w, ek, hh[1], ll[1]);
      } else {
        split3_pair(kreg[j].x, kreg[j].y, hh[0], mm[0], ll[0]);
        split3_pair(kreg[j].z, kreg[j].w, hh[1], mm[1], ll[1]);
      }
      char *d = Kp + row * 128 + ((((c4 >> 1) ^ ((row >> 1) & 7)) << 4) | ((c4 & 1) << 3));
      *reinterpret_cast<uint2 *>(d) = make_uint2(hh[0], hh[1]);
      if constexpr (!H) *reinterpret_cast<uint2 *>(d + PARTB) = make_uint2(mm[0], mm[1]);
      *reinterpret_cast<uint2 *>(d + (NP - 1) * PARTB) = make_uint2(ll[0], ll[1]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = 4 * c4 + i;
      unsigned hh[2], mm[2], ll[2];
      if constexpr (H) {
        split2h_pair(vreg[0][i], vreg[1][i], ev_run, hh[0], ll[0]);
        split2h_pair(vreg[2][i], vreg[3][i], ev_run, hh[1], ll[1]);
      } else {
        split3_pair(vreg[0][i], vreg[1][i], hh[0], mm[0], ll[0]);
        split3_pair(vreg[2][i], vreg[3][i], hh[1], mm[1], ll[1]);
      }
      char *d = Vp + row * 128 + (((vslot ^ (((row >> 1) ^ (row >> 3)) & 7)) << 4) | (vhalf << 3));   // V^T swizzle: see the fragment read
      *reinterpret_cast<uint2 *>(d) = make_uint2(hh[0], hh[1]);
      if constexpr (!H) *reinterpret_cast<uint2 *>(d + PARTB) = make_uint2(mm[0], mm[1]);
      *reinterpret_cast<uint2 *>(d + (NP - 1) * PARTB) = make_uint2(ll[0], ll[1]);
    }
  };
  const int frow = li * 128, fsw = (li >> 1) & 7;

  fetch(0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * 64;
    if constexpr (H) publish_tile_max();
    __syncthreads();   // previous tile fully consumed
    stage();
    __syncthreads();
    if (kt + 1 < nkt) fetch(kt + 1);

    f32x4 st[QW][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
      for (int g = 0; g < QW; ++g) st[g][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < (DH + 31) / 32; ++ks) {
        const char *kq = Kp + mt * 2048 + frow + (((ks * 4 + lk) ^ fsw) << 4);
        if constexpr (H) {
          const f16x8 kh = *reinterpret_cast<const f16x8 *>(kq), kl = *reinterpret_cast<const f16x8 *>(kq + PARTB);
#pragma unroll
          for (int g = 0; g < QW; ++g) {
            const f16x8 qh = __builtin_bit_cast(f16x8, qf[g][ks][0]), ql = __builtin_bit_cast(f16x8, qf[g][ks][1]);
            st[g][mt] = ASX_MFMA_F16(kl, qh, st[g][mt]);
            st[g][mt] = ASX_MFMA_F16(kh, ql, st[g][mt]);
            st[g][mt] = ASX_MFMA_F16(kh, qh, st[g][mt]);
          }
          continue;
        }
        const bf16x8 kh = *reinterpret_cast<const bf16x8 *>(kq);
        const bf16x8 km = *reinterpret_cast<const bf16x8 *>(kq + PARTB);
        const bf16x8 kl = *reinterpret_cast<const bf16x8 *>(kq + (NP - 1) * PARTB);
#pragma unroll
        for (int g = 0; g < QW; ++g) {
          const bf16x8 qh = __builtin_bit_cast(bf16x8, qf[g][ks][0]), qm = __builtin_bit_cast(bf16x8, qf[g][ks][1]),
                       ql = __builtin_bit_cast(bf16x8, qf[g][ks][NP - 1]);
          st[g][mt] = ASX_MFMA_BF16(kl, qh, st[g][mt]);
          st[g][mt] = ASX_MFMA_BF16(kh, ql, st[g][mt]);
          st[g][mt] = ASX_MFMA_BF16(km, qm, st[g][mt]);
          st[g][mt] = ASX_MFMA_BF16(km, qh, st[g][mt]);
          st[g][mt] = ASX_MFMA_BF16(kh, qm, st[g][mt]);
          st[g][mt] = ASX_MFMA_BF16(kh, qh, st[g][mt]);
        }
      }
    }
#pragma unroll
    for (int g = 0; g < QW; ++g) {
      float mx = -INFINITY;
      const float sfac = H ? __builtin_ldexpf(a.scale, -(ek + eq[g])) : a.scale;   // H: back to the operands' own scale, exact
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = k0 + mt * 16 + 4 * lk + r;
          const float sv = (key < a.nk) ? st[g][mt][r] * sfac : -INFINITY;
          st[g][mt][r] = sv;
          mx = fmaxf(mx, sv);
        }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float m_new = fmaxf(m_run[g], mx);
      const float corr = (m_run[g] == -INFINITY) ? 0.f : (a.exact ? expf(m_run[g] - m_new) : __expf(m_run[g] - m_new));
      float psum = 0.f;
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = (st[g][mt][r] == -INFINITY) ? 0.f : (a.exact ? expf(st[g][mt][r] - m_new) : __expf(st[g][mt][r] - m_new));
          st[g][mt][r] = p;
          psum += p;
        }
      }
      psum += __shfl_xor(psum, 16);
      psum += __shfl_xor(psum, 32);
      l_run[g] = l_run[g] * corr + psum;
      m_run[g] = m_new;
      const float corr_o = H ? corr * fdev : corr;     // H: the O accumulators follow V's running exponent
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) acc_o[g][dt] *= corr_o;
    }
#pragma unroll
    for (int kp2 = 0; kp2 < 2; ++kp2) {
      if constexpr (H) {
        f16x8 p_h[QW], p_l[QW];
#pragma unroll
        for (int g = 0; g < QW; ++g) {
          u32x4 ph, pl;
          split2h_oct(st[g][2 * kp2], st[g][2 * kp2 + 1], 14, ph, pl);  // probabilities x 2^14 (kernels_rof.h: attention6_kernel); undone with V's exponent
          p_h[g] = __builtin_bit_cast(f16x8, ph);
          p_l[g] = __builtin_bit_cast(f16x8, pl);
        }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
          const char *vq = Vp + dt * 2048 + frow + (((kp2 * 4 + lk) ^ (fsw ^ ((2 * dt + (li >> 3)) & 7))) << 4);
          const f16x8 vh = *reinterpret_cast<const f16x8 *>(vq), vl = *reinterpret_cast<const f16x8 *>(vq + PARTB);
#pragma unroll
          for (int g = 0; g < QW; ++g) {
            acc_o[g][dt] = ASX_MFMA_F16(vl, p_h[g], acc_o[g][dt]);
            acc_o[g][dt] = ASX_MFMA_F16(vh, p_l[g], acc_o[g][dt]);
            acc_o[g][dt] = ASX_MFMA_F16(vh, p_h[g], acc_o[g][dt]);
          }
        }
        continue;
      }
      bf16x8 p_h[QW], p_m[QW], p_l[QW];
#pragma unroll
      for (int g = 0; g < QW; ++g) {
        u32x4 ph, pm, pl;
        split3_oct(st[g][2 * kp2], st[g][2 * kp2 + 1], ph, pm, pl);
        p_h[g] = __builtin_bit_cast(bf16x8, ph);
        p_m[g] = __builtin_bit_cast(bf16x8, pm);
        p_l[g] = __builtin_bit_cast(bf16x8, pl);
      }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const char *vq = Vp + dt * 2048 + frow + (((kp2 * 4 + lk) ^ (fsw ^ ((2 * dt + (li >> 3)) & 7))) << 4);   // V^T swizzle ((row >> 1) ^ (row >> 3)) & 7
        const bf16x8 vh = *reinterpret_cast<const bf16x8 *>(vq);
        const bf16x8 vm = *reinterpret_cast<const bf16x8 *>(vq + PARTB);
        const bf16x8 vl = *reinterpret_cast<const bf16x8 *>(vq + (NP - 1) * PARTB);
#pragma unroll
        for (int g = 0; g < QW; ++g) {
          acc_o[g][dt] = ASX_MFMA_BF16(vl, p_h[g], acc_o[g][dt]);
          acc_o[g][dt] = ASX_MFMA_BF16(vh, p_l[g], acc_o[g][dt]);
          acc_o[g][dt] = ASX_MFMA_BF16(vm, p_m[g], acc_o[g][dt]);
          acc_o[g][dt] = ASX_MFMA_BF16(vm, p_h[g], acc_o[g][dt]);
          acc_o[g][dt] = ASX_MFMA_BF16(vh, p_m[g], acc_o[g][dt]);
          acc_o[g][dt] = ASX_MFMA_BF16(vh, p_h[g], acc_o[g][dt]);
        }
      }
    }
  }

#pragma unroll
  for (int g = 0; g < QW; ++g) {
    const int q = q0 + (wave * QW + g) * 16 + li;
    if (q < a.nq) {
      const float inv = 1.0f / l_run[g];
      float *orow = a.out + ((int64_t)b * a.nq + q) * a.ldo + h * DH;
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        f32x4 o = acc_o[g][dt];
        o *= inv;
        if constexpr (H) {                             // V's exponent (exact)
          o.x = __builtin_ldexpf(o.x, -ev_run - 14);
          o.y = __builtin_ldexpf(o.y, -ev_run - 14);
          o.z = __builtin_ldexpf(o.z, -ev_run - 14);
          o.w = __builtin_ldexpf(o.w, -ev_run - 14);
        }
        *reinterpret_cast<f32x4 *>(orow + dt * 16 + 4 * lk) = o;
      }
    }
  }
}

}  // namespace asx
