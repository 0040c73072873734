// Stand-alone harness of the bf16x6 row GEMM (csrc/kernels_gemm3.h) against the fp32-MFMA kernel it replaces (kernels_gemm2.h)
// and a float64 host GEMM on sampled rows: error of both kernels, time per launch on the TDF / Roformer / Demucs shapes.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -o tools/proto_gemm3 tools/proto_gemm3.hip && tools/proto_gemm3 [abl] [first] [last] [tile_map] [h]
// h = 1: the fp16 x 3 arithmetic (tdf3_kernel<..., H = true>) in the tdf3 column; the "spread" shapes give x a 2^-20 decay along k (and
// weights that look at the quiet half only in the first 16 columns): the case a block exponent has to survive.
// argv[8] = 1: a TDF block's two linears through a pair image (run_chain); 2: the last linear with the output conv in its epilogue (run_cg).
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../python-audio-separator_amd/csrc/kernels_net.h"
#include "../python-audio-separator_amd/csrc/kernels_gemm2.h"
#include "../python-audio-separator_amd/csrc/kernels_gemm3.h"

using namespace asx;

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "HIP %s at line %d\n", hipGetErrorString(e_), __LINE__); \
      exit(2);                                                                 \
    }                                                                          \
  } while (0)

template <int NREP, int MREP, int ABL>
static void launch3(const TdfDmaArgs &a, const u32x4 *w3, hipStream_t s) {
  constexpr int BM = 16 * MREP, BN = 64 * NREP, LDS = 2 * 3 * BM * 64;
  const int64_t nbm = (a.M + BM - 1) / BM;
  const int nbn = (a.N + BN - 1) / BN;
  hipLaunchKernelGGL((tdf3_kernel<NREP, MREP, ABL>), dim3((unsigned)(nbm * nbn)), dim3(256), LDS, s, a, w3, RowGather{});
}
template <int NREP, int MREP>
static void launch2(const TdfDmaArgs &a, hipStream_t s) {
  constexpr int BM = 16 * MREP, BN = 64 * NREP, LDS = 2 * (BM + BN) * 32 * 4;
  static bool done = false;
  if (!done) {
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&tdf2_kernel<NREP, MREP, 0, 32>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    done = true;
  }
  const int64_t nbm = (a.M + BM - 1) / BM;
  const int nbn = (a.N + BN - 1) / BN;
  hipLaunchKernelGGL((tdf2_kernel<NREP, MREP, 0, 32>), dim3((unsigned)(nbm * nbn)), dim3(256), LDS, s, a, 1, -1);
}

template <int NREP, int MREP, int ABL = 0, bool PS = false, int NW = 4>
static void launch3h(const TdfDmaArgs &a, const u32x4 *w3, hipStream_t s) {
  constexpr int BM = 16 * MREP, BN = 16 * NREP * NW, LDS = tdf3h_lds_bytes(BM);
  const int64_t nbm = (a.M + BM - 1) / BM;
  const int nbn = (a.N + BN - 1) / BN;
  hipLaunchKernelGGL((tdf3_kernel<NREP, MREP, ABL, false, true, PS, NW>), dim3((unsigned)(nbm * nbn)), dim3(64 * NW), LDS, s, a, w3, RowGather{});
}

static int g_map = 0;   // TdfDmaArgs::tile_map of the tdf3 launches (argv[4])
static int g_h = 0;     // 1: fp16 x 3 (argv[5])
static int g_tile = 0;  // tile of the fp16 x 3 launches: 0 = 128 x 192, 1 = 128 x 128, 2 = 64 x 128 (argv[7])
static void launch3h_sel(const TdfDmaArgs &a, const u32x4 *w3, hipStream_t s);
static int g_full = 0;  // 1: compare the WHOLE output of two tdf3 runs bit for bit and against tdf2 (argv[6]) -- the sampled rows miss a rare race
struct Shape {
  const char *name;
  int64_t M;
  int N, K, C, T, relu, res, bias;
  int spread = 0;
  int rot = 0;            // 1: rotary epilogue on the first 2 N / 3 columns + a per-row factor (the BS-Roformer qkv projection); full compare only
};

static double run_shape(const Shape &sh, int abl, int reps) {
  const int64_t M = sh.M;
  const int N = sh.N, K = sh.K;
  std::mt19937 rng(1234 + N + K);
  std::normal_distribution<float> nd(0.f, 1.f);
  // host data only for the sampled rows: x is generated on the host in full when small, else tiled from a 4096-row block
  const int64_t HB = std::min<int64_t>(M, 4096);
  std::vector<float> hx((size_t)HB * K), hw((size_t)N * K), hb(N), hsc(sh.C), hsh(sh.C), hr((size_t)HB * N);
  for (auto &v : hx) v = nd(rng) * 3.0f;
  for (auto &v : hw) v = nd(rng) / std::sqrt((float)K);
  if (sh.spread) {
    for (int64_t r = 0; r < HB; ++r) {
      const float rowmag = std::ldexp(1.0f, (int)(r % 7) * 3 - 9);           // rows of one 128-row tile differ by up to 2^18
      for (int k = 0; k < K; ++k) hx[(size_t)r * K + k] *= rowmag * std::ldexp(1.0f, -(int)(20.0 * k / K));
    }
    for (int n = 0; n < std::min(N, 16); ++n)
      for (int k = 0; k < K / 2; ++k) hw[(size_t)n * K + k] = 0.f;          // these columns see the quiet half of k only
    for (int n = 16; n < std::min(N, 32); ++n)
      for (int k = 0; k < K; ++k) hw[(size_t)n * K + k] *= 1e-6f;           // a quiet weight tile
  }
  for (auto &v : hb) v = nd(rng);
  for (auto &v : hsc) v = 0.5f + 0.5f * std::fabs(nd(rng));
  for (auto &v : hsh) v = 0.2f * nd(rng);
  for (auto &v : hr) v = nd(rng);
  float *dx, *dw, *db, *dsc, *dsh, *dr, *dy2, *dy3;
  u32x4 *dw3;
  CK(hipMalloc(&dx, (size_t)M * K * 4));
  CK(hipMalloc(&dw, (size_t)N * K * 4));
  CK(hipMalloc(&db, N * 4));
  CK(hipMalloc(&dsc, sh.C * 4));
  CK(hipMalloc(&dsh, sh.C * 4));
  CK(hipMalloc(&dr, (size_t)M * N * 4));
  CK(hipMalloc(&dy2, (size_t)M * N * 4));
  CK(hipMalloc(&dy3, (size_t)M * N * 4));
  const int ntiles = (N + 15) / 16, nk = ((K + 63) / 64) * 2;
  CK(hipMalloc(&dw3, (size_t)ntiles * nk * 3 * 1024 + (size_t)ntiles * 16));
  for (int64_t r0 = 0; r0 < M; r0 += HB) {
    const int64_t n = std::min<int64_t>(HB, M - r0);
    CK(hipMemcpy(dx + r0 * K, hx.data(), (size_t)n * K * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dr + r0 * N, hr.data(), (size_t)n * N * 4, hipMemcpyHostToDevice));
  }
  CK(hipMemcpy(dw, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(db, hb.data(), N * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsc, hsc.data(), sh.C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsh, hsh.data(), sh.C * 4, hipMemcpyHostToDevice));
  CK(hipMemset(dy2, 0xff, (size_t)M * N * 4));
  CK(hipMemset(dy3, 0xff, (size_t)M * N * 4));

  float2 *drot = nullptr;
  float *drs = nullptr;
  if (sh.rot) {
    const int half = 32, pos_mod = 801;
    std::vector<float2> hrot((size_t)pos_mod * half);
    for (auto &v : hrot) {
      const float ang = nd(rng) * 3.0f;
      v = make_float2(std::cos(ang), std::sin(ang));
    }
    std::vector<float> hrs((size_t)M);
    for (auto &v : hrs) v = 0.5f + std::fabs(nd(rng));
    CK(hipMalloc(&drot, hrot.size() * 8));
    CK(hipMalloc(&drs, hrs.size() * 4));
    CK(hipMemcpy(drot, hrot.data(), hrot.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(drs, hrs.data(), hrs.size() * 4, hipMemcpyHostToDevice));
  }
  TdfDmaArgs a{};
  if (sh.rot) {
    if (sh.rot != 3) {
      a.rot_tab = drot;
      a.rot_cols = 2 * N / 3;
      a.rot_half = 32;
      a.rot_pos_mod = 801;
      a.rot_pos_div = 62;
    }
    if (sh.rot != 2) a.rscale = drs;
  }
  a.x = dx;
  a.w = dw;
  a.bias = sh.bias ? db : nullptr;
  a.scale = dsc;
  a.shift = dsh;
  a.res = sh.res ? dr : nullptr;
  a.y = dy2;
  a.M = M;
  a.N = N;
  a.K = K;
  a.C = sh.C;
  a.T = sh.T;
  a.relu = sh.relu;
  a.tile_map = g_map;

  const int64_t total = (int64_t)ntiles * nk * 64;
  if (g_h) hipLaunchKernelGGL(w3h_split_kernel<2>, dim3((unsigned)ntiles), dim3(256), 0, 0, dw, dw3, N, K, ntiles);
  else hipLaunchKernelGGL(w3_split_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, dw, dw3, N, K, total);
  CK(hipDeviceSynchronize());

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto time_it = [&](auto &&fn) {
    fn();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < reps; ++i) fn();
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms / reps;
  };
  a.y = dy2;
  const double t2 = time_it([&]() { launch2<3, 8>(a, 0); });
  a.y = dy3;
  double t3 = 0;
  switch (g_h ? 100 : abl) {
    case 100: t3 = time_it([&]() { launch3h_sel(a, dw3, 0); }); break;
    case 0: t3 = time_it([&]() { launch3<3, 8, 0>(a, dw3, 0); }); break;
    case 1: t3 = time_it([&]() { launch3<3, 8, 1>(a, dw3, 0); }); break;
    case 2: t3 = time_it([&]() { launch3<3, 8, 2>(a, dw3, 0); }); break;
    case 4: t3 = time_it([&]() { launch3<3, 8, 4>(a, dw3, 0); }); break;
    case 8: t3 = time_it([&]() { launch3<3, 8, 8>(a, dw3, 0); }); break;
    case 9: t3 = time_it([&]() { launch3<3, 8, 9>(a, dw3, 0); }); break;
    case 13: t3 = time_it([&]() { launch3<3, 8, 13>(a, dw3, 0); }); break;
    default: fprintf(stderr, "abl?\n"); exit(2);
  }
  CK(hipGetLastError());
  if (g_full) {
    float *dy3b;
    CK(hipMalloc(&dy3b, (size_t)M * N * 4));
    CK(hipMemset(dy3b, 0xff, (size_t)M * N * 4));
    a.y = dy3b;
    if (g_h) launch3h_sel(a, dw3, 0);
    else launch3<3, 8, 0>(a, dw3, 0);
    CK(hipDeviceSynchronize());
    const int64_t CH = 1 << 24;
    std::vector<float> b2(CH), b3(CH), b3b(CH);
    int64_t ndiff = 0, nbig = 0, first = -1;
    double worst = 0;
    for (int64_t o = 0; o < M * N; o += CH) {
      const int64_t n = std::min<int64_t>(CH, M * N - o);
      CK(hipMemcpy(b2.data(), dy2 + o, (size_t)n * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(b3.data(), dy3 + o, (size_t)n * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(b3b.data(), dy3b + o, (size_t)n * 4, hipMemcpyDeviceToHost));
      for (int64_t i = 0; i < n; ++i) {
        if (memcmp(&b3[i], &b3b[i], 4) != 0) {
          if (first < 0) first = o + i;
          if (ndiff < 4)
            printf("    row %lld col %lld: run A %.6e run B %.6e fp32 kernel %.6e\n", (long long)((o + i) / N), (long long)((o + i) % N), b3[i], b3b[i],
                   b2[i]);
          ++ndiff;
        }
        const double d = std::fabs((double)b3[i] - b2[i]);
        worst = std::max(worst, d);
        if (d > 1e-3 * (1.0 + std::fabs(b2[i]))) ++nbig;
      }
    }
    printf("  full compare: two tdf3 runs differ in %lld elements (first at row %lld col %lld); tdf3 vs tdf2: max abs %.3e, %lld elements off by > 1e-3\n",
           (long long)ndiff, (long long)(first < 0 ? -1 : first / N), (long long)(first < 0 ? -1 : first % N), worst, (long long)nbig);
    CK(hipFree(dy3b));
  }
  const double flops = 2.0 * M * N * K;

  // float64 reference on sampled rows (first HB rows suffice: the data repeats), both kernels
  const int nsamp = 64;
  std::vector<float> y2((size_t)N), y3((size_t)N);
  double e2 = 0, e3 = 0, d23 = 0, nrm = 0, mx2 = 0, mx3 = 0, worst3 = 0, worst2 = 0;   // worst*: row x column-group error over the group's own scale
  int nan3 = 0;
  for (int si = 0; si < nsamp; ++si) {
    int64_t row = (int64_t)((double)si / nsamp * M);
    if (si == nsamp - 1) row = M - 1;
    const int64_t hrow = row % HB;
    CK(hipMemcpy(y2.data(), dy2 + row * N, N * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(y3.data(), dy3 + row * N, N * 4, hipMemcpyDeviceToHost));
    const int c = (int)((row / sh.T) % sh.C);
    double ge2[3] = {0, 0, 0}, ge3[3] = {0, 0, 0}, gn[3] = {0, 0, 0};
    for (int n = 0; n < N; ++n) {
      double acc = 0;
      for (int k = 0; k < K; ++k) acc += (double)hx[hrow * K + k] * (double)hw[(size_t)n * K + k];
      double v = hsc[c] * (acc + (sh.bias ? hb[n] : 0.0)) + hsh[c];
      if (sh.relu == 1) v = v > 0 ? v : 0;
      if (sh.res) v += hr[hrow * N + n];
      if (!std::isfinite(y3[n])) ++nan3;
      e2 += (y2[n] - v) * (y2[n] - v);
      e3 += (y3[n] - v) * (y3[n] - v);
      d23 += ((double)y2[n] - y3[n]) * ((double)y2[n] - y3[n]);
      nrm += v * v;
      mx2 = std::max(mx2, std::fabs(y2[n] - v));
      mx3 = std::max(mx3, std::fabs(y3[n] - v));
      const int g = n < 16 ? 0 : (n < 32 ? 1 : 2);
      const double pre = hsc[c] * (acc + (sh.bias ? hb[n] : 0.0)) + hsh[c];   // scale of the group before ReLU / residual
      ge2[g] += (y2[n] - v) * (y2[n] - v);
      ge3[g] += (y3[n] - v) * (y3[n] - v);
      gn[g] += pre * pre;
    }
    for (int g = 0; g < 3; ++g)
      if (gn[g] > 0) {
        worst2 = std::max(worst2, std::sqrt(ge2[g] / gn[g]));
        worst3 = std::max(worst3, std::sqrt(ge3[g] / gn[g]));
      }
  }
  printf("%-22s M=%-8lld N=%-5d K=%-5d  tdf2 %8.3f ms %6.1f TF | tdf3 %8.3f ms %6.1f TF-eq (x%.2f) | relrms vs f64: tdf2 %.2e tdf3 %.2e  "
         "maxabs %.2e / %.2e  tdf2-vs-tdf3 %.2e  nonfinite %d  worst row-group %.2e / %.2e\n",
         sh.name, (long long)M, N, K, t2, flops / t2 * 1e-9, t3, flops / t3 * 1e-9, t2 / t3, std::sqrt(e2 / nrm), std::sqrt(e3 / nrm), mx2, mx3,
         std::sqrt(d23 / nrm), nan3, worst2, worst3);
  fflush(stdout);
  CK(hipFree(dx));
  CK(hipFree(dw));
  CK(hipFree(db));
  CK(hipFree(dsc));
  CK(hipFree(dsh));
  CK(hipFree(dr));
  CK(hipFree(dy2));
  CK(hipFree(dy3));
  CK(hipFree(dw3));
  return t3;
}


// ---- a TDF block's two linears with the bottleneck activations as a PAIR IMAGE (argv[8] = 1): gemm1 (F -> F/8, BN, ReLU) writes H split,
// gemm2 (F/8 -> F, BN, ReLU, + x) reads the parts; against the same two launches through an fp32 H, and a float64 chain on sampled rows
static void run_chain(const char *name, int64_t M, int F, int F8, int C, int T, int reps) {
  std::mt19937 rng(99 + F);
  std::normal_distribution<float> nd(0.f, 1.f);
  const int64_t HB = std::min<int64_t>(M, 4096);
  std::vector<float> hx((size_t)HB * F), hw1((size_t)F8 * F), hw2((size_t)F * F8), hsc1(C), hsh1(C), hsc2(C), hsh2(C);
  for (int64_t r = 0; r < HB; ++r) {
    const float rowmag = std::ldexp(1.0f, (int)(r % 5) * 4 - 8);   // rows of a tile differ by up to 2^16
    for (int k = 0; k < F; ++k) hx[(size_t)r * F + k] = nd(rng) * 3.0f * rowmag;
  }
  for (auto &v : hw1) v = nd(rng) / std::sqrt((float)F);
  for (auto &v : hw2) v = nd(rng) / std::sqrt((float)F8);
  for (int n = 0; n < F8 / 2; ++n)                       // the first half of H's columns (one exponent span of two) is 2^-12 of the second
    for (int k = 0; k < F; ++k) hw1[(size_t)n * F + k] *= 2.44140625e-4f;
  for (int c = 0; c < C; ++c) {
    hsc1[c] = 0.5f + 0.5f * std::fabs(nd(rng));
    hsh1[c] = 0.2f * nd(rng) * 1e-3f;
    hsc2[c] = 0.5f + 0.5f * std::fabs(nd(rng));
    hsh2[c] = 0.2f * nd(rng);
  }
  float *dx, *dw1, *dw2, *dsc1, *dsh1, *dsc2, *dsh2, *dhA, *dhB, *dyA, *dyB;
  int *dexp;
  u32x4 *dw31, *dw32;
  CK(hipMalloc(&dx, (size_t)M * F * 4));
  CK(hipMalloc(&dw1, hw1.size() * 4));
  CK(hipMalloc(&dw2, hw2.size() * 4));
  CK(hipMalloc(&dsc1, C * 4));
  CK(hipMalloc(&dsh1, C * 4));
  CK(hipMalloc(&dsc2, C * 4));
  CK(hipMalloc(&dsh2, C * 4));
  CK(hipMalloc(&dhA, (size_t)M * F8 * 4));
  CK(hipMalloc(&dhB, (size_t)M * F8 * 4));
  CK(hipMalloc(&dyA, (size_t)M * F * 4));
  CK(hipMalloc(&dyB, (size_t)M * F * 4));
  const int cols = 192, nsp = (F8 + cols - 1) / cols;
  CK(hipMalloc(&dexp, (size_t)M * nsp * 4));
  for (int64_t r0 = 0; r0 < M; r0 += HB) CK(hipMemcpy(dx + r0 * F, hx.data(), (size_t)std::min<int64_t>(HB, M - r0) * F * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dw1, hw1.data(), hw1.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dw2, hw2.data(), hw2.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsc1, hsc1.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsh1, hsh1.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsc2, hsc2.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsh2, hsh2.data(), C * 4, hipMemcpyHostToDevice));
  auto image = [&](const float *dw, int N, int K, u32x4 *&img) {
    const int ntiles = (N + 15) / 16, nk = ((K + 63) / 64) * 2;
    CK(hipMalloc(&img, (size_t)ntiles * nk * 2 * 1024 + (size_t)ntiles * 16));
    hipLaunchKernelGGL(w3h_split_kernel<2>, dim3((unsigned)ntiles), dim3(256), 0, 0, dw, img, N, K, ntiles);
  };
  image(dw1, F8, F, dw31);
  image(dw2, F, F8, dw32);
  CK(hipDeviceSynchronize());
  TdfDmaArgs g1{}, g2{};
  g1.x = dx; g1.w = dw1; g1.scale = dsc1; g1.shift = dsh1; g1.M = M; g1.N = F8; g1.K = F; g1.C = C; g1.T = T; g1.relu = 1; g1.tile_map = 1;
  g2.w = dw2; g2.scale = dsc2; g2.shift = dsh2; g2.res = dx; g2.M = M; g2.N = F; g2.K = F8; g2.C = C; g2.T = T; g2.relu = 1; g2.tile_map = 0;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto time_it = [&](auto &&fn) {
    fn();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < reps; ++i) fn();
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms / reps;
  };
  TdfDmaArgs a1 = g1, a2 = g2, b1 = g1, b2 = g2;
  a1.y = dhA; a2.x = dhA; a2.y = dyA;
  b1.y = dhB; b1.yexp = dexp; b1.yexp_n = nsp;
  b2.x = dhB; b2.y = dyB; b2.xexp = dexp; b2.xexp_n = nsp; b2.xexp_gs = cols / 32; b2.xexp_inv = (65536 + b2.xexp_gs - 1) / b2.xexp_gs;
  const double tA1 = time_it([&]() { launch3h<3, 8>(a1, dw31, 0); });
  const double tA2 = time_it([&]() { launch3h<3, 8>(a2, dw32, 0); });
  const double tB1 = time_it([&]() { launch3h<3, 8>(b1, dw31, 0); });
  const double tB2 = time_it([&]() { launch3h<3, 8, 0, true>(b2, dw32, 0); });
  CK(hipGetLastError());
  // sampled rows against float64
  const int nsamp = 48;
  std::vector<float> yA(F), yB(F), hA(F8);
  std::vector<uint32_t> hBraw(F8);
  std::vector<int> ex(nsp);
  double eA = 0, eB = 0, nrm = 0, dAB = 0, hdec = 0, hnrm = 0, worstq = 0;
  int nonfin = 0;
  for (int si = 0; si < nsamp; ++si) {
    int64_t row = (int64_t)((double)si / nsamp * M);
    if (si == nsamp - 1) row = M - 1;
    const int64_t hrow = row % HB;
    const int c = (int)((row / T) % C);
    CK(hipMemcpy(yA.data(), dyA + row * F, F * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(yB.data(), dyB + row * F, F * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hA.data(), dhA + row * F8, F8 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hBraw.data(), dhB + row * F8, F8 * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ex.data(), dexp + row * nsp, nsp * 4, hipMemcpyDeviceToHost));
    std::vector<double> h64(F8);
    for (int n = 0; n < F8; ++n) {
      double acc = 0;
      for (int k = 0; k < F; ++k) acc += (double)hx[hrow * F + k] * (double)hw1[(size_t)n * F + k];
      const double v = hsc1[c] * acc + hsh1[c];
      h64[n] = v > 0 ? v : 0;
    }
    // decode the pair image: group of four columns = four h then four l
    double qmax[2] = {0, 0}, qerr[2] = {0, 0};
    for (int n = 0; n < F8; ++n) {
      const int g = n >> 2, i = n & 3;
      const uint16_t *p = reinterpret_cast<const uint16_t *>(hBraw.data() + g * 4);
      auto f16 = [](uint16_t b) {
        const int s = b >> 15, e = (b >> 10) & 31, m = b & 1023;
        double v = e == 0 ? std::ldexp((double)m, -24) : (e == 31 ? (m ? NAN : INFINITY) : std::ldexp(1.0 + m / 1024.0, e - 15));
        return s ? -v : v;
      };
      const double dec = std::ldexp(f16(p[i]) + f16(p[4 + i]), -ex[n / cols]);
      hdec += (dec - hA[n]) * (dec - hA[n]);
      hnrm += (double)hA[n] * hA[n];
      const int q = n / cols;
      qmax[q] = std::max(qmax[q], std::fabs((double)hA[n]));
      qerr[q] = std::max(qerr[q], std::fabs(dec - hA[n]));
    }
    for (int q = 0; q < 2 && q < nsp; ++q)
      if (qmax[q] > 0) worstq = std::max(worstq, qerr[q] / qmax[q]);
    for (int n = 0; n < F; ++n) {
      double acc = 0;
      for (int k = 0; k < F8; ++k) acc += h64[k] * (double)hw2[(size_t)n * F8 + k];
      double v = hsc2[c] * acc + hsh2[c];
      v = (v > 0 ? v : 0) + hx[hrow * F + n];
      if (!std::isfinite(yB[n])) ++nonfin;
      eA += (yA[n] - v) * (yA[n] - v);
      eB += (yB[n] - v) * (yB[n] - v);
      dAB += ((double)yA[n] - yB[n]) * ((double)yA[n] - yB[n]);
      nrm += v * v;
    }
  }
  printf("%-14s M=%-8lld F=%-5d F/8=%-4d | gemm1 fp32-out %.3f ms, pair-image-out %.3f ms | gemm2 fp32-in %.3f ms, pair-image-in %.3f ms | block %.3f -> %.3f ms\n"
         "    y vs f64: fp32 H %.2e, pair image %.2e; the two %.2e apart; nonfinite %d | H decoded vs fp32 H: rel rms %.2e, worst |d| / span max %.2e\n",
         name, (long long)M, F, F8, tA1, tB1, tA2, tB2, tA1 + tA2, tB1 + tB2, std::sqrt(eA / nrm), std::sqrt(eB / nrm), std::sqrt(dAB / nrm), nonfin,
         std::sqrt(hdec / hnrm), worstq);
  fflush(stdout);
  for (void *p : {(void *)dx, (void *)dw1, (void *)dw2, (void *)dsc1, (void *)dsh1, (void *)dsc2, (void *)dsh2, (void *)dhA, (void *)dhB, (void *)dyA,
                  (void *)dyB, (void *)dexp, (void *)dw31, (void *)dw32})
    CK(hipFree(p));
}

// ---- the net's last linear with the 48 -> 4 output conv in its epilogue (argv[8] = 2): tdf3_kernel<2, 12, ..., CG> on channel-grouped row
// tiles against the 128 x 192 tile that writes y, and the 192 x 128 tile on plain rows (the tile shape alone); the fused output against a
// float64 output conv of the y the 128 x 192 launch wrote, on sampled (b, t)
static void launch3h_cg(const TdfDmaArgs &a, const u32x4 *w3, hipStream_t s) {
  constexpr int LDS = tdf3h_lds_bytes(TdfCgMap::BM);
  static bool done = false;
  if (!done) {
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&tdf3_kernel<2, 12, 0, false, true, false, 4, true>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    CK(hipFuncSetAttribute(reinterpret_cast<const void *>(&tdf3_kernel<2, 12, 0, false, true, false, 4, false>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    done = true;
  }
  const unsigned grid = (unsigned)((a.M / TdfCgMap::BM) * (a.N / TdfCgMap::BN));
  if (a.fo_out) hipLaunchKernelGGL((tdf3_kernel<2, 12, 0, false, true, false, 4, true>), dim3(grid), dim3(256), LDS, s, a, w3, RowGather{});
  else hipLaunchKernelGGL((tdf3_kernel<2, 12, 0, false, true, false, 4, false>), dim3(grid), dim3(256), LDS, s, a, w3, RowGather{});
}
static void run_cg(const char *name, int B, int T, int N, int K, int reps) {
  const int C = TdfCgMap::C;
  const int64_t M = (int64_t)B * C * T;
  if (T % 4 || N % 128 || K % 32) { fprintf(stderr, "run_cg: shape\n"); exit(2); }
  std::mt19937 rng(7 + N + T);
  std::normal_distribution<float> nd(0.f, 1.f);
  const int64_t HB = std::min<int64_t>(M, 4096);
  std::vector<float> hx((size_t)HB * K), hw((size_t)N * K), hsc(C), hsh(C), hr((size_t)HB * N), hwo(4 * C + 4), hwt(4 * C + 4);
  for (int64_t r = 0; r < HB; ++r) {
    const float rowmag = std::ldexp(1.0f, (int)(r % 5) * 3 - 6);
    for (int k = 0; k < K; ++k) hx[(size_t)r * K + k] = nd(rng) * rowmag;
  }
  for (auto &v : hw) v = nd(rng) / std::sqrt((float)K);
  for (auto &v : hsc) v = 0.5f + 0.5f * std::fabs(nd(rng));
  for (auto &v : hsh) v = 0.2f * nd(rng);
  for (auto &v : hr) v = nd(rng);
  for (auto &v : hwo) v = nd(rng) / std::sqrt((float)C);       // w_out [4][48], b_out [4]
  for (int oc = 0; oc < 4; ++oc)
    for (int c = 0; c < C; ++c) hwt[c * 4 + oc] = hwo[oc * C + c];
  for (int oc = 0; oc < 4; ++oc) hwt[4 * C + oc] = hwo[4 * C + oc];
  float *dx, *dw, *dsc, *dsh, *dr, *dy, *dwo, *dout;
  u32x4 *dw3;
  CK(hipMalloc(&dx, (size_t)M * K * 4));
  CK(hipMalloc(&dw, hw.size() * 4));
  CK(hipMalloc(&dsc, C * 4));
  CK(hipMalloc(&dsh, C * 4));
  CK(hipMalloc(&dr, (size_t)M * N * 4));
  CK(hipMalloc(&dy, (size_t)M * N * 4));
  CK(hipMalloc(&dwo, hwt.size() * 4));
  CK(hipMalloc(&dout, (size_t)B * 4 * T * N * 4));
  for (int64_t r0 = 0; r0 < M; r0 += HB) {
    const int64_t n = std::min<int64_t>(HB, M - r0);
    CK(hipMemcpy(dx + r0 * K, hx.data(), (size_t)n * K * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dr + r0 * N, hr.data(), (size_t)n * N * 4, hipMemcpyHostToDevice));
  }
  CK(hipMemcpy(dw, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsc, hsc.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dsh, hsh.data(), C * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(dwo, hwt.data(), hwt.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemset(dout, 0xff, (size_t)B * 4 * T * N * 4));
  const int ntiles = (N + 15) / 16, nk = ((K + 63) / 64) * 2;
  CK(hipMalloc(&dw3, (size_t)ntiles * nk * 2 * 1024 + (size_t)ntiles * 16));
  hipLaunchKernelGGL(w3h_split_kernel<2>, dim3((unsigned)ntiles), dim3(256), 0, 0, dw, dw3, N, K, ntiles);
  CK(hipDeviceSynchronize());
  TdfDmaArgs a{};
  a.x = dx; a.w = dw; a.scale = dsc; a.shift = dsh; a.res = dr; a.y = dy; a.M = M; a.N = N; a.K = K; a.C = C; a.T = T; a.relu = 1;
  a.tile_map = (N + 127) / 128 < 8 ? 1 : 0;
  TdfDmaArgs f = a;
  f.y = nullptr; f.fo_w = dwo; f.fo_out = dout; f.fo_bs = (int64_t)4 * T * N;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  auto time_it = [&](auto &&fn) {
    fn();
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0, 0));
    for (int i = 0; i < reps; ++i) fn();
    CK(hipEventRecord(e1, 0));
    CK(hipEventSynchronize(e1));
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    return (double)ms / reps;
  };
  const double t_cg = time_it([&]() { launch3h_cg(f, dw3, 0); });
  const double t_212 = time_it([&]() { launch3h_cg(a, dw3, 0); });
  const double t_38 = time_it([&]() { launch3h<3, 8>(a, dw3, 0); });     // last: dy holds ITS y below
  CK(hipGetLastError());
  // second fused run into another buffer: bit for bit
  float *dout2;
  CK(hipMalloc(&dout2, (size_t)B * 4 * T * N * 4));
  f.fo_out = dout2;
  launch3h_cg(f, dw3, 0);
  CK(hipDeviceSynchronize());
  const int nsamp = 32;
  std::vector<float> yrow(N), o1(N), o2(N);
  std::vector<double> ref((size_t)4 * N);
  double err = 0, nrm = 0;
  long long ndiff = 0, nonfin = 0;
  for (int si = 0; si < nsamp; ++si) {
    const int b = (int)((int64_t)si * B / nsamp), t = (si * 37 + 3) % T;
    std::fill(ref.begin(), ref.end(), 0.0);
    for (int c = 0; c < C; ++c) {
      CK(hipMemcpy(yrow.data(), dy + (((int64_t)b * C + c) * T + t) * N, N * 4, hipMemcpyDeviceToHost));
      for (int oc = 0; oc < 4; ++oc)
        for (int n = 0; n < N; ++n) ref[(size_t)oc * N + n] += (double)hwo[oc * C + c] * yrow[n];
    }
    for (int oc = 0; oc < 4; ++oc) {
      const int64_t off = (((int64_t)b * 4 + oc) * T + t) * N;
      CK(hipMemcpy(o1.data(), dout + off, N * 4, hipMemcpyDeviceToHost));
      CK(hipMemcpy(o2.data(), dout2 + off, N * 4, hipMemcpyDeviceToHost));
      for (int n = 0; n < N; ++n) {
        const double v = ref[(size_t)oc * N + n] + hwo[4 * C + oc];
        if (!std::isfinite(o1[n])) ++nonfin;
        if (memcmp(&o1[n], &o2[n], 4) != 0) ++ndiff;
        err += (o1[n] - v) * (o1[n] - v);
        nrm += v * v;
      }
    }
  }
  printf("%-14s B=%d T=%d N=%d K=%d | 128x192 (writes y) %.3f ms | 192x128 plain rows (writes y) %.3f ms | 192x128 channel-grouped + output conv %.3f ms\n"
         "    fused output vs float64 conv of the 128x192 y: rel rms %.2e, nonfinite %lld, two fused runs differ in %lld of the sampled elements\n",
         name, B, T, N, K, t_38, t_212, t_cg, std::sqrt(err / nrm), nonfin, ndiff);
  fflush(stdout);
  for (void *p : {(void *)dx, (void *)dw, (void *)dsc, (void *)dsh, (void *)dr, (void *)dy, (void *)dwo, (void *)dout, (void *)dout2, (void *)dw3}) CK(hipFree(p));
}

static int g_habl = 0;  // ablation of the fp16 x 3 launches (argv[1] when h = 1): 1 no split, 4 no epilogue traffic, 8 no weight loads, 16 no rescale, sums
static void launch3h_sel(const TdfDmaArgs &a, const u32x4 *w3, hipStream_t s) {
  if (g_tile == 0 && g_habl) {
    switch (g_habl) {
      case 1: return launch3h<3, 8, 1>(a, w3, s);
      case 4: return launch3h<3, 8, 4>(a, w3, s);
      case 8: return launch3h<3, 8, 8>(a, w3, s);
      case 16: return launch3h<3, 8, 16>(a, w3, s);
      case 17: return launch3h<3, 8, 17>(a, w3, s);
      case 21: return launch3h<3, 8, 21>(a, w3, s);
      case 29: return launch3h<3, 8, 29>(a, w3, s);
      case 32: return launch3h<3, 8, 32>(a, w3, s);
      case 64: {   // timing only: the pair-image reader on fp32 data (garbage results) -- loads and LDS stores stay, the split arithmetic goes
        static int *zt = nullptr;
        if (!zt) {
          CK(hipMalloc(&zt, (size_t)1 << 22));
          CK(hipMemset(zt, 0, (size_t)1 << 22));
        }
        TdfDmaArgs b = a;
        b.xexp = zt;
        b.xexp_n = 1;
        b.xexp_gs = a.K / 32;
        b.xexp_inv = (65536 + b.xexp_gs - 1) / b.xexp_gs;
        return launch3h<3, 8, 0, true>(b, w3, s);
      }
      default: fprintf(stderr, "h abl?\n"); exit(2);
    }
  }
  if (g_tile == 3) return launch3h<3, 8, 0, false, 8>(a, w3, s);   // 128 x 384, eight waves
  if (g_tile == 4) return launch3h<2, 8, 0, false, 8>(a, w3, s);   // 128 x 256, eight waves
  if (g_tile == 1) launch3h<2, 8>(a, w3, s);
  else if (g_tile == 2) launch3h<2, 4>(a, w3, s);
  else launch3h<3, 8>(a, w3, s);
}

int main(int argc, char **argv) {
  const int abl = argc > 1 ? atoi(argv[1]) : 0;
  const int first = argc > 2 ? atoi(argv[2]) : 0;
  const int last = argc > 3 ? atoi(argv[3]) : 99;
  g_map = argc > 4 ? atoi(argv[4]) : 0;
  g_h = argc > 5 ? atoi(argv[5]) : 0;
  g_full = argc > 6 ? atoi(argv[6]) : 0;
  g_tile = argc > 7 ? atoi(argv[7]) : 0;
  if (g_h) g_habl = abl;
  if (argc > 8 && atoi(argv[8]) == 1) {
    run_chain("ragged small", 1000, 384, 192, 3, 8, 3);
    run_chain("tdf L0 block", 675840, 3072, 384, 48, 256, 5);
    run_chain("tdf L1 block", 675840, 1536, 192, 96, 128, 5);
    run_chain("tdf L2 block", 506880, 768, 96, 144, 64, 5);
    return 0;
  }
  if (argc > 8 && atoi(argv[8]) == 2) {
    run_cg("small", 3, 12, 768, 96, 3);
    run_cg("tdf L0 gemm2", 55, 256, 3072, 384, 5);
    return 0;
  }
  std::vector<Shape> shapes = {
      {"small ragged", 1000, 200, 192, 3, 8, 1, 1, 1},
      {"small gelu", 4096 + 64, 512, 256, 1, 1, 2, 1, 1},
      {"odd stages", 1000, 200, 96, 3, 8, 1, 1, 1},
      {"tdf L2 gemm2", 506880, 768, 96, 144, 64, 1, 1, 0},
      {"tdf L0 gemm1", 675840, 384, 3072, 48, 256, 1, 0, 0},
      {"tdf L0 gemm2", 675840, 3072, 384, 48, 256, 1, 1, 0},
      {"tdf L1 gemm1", 675840, 192, 1536, 96, 128, 1, 0, 0},
      {"tdf L1 gemm2", 675840, 1536, 192, 96, 128, 1, 1, 0},
      {"rof ff1", 480000, 2048, 512, 1, 1, 2, 0, 1},
      {"rof ff2", 480000, 512, 2048, 1, 1, 0, 1, 1},
      {"rof qkv", 480000, 1536, 512, 1, 1, 0, 0, 0},
      {"ht lin", 43008, 1536, 384, 1, 1, 2, 0, 1},
      {"rof qkv rotary", 49664, 1536, 512, 1, 1, 0, 0, 0, 0, 1},
      {"rof qkv rot only", 49664, 1536, 512, 1, 1, 0, 0, 0, 0, 2},
      {"rof qkv rscale only", 49664, 1536, 512, 1, 1, 0, 0, 0, 0, 3},
      {"rof qkv plain 49664", 49664, 1536, 512, 1, 1, 0, 0, 0, 0, 0},
      {"spread small", 4096 + 64, 512, 256, 1, 1, 0, 1, 1, 1},
      {"spread tdf L0 gemm1", 67584, 384, 3072, 48, 256, 1, 0, 0, 1},
      {"spread tdf L0 gemm2", 67584, 3072, 384, 48, 256, 1, 1, 0, 1},
  };
  for (int i = first; i < (int)shapes.size() && i <= last; ++i) run_shape(shapes[i], abl, 5);
  return 0;
}
