// The plan of the rational polyphase converter (asx_resample_rational) on the host (no HIP): the Kaiser low-pass for a pair of sample
// rates, the length rule, the coefficient table as the device reads it, the tile geometry of resample_rational_kernel and a scalar
// float64 evaluation of the definition.  Included by asx.hip and, for the host test, by tests/host/resample_plan_host.cpp.
//
// Definition.  g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g.  With the taps h[n], n = -half .. half, designed on the grid of
// rate L * sr_in,
//     y[m] = sum over 0 <= i < n_in with |m * M - i * L| <= half of x[i] * h[m * M - i * L],      0 <= m < n_out = ceil(n_in * L / M)
// -- zero history at both ends, zero delay, n_out as librosa's ceil(n * ratio).  Every index is int64.
//
// Design (float64; this project's own filter in the class soxr publishes for its "HQ" recipe: 20 bit, pass band to 0.913 of the lower Nyquist
// frequency).  G = max(L, M); in units of the grid's Nyquist frequency fpass = 0.913 / G, fstop = 1 / G, width = fstop - fpass,
// fc = (fpass + fstop) / 2.  Kaiser window for A = 125 dB: beta = 0.1102 (A - 8.7), N = ceil((A - 7.95) / (2.285 pi width) + 1) (what
// scipy.signal.kaiserord(125, width) returns), half = ceil((N - 1) / 2 / L) * L,
//     h[n] = fc sinc(fc n) I0(beta sqrt(1 - (n / half)^2)) / I0(beta),   scaled so that sum(h) == L.
// T = 2 half / L + 1 taps per output at most.
//
// Device table [T][L], float32, minor index r = m mod L (NOT the phase (m M) mod L: consecutive outputs then read consecutive
// coefficients).  With P = half / L, q = floor(m M / L) and p = (m M) mod L = ((m mod L) M) mod L,
//     y[m] = sum over t = 0 .. T - 1 of tab[t][m mod L] * x[q + P - t],     tab[t][r] = h[p(r) + (t - P) L]  (0 where that is past half),
// x read as 0 outside [0, n_in).  The device accumulates in float32 FMAs.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

constexpr double RESAMPLE_ATTEN_DB = 125.0;          // stop-band rejection / pass-band ripple of the Kaiser design
constexpr double RESAMPLE_PASSBAND = 0.913;          // pass-band edge over the lower Nyquist frequency
constexpr int64_t RESAMPLE_MAX_TABLE = (int64_t)1 << 20;   // floats of the coefficient table L * T a pair may need
constexpr int64_t RESAMPLE_MAX_N = (int64_t)1 << 40;       // samples per channel
constexpr int RESAMPLE_THREADS = 256;                // threads of a workgroup of resample_rational_kernel
constexpr int64_t RESAMPLE_MAX_LDS_FLOATS = 16384;   // staged input span + LDS-resident taps of one workgroup (64 KiB)
constexpr int64_t RESAMPLE_LDS_TAPS = 2048;          // tables of at most this many floats (L = 1, 2, 4 ...) are read from LDS

struct ResamplePlan {
  int64_t sr_in = 0, sr_out = 0;
  int64_t L = 0, M = 0;       // up / down factors
  int64_t N = 0;              // kaiserord's tap count
  int64_t half = 0, P = 0;    // half = P * L
  int64_t T = 0;              // taps per phase, 2 P + 1
  double beta = 0.0, fc = 0.0;
  // tile of the device kernel: J consecutive outputs per period (a multiple of L), K periods per workgroup; a workgroup owns the J * K consecutive
  // outputs from tile * J * K and stages span floats of the input
  int64_t J = 0, span = 0;
  int K = 0;
  bool taps_in_lds = false;
};

static inline int64_t resample_gcd(int64_t a, int64_t b) {
  while (b) {
    const int64_t t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// modified Bessel function of the first kind, order 0: the power series (every term positive; converged to the last bit long before 200 terms
// for the beta ~ 12.8 of the design)
static inline double resample_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < sum * 1e-18) break;
  }
  return sum;
}

// "" and the plan, or why the pair is refused
static inline std::string resample_plan_make(int64_t sr_in, int64_t sr_out, ResamplePlan &p) {
  p = ResamplePlan();
  if (sr_in < 1 || sr_out < 1 || sr_in > 100000000 || sr_out > 100000000)
    return "sample rates " + std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " Hz (1 .. 10^8 each)";
  if (sr_in == sr_out) return "the rates are equal (" + std::to_string(sr_in) + " Hz): nothing to convert";
  const int64_t g = resample_gcd(sr_in, sr_out);
  p.sr_in = sr_in;
  p.sr_out = sr_out;
  p.L = sr_out / g;
  p.M = sr_in / g;
  const double G = (double)(p.L > p.M ? p.L : p.M);
  const double fpass = RESAMPLE_PASSBAND / G, fstop = 1.0 / G, width = fstop - fpass;
  p.fc = 0.5 * (fpass + fstop);
  p.beta = 0.1102 * (RESAMPLE_ATTEN_DB - 8.7);
  const double numtaps = (RESAMPLE_ATTEN_DB - 7.95) / 2.285 / (M_PI * width) + 1.0;
  if (!(numtaps < 4e15)) return "the filter for " + std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " Hz is too long";
  p.N = (int64_t)std::ceil(numtaps);
  p.P = (p.N - 1 + 2 * p.L - 1) / (2 * p.L);   // ceil((N - 1) / 2 / L)
  p.half = p.P * p.L;
  p.T = 2 * p.P + 1;
  if (p.L * p.T > RESAMPLE_MAX_TABLE || p.L > RESAMPLE_MAX_TABLE || p.T > RESAMPLE_MAX_TABLE)
    return std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " Hz needs a coefficient table of " + std::to_string(p.L) + " x " +
           std::to_string(p.T) + " floats (L = " + std::to_string(p.L) + ", M = " + std::to_string(p.M) + "; at most 2^20 are built)";
  // the tile: K = 8 periods unless even one period of L outputs would not fit the LDS budget; J = the multiple of L up to 1024 that keeps most
  // lanes of the 256-thread passes busy (the largest such on ties) and fits
  p.taps_in_lds = p.L * p.T <= RESAMPLE_LDS_TAPS;
  const int64_t budget = RESAMPLE_MAX_LDS_FLOATS - (p.taps_in_lds ? p.L * p.T : 0);
  for (p.K = 8; p.K > 1 && p.K * p.M + p.T > budget; p.K /= 2) {}
  if (p.K * p.M + p.T > budget) return std::to_string(sr_in) + " -> " + std::to_string(sr_out) + " Hz: one period of the input does not fit a workgroup";
  double best = -1.0;
  for (int64_t kg = 1; kg * p.L <= (p.L > 1024 ? p.L : 1024); ++kg) {
    const int64_t J = kg * p.L;
    if (kg * p.K * p.M + p.T > budget) break;
    const int64_t passes = (J + RESAMPLE_THREADS - 1) / RESAMPLE_THREADS;
    const double eff = (double)J / (double)(passes * RESAMPLE_THREADS);
    if (eff >= best) {
      best = eff;
      p.J = J;
    }
  }
  p.span = (p.J / p.L) * p.K * p.M + p.T;
  return "";
}

// librosa's ceil(n_in * sr_out / sr_in)
static inline int64_t resample_plan_n_out(const ResamplePlan &p, int64_t n_in) { return (n_in * p.L + p.M - 1) / p.M; }

// "" or why a call of that length is refused
static inline std::string resample_plan_check_n(const ResamplePlan &p, int64_t n_in) {
  if (n_in < 1 || n_in > RESAMPLE_MAX_N) return "n_in = " + std::to_string(n_in) + " (1 .. 2^40)";
  const int64_t n_out = resample_plan_n_out(p, n_in);
  if (n_out > RESAMPLE_MAX_N) return "n_out = " + std::to_string(n_out) + " (at most 2^40)";
  if ((n_out + p.J * p.K - 1) / (p.J * p.K) > 2147483647) return "too many tiles for one launch";
  return "";
}

// the same for the writer-side form, whose n_out is the caller's (asx_resample_rational_stem): outputs at or past resample_plan_n_out follow from
// the definition and are exactly 0 from m = ceil(((n_in - 1) L + half + 1) / M) on, where the filter has left the input
static inline std::string resample_plan_check_stem(const ResamplePlan &p, int64_t n_in, int64_t n_out) {
  if (n_in < 1 || n_in > RESAMPLE_MAX_N) return "n_in = " + std::to_string(n_in) + " (1 .. 2^40)";
  if (n_out < 1 || n_out > RESAMPLE_MAX_N) return "n_out = " + std::to_string(n_out) + " (1 .. 2^40)";
  if ((n_out + p.J * p.K - 1) / (p.J * p.K) > 2147483647) return "n_out = " + std::to_string(n_out) + ": too many tiles for one launch";
  return "";
}

// h[n + half], n = -half .. half, float64
static inline void resample_plan_taps(const ResamplePlan &p, std::vector<double> &h) {
  h.assign((size_t)(2 * p.half + 1), 0.0);
  const double i0b = resample_i0(p.beta);
  double sum = 0.0;
  for (int64_t n = -p.half; n <= p.half; ++n) {
    const double a = p.fc * (double)n;
    const double sinc = n == 0 ? 1.0 : std::sin(M_PI * a) / (M_PI * a);
    const double r = (double)n / (double)p.half;
    const double w = resample_i0(p.beta * std::sqrt(std::fmax(0.0, 1.0 - r * r))) / i0b;
    h[(size_t)(n + p.half)] = p.fc * sinc * w;
    sum += h[(size_t)(n + p.half)];
  }
  const double scale = (double)p.L / sum;
  for (double &v : h) v *= scale;
}

// the device table [T][L] (see the head of this file), the taps rounded to float32
static inline void resample_plan_table(const ResamplePlan &p, const std::vector<double> &h, std::vector<float> &tab) {
  tab.assign((size_t)(p.T * p.L), 0.f);
  for (int64_t r = 0; r < p.L; ++r) {
    const int64_t ph = (r * p.M) % p.L;
    for (int64_t t = 0; t < p.T; ++t) {
      const int64_t n = ph + (t - p.P) * p.L;
      if (n >= -p.half && n <= p.half) tab[(size_t)(t * p.L + r)] = (float)h[(size_t)(n + p.half)];
    }
  }
}

// y[m] of the definition in float64 (h from resample_plan_taps)
static inline double resample_plan_evaluate(const ResamplePlan &p, const std::vector<double> &h, const double *x, int64_t n_in, int64_t m) {
  const int64_t c = m * p.M;
  // i from ceil((c - half) / L) to floor((c + half) / L), inside the input
  int64_t lo = c - p.half, hi = (c + p.half) / p.L;
  lo = lo <= 0 ? 0 : (lo + p.L - 1) / p.L;
  if (hi > n_in - 1) hi = n_in - 1;
  double acc = 0.0;
  for (int64_t i = lo; i <= hi; ++i) acc += x[i] * h[(size_t)(c - i * p.L + p.half)];
  return acc;
}
