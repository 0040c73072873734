// Host driver of csrc/resample_plan.h (tests/test_host_resample_plan.py).
//   resample_plan_host plan <sr_in> <sr_out> [<n_in>]...   "plan <L> <M> <N> <half> <T> <J> <K> <span> <taps_in_lds>", then "n_out <n_in> <n_out>" per
//                                                          length; a refused pair prints "error <message>" and exits with 3
//   resample_plan_host taps <sr_in> <sr_out>               the 2 half + 1 taps, raw float64, on stdout
//   resample_plan_host table <sr_in> <sr_out>              the device table [T][L], raw float32
//   resample_plan_host sine <sr_in> <sr_out> <f_hz> <phi> <n_in> <m_lo> <m_hi>
//                                                          evaluate() for m_lo <= m < m_hi on x[i] = sin(2 pi f i / sr_in + phi), raw float64
//   resample_plan_host layout <sr_in> <sr_out> <n_in>      max over all outputs of |evaluate() - the table form of the sum in float64| on a fixed
//                                                          pseudo-random input (both use float32-rounded taps), as "%.17g"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../python-audio-separator_amd/csrc/resample_plan.h"

int main(int argc, char **argv) {
  if (argc < 4) return 1;
  const char *mode = argv[1];
  ResamplePlan p;
  const std::string why = resample_plan_make(atoll(argv[2]), atoll(argv[3]), p);
  if (!why.empty()) {
    printf("error %s\n", why.c_str());
    return 3;
  }
  if (!strcmp(mode, "plan")) {
    printf("plan %lld %lld %lld %lld %lld %lld %d %lld %d\n", (long long)p.L, (long long)p.M, (long long)p.N, (long long)p.half, (long long)p.T,
           (long long)p.J, p.K, (long long)p.span, (int)p.taps_in_lds);
    for (int a = 4; a < argc; ++a) {
      const long long n = atoll(argv[a]);
      const std::string bad = resample_plan_check_n(p, n);
      if (!bad.empty()) {
        printf("error %s\n", bad.c_str());
        return 3;
      }
      printf("n_out %lld %lld\n", n, (long long)resample_plan_n_out(p, n));
    }
    return 0;
  }
  std::vector<double> h;
  resample_plan_taps(p, h);
  if (!strcmp(mode, "taps")) return fwrite(h.data(), sizeof(double), h.size(), stdout) == h.size() ? 0 : 1;
  if (!strcmp(mode, "table")) {
    std::vector<float> tab;
    resample_plan_table(p, h, tab);
    return fwrite(tab.data(), sizeof(float), tab.size(), stdout) == tab.size() ? 0 : 1;
  }
  if (!strcmp(mode, "sine") && argc == 9) {
    const double f = strtod(argv[4], nullptr), phi = strtod(argv[5], nullptr);
    const long long n_in = atoll(argv[6]), m_lo = atoll(argv[7]), m_hi = atoll(argv[8]);
    if (n_in < 1 || m_lo < 0 || m_hi < m_lo || m_hi > resample_plan_n_out(p, n_in)) return 1;
    std::vector<double> x((size_t)n_in), y((size_t)(m_hi - m_lo));
    for (long long i = 0; i < n_in; ++i) x[(size_t)i] = std::sin(2.0 * M_PI * f * (double)i / (double)p.sr_in + phi);
    for (long long m = m_lo; m < m_hi; ++m) y[(size_t)(m - m_lo)] = resample_plan_evaluate(p, h, x.data(), n_in, m);
    return fwrite(y.data(), sizeof(double), y.size(), stdout) == y.size() ? 0 : 1;
  }
  if (!strcmp(mode, "layout") && argc == 5) {
    const long long n_in = atoll(argv[4]);
    if (n_in < 1) return 1;
    std::vector<float> tab;
    resample_plan_table(p, h, tab);
    for (double &v : h) v = (double)(float)v;
    std::vector<double> x((size_t)n_in);
    unsigned long long s = 0x9E3779B97F4A7C15ull;
    for (double &v : x) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      v = (double)(long long)(s >> 11) / 4503599627370496.0 - 1.0;   // [-1, 1)
    }
    double worst = 0.0;
    const long long n_out = resample_plan_n_out(p, n_in);
    for (long long m = 0; m < n_out; ++m) {
      const long long q = m * p.M / p.L;
      double acc = 0.0;
      for (long long t = 0; t < p.T; ++t) {
        const long long i = q + p.P - t;
        if (i >= 0 && i < n_in) acc += (double)tab[(size_t)(t * p.L + m % p.L)] * x[(size_t)i];
      }
      worst = std::fmax(worst, std::fabs(acc - resample_plan_evaluate(p, h, x.data(), n_in, m)));
    }
    printf("%.17g\n", worst);
    return 0;
  }
  return 1;
}
