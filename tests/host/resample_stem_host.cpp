// Host driver of csrc/resample_plan.h for the writer-side form of the converter (tests/test_host_output_rate.py).
//   resample_stem_host plan <sr_in> <sr_out>                  "plan <L> <M> <half> <T> <J> <K> <span> <taps_in_lds>"; a refused pair prints
//                                                             "error <message>" and exits with 3
//   resample_stem_host check <sr_in> <sr_out> <n_in> <n_out>  "ok", or "error <message>" and exit code 3 (resample_plan_check_stem)
//   resample_stem_host eval <sr_in> <sr_out> <n_in> <n_out>   resample_plan_evaluate() for 0 <= m < n_out -- n_out is free -- on the n_in raw float64
//                                                             samples read from stdin; raw float64 on stdout
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
    printf("plan %lld %lld %lld %lld %lld %d %lld %d\n", (long long)p.L, (long long)p.M, (long long)p.half, (long long)p.T, (long long)p.J, p.K,
           (long long)p.span, (int)p.taps_in_lds);
    return 0;
  }
  if (argc != 6) return 1;
  const long long n_in = atoll(argv[4]), n_out = atoll(argv[5]);
  const std::string bad = resample_plan_check_stem(p, n_in, n_out);
  if (!strcmp(mode, "check")) {
    if (bad.empty()) {
      printf("ok\n");
      return 0;
    }
    printf("error %s\n", bad.c_str());
    return 3;
  }
  if (strcmp(mode, "eval") || !bad.empty() || n_in > 1 << 24 || n_out > 1 << 24) return 1;
  std::vector<double> x((size_t)n_in), y((size_t)n_out), h;
  if (fread(x.data(), sizeof(double), x.size(), stdin) != x.size()) return 1;
  resample_plan_taps(p, h);
  for (long long m = 0; m < n_out; ++m) y[(size_t)m] = resample_plan_evaluate(p, h, x.data(), n_in, m);
  return fwrite(y.data(), sizeof(double), y.size(), stdout) == y.size() ? 0 : 1;
}
