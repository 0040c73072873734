// Host driver of csrc/ens_pool_plan.h (tests/test_host_ensemble_batch.py).
//   ens_pool_host <algorithm> <silent_below> {<n>:<peak_after>[,<n>:<peak_after>]... | none} x jobs
// (numbers as strtod reads them, so hexadecimal floats pass exactly; "none" is a job without contributors) prints
// "plan <wave_blocks> <frames> <fold_blocks> <picks>" and per job
// "job <live> <n_max> <T> <n_out> <wave_blocks> <wave_blk0> <frames> <frame0> <fold_blocks> <fold_blk0> <pick> <who>..."; a rejected
// list prints "error <message>" and exits with 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../python-audio-separator_amd/csrc/ens_pool_plan.h"

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  const int alg = atoi(argv[1]);
  const double silent_below = strtod(argv[2], nullptr);
  std::vector<EnsPlanJobIn> jobs;
  for (int a = 3; a < argc; ++a) {
    EnsPlanJobIn in;
    if (strcmp(argv[a], "none") != 0) {
      const char *p = argv[a];
      while (*p) {
        char *end = nullptr;
        const long long n = strtoll(p, &end, 10);
        if (*end != ':') return 1;
        const float peak = (float)strtod(end + 1, &end);
        if (in.k < ENS_PLAN_MAX_K) {
          in.n[in.k] = n;
          in.peak_after[in.k] = peak;
        }
        ++in.k;   // (beyond ENS_PLAN_MAX_K: counted, for the check to refuse)
        p = *end == ',' ? end + 1 : end;
        if (*end != ',' && *end != 0) return 1;
      }
    }
    jobs.push_back(in);
  }
  const std::string why = ens_pool_check(jobs.data(), (int)jobs.size(), alg);
  if (!why.empty()) {
    printf("error %s\n", why.c_str());
    return 3;
  }
  EnsPoolPlan pp;
  ens_pool_build(jobs.data(), (int)jobs.size(), alg, silent_below, pp);
  printf("plan %lld %lld %lld %d\n", (long long)pp.wave_blocks, (long long)pp.frames, (long long)pp.fold_blocks, pp.picks);
  for (const EnsPlanJob &p : pp.job) {
    printf("job %d %lld %d %lld %lld %lld %lld %lld %lld %lld %d", p.live, (long long)p.n_max, p.T, (long long)p.n_out, (long long)p.wave_blocks,
           (long long)p.wave_blk0, (long long)p.frames, (long long)p.frame0, (long long)p.fold_blocks, (long long)p.fold_blk0, (int)p.pick);
    for (int c = 0; c < p.live; ++c) printf(" %d", p.who[c]);
    printf("\n");
  }
  return 0;
}
