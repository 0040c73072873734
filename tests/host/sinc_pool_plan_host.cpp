// Host driver of csrc/sinc_pool_plan.h (tests/test_host_sinc_pool_plan.py).
//   sinc_pool_plan_host <ratio> <mono_calls> {<n_in>:<n_out>:<channels>[:nox][:noy]} x jobs
// (the ratio as strtod reads it, so a hexadecimal float passes exactly; ":nox" / ":noy" give the job a null input / output; a first
// job argument "many=<count>" stands for <count> copies of the job 16:16:1; "nolist" passes a null list of one job) prints
// "plan <blocks> <max_channels>" and per job "job <n_gen> <blocks> <blk0>"; a rejected list prints "error <message>" and exits with 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../python-audio-separator_amd/csrc/sinc_pool_plan.h"

int main(int argc, char **argv) {
  if (argc < 3) return 1;
  const double ratio = strtod(argv[1], nullptr);
  const bool mono_calls = atoi(argv[2]) != 0;
  static const float dummy_x = 0.f;
  static float dummy_y = 0.f;
  std::vector<SincPlanJobIn> jobs;
  bool no_list = false;
  for (int a = 3; a < argc; ++a) {
    if (strcmp(argv[a], "nolist") == 0) {
      no_list = true;
      continue;
    }
    if (strncmp(argv[a], "many=", 5) == 0) {
      jobs.assign((size_t)atol(argv[a] + 5), SincPlanJobIn{&dummy_x, &dummy_y, 16, 16, 1});
      continue;
    }
    char *end = nullptr;
    SincPlanJobIn in{&dummy_x, &dummy_y, 0, 0, 0};
    in.n_in = strtoll(argv[a], &end, 10);
    if (*end != ':') return 1;
    in.n_out = strtoll(end + 1, &end, 10);
    if (*end != ':') return 1;
    in.channels = (int)strtol(end + 1, &end, 10);
    while (*end == ':') {
      if (strncmp(end, ":nox", 4) == 0) in.x = nullptr;
      else if (strncmp(end, ":noy", 4) == 0) in.y = nullptr;
      else return 1;
      end += 4;
    }
    if (*end != 0) return 1;
    jobs.push_back(in);
  }
  const int n_jobs = no_list ? 1 : (int)jobs.size();
  const std::string why = sinc_pool_check(no_list ? nullptr : jobs.data(), n_jobs, ratio);
  if (!why.empty()) {
    printf("error %s\n", why.c_str());
    return 3;
  }
  SincPoolPlan pp;
  sinc_pool_build(jobs.data(), n_jobs, ratio, mono_calls, pp);
  printf("plan %lld %d\n", (long long)pp.blocks, pp.max_channels);
  for (const SincPlanJob &p : pp.job) printf("job %lld %lld %lld\n", (long long)p.n_gen, (long long)p.blocks, (long long)p.blk0);
  return 0;
}
