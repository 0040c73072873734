// Host driver of csrc/apply_plan.h (tests/test_host_apply_plan.py).
//   apply_plan_host <N> <segment> <samplerate> <overlap> <centered 0|1> <shifts> [offset ...]
// prints "plan <stride> <max_shift> <segment>", one "shift <offset> <VL> <first> <nk>" per shift and one "chunk <start> <clen>"
// per chunk; a rejected plan prints "error <message>" and exits with 3.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../python-audio-separator_amd/csrc/apply_plan.h"

int main(int argc, char **argv) {
  if (argc < 7) return 1;
  const int shifts = atoi(argv[6]);
  if (argc != 7 + (shifts > 0 ? shifts : 0)) return 1;
  std::vector<int64_t> offsets;
  for (int i = 0; i < shifts; ++i) offsets.push_back(atoll(argv[7 + i]));
  ApplyPlan p;
  std::string err;
  if (!apply_plan_build(atoll(argv[1]), atoll(argv[2]), atoll(argv[3]), shifts, offsets.data(), strtod(argv[4], nullptr), atoi(argv[5]) != 0, p,
                        err)) {
    printf("error %s\n", err.c_str());
    return 3;
  }
  printf("plan %lld %lld %lld\n", (long long)p.stride, (long long)p.max_shift, (long long)p.segment);
  for (const ApplyShift &sh : p.shifts) printf("shift %lld %lld %d %d\n", (long long)sh.offset, (long long)sh.VL, sh.first, sh.nk);
  for (size_t k = 0; k < p.starts.size(); ++k) printf("chunk %lld %lld\n", (long long)p.starts[k], (long long)p.clen[k]);
  return 0;
}
