// Host driver of csrc/vr_pool_plan.h (tests/test_host_vr_batch.py).
//   vr_pool_host <window_size> <offset> <max_batch> <high_end 0|1> <top_crop_stop> <pre_filter_start> <pre_filter_stop>
//                <n_bands> {<sr> <hl> <n_fft>} x n_bands  {<n_samples> | null} x songs
// prints "plan <roi> <he_rows> <frames> <per_pass plain> <per_pass tta>", one "song <T> <n_out> <patches> <frame0>" per song,
// the flat lists as "patch <plain|tta> <song> <k>", and per pass "pass <plain|tta> <j0> <B>" followed by its
// "run <song> <k0> <slot0> <count>" lines; a rejected pool prints "error <message>" and exits with 3.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../python-audio-separator_amd/csrc/vr_pool_plan.h"

int main(int argc, char **argv) {
  if (argc < 9) return 1;
  VrPlanCfg c;
  c.window_size = atoi(argv[1]);
  c.offset = atoi(argv[2]);
  c.max_batch = atoi(argv[3]);
  const bool high_end = atoi(argv[4]) != 0;
  c.top_crop_stop = atoi(argv[5]);
  c.pre_filter_start = atoi(argv[6]);
  c.pre_filter_stop = atoi(argv[7]);
  const int nb = atoi(argv[8]);
  if (nb < 1 || argc < 9 + 3 * nb) return 1;
  std::vector<int> sr(nb);
  c.band.resize(nb);
  for (int d = 0; d < nb; ++d) {
    sr[d] = atoi(argv[9 + 3 * d]);
    c.band[d].hl = atoi(argv[10 + 3 * d]);
    if (d == nb - 1) c.top_n_fft = atoi(argv[11 + 3 * d]);
  }
  for (int d = 0; d + 1 < nb; ++d) vr_plan_ratio(sr[d + 1], sr[d], c.band[d].up, c.band[d].down);
  std::vector<VrPoolSongIn> songs;
  for (int i = 9 + 3 * nb; i < argc; ++i) songs.push_back(VrPoolSongIn{strcmp(argv[i], "null") != 0, atoll(argv[i])});
  VrPoolPlan pp;
  std::string err;
  if (!vr_pool_build(c, songs.data(), (int)songs.size(), high_end, pp, err)) {
    printf("error %s\n", err.c_str());
    return 3;
  }
  const std::vector<VrPoolPatch> *lists[2] = {&pp.plain, &pp.tta};
  const char *names[2] = {"plain", "tta"};
  int per[2];
  for (int l = 0; l < 2; ++l) per[l] = lists[l]->empty() ? 0 : vr_pool_per_pass(c, (int)lists[l]->size());
  printf("plan %d %d %lld %d %d\n", pp.roi, pp.he_rows, (long long)pp.frames, per[0], per[1]);
  for (const VrPoolSong &s : pp.song) printf("song %d %lld %d %lld\n", s.T, (long long)s.n_out, s.patches, (long long)s.frame0);
  std::vector<VrPoolRun> runs;
  for (int l = 0; l < 2; ++l) {
    for (const VrPoolPatch &p : *lists[l]) printf("patch %s %d %d\n", names[l], p.song, p.k);
    const int total = (int)lists[l]->size();
    for (int j0 = 0; j0 < total; j0 += per[l]) {
      const int B = std::min(per[l], total - j0);
      printf("pass %s %d %d\n", names[l], j0, B);
      vr_pool_runs(*lists[l], j0, B, runs);
      for (const VrPoolRun &r : runs) printf("run %d %d %d %d\n", r.song, r.k0, r.slot0, r.count);
    }
  }
  return 0;
}
