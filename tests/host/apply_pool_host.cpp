// Host driver of the pool plan in csrc/apply_plan.h (tests/test_host_demucs_batch.py).
//   apply_pool_host <segment> <samplerate> <overlap> <centered 0|1> <shifts> <n_songs> then per song: <N> [offset ...]
// prints "pool <stride> <max_shift> <segment> <nsh>", one "shift <song> <offset> <VL> <first> <nk>" per (song, shift) and one
// "seg <song> <start> <clen>" per segment of the pooled list;
// a rejected pool prints "error <message>" and exits with 3.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../python-audio-separator_amd/csrc/apply_plan.h"

int main(int argc, char **argv) {
  if (argc < 7) return 1;
  const int shifts = atoi(argv[5]), n_songs = atoi(argv[6]);
  const int per = 1 + (shifts > 0 ? shifts : 0);
  if (argc != 7 + n_songs * per) return 1;
  std::vector<std::vector<int64_t>> offsets((size_t)n_songs);
  std::vector<ApplyPoolSong> songs;
  for (int i = 0; i < n_songs; ++i) {
    for (int k = 1; k < per; ++k) offsets[i].push_back(atoll(argv[7 + i * per + k]));
    songs.push_back(ApplyPoolSong{atoll(argv[7 + i * per]), offsets[i].data()});
  }
  ApplyPoolPlan pp;
  std::string err;
  if (!apply_pool_build(songs.data(), n_songs, atoll(argv[1]), atoll(argv[2]), shifts, strtod(argv[3], nullptr), atoi(argv[4]) != 0, pp, err)) {
    printf("error %s\n", err.c_str());
    return 3;
  }
  printf("pool %lld %lld %lld %d\n", (long long)pp.stride, (long long)pp.max_shift, (long long)pp.segment, pp.nsh);
  for (size_t i = 0; i < pp.shifts.size(); ++i)
    printf("shift %d %lld %lld %d %d\n", (int)(i / pp.nsh), (long long)pp.shifts[i].offset, (long long)pp.shifts[i].VL, pp.shifts[i].first,
           pp.shifts[i].nk);
  for (size_t k = 0; k < pp.starts.size(); ++k) printf("seg %d %lld %lld\n", pp.song[k], (long long)pp.starts[k], (long long)pp.clen[k]);
  return 0;
}
