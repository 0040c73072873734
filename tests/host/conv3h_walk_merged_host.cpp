// Host program of tests/test_host_conv3h_walk_merged.py: csrc/conv3h_walk_plan.h with merged output slices (nob groups per walker), no GPU.
//   conv3h_walk_merged_host check nob B tilesT tilesF [B tilesT tilesF ...]
//     -> for both schedules: every (item, strip < tilesF, tile row) is taken exactly once per output slice by the workgroups the map
//        conv3h_walk_wg sends to the table's rows; the map is a bijection from the busy workgroups onto (row, output slice, strip in band);
//        nob = 1: the table equals the one planned without the argument, entry for entry.  One line per shape and schedule:
//        "shape mode B tilesT tilesF nob bw walkers longest busy groups"
//   conv3h_walk_merged_host bench
//     -> the three benchmark shapes (55 chunks, levels 1 to 3 of the HQ_3 geometry) as n x n launches and merged: wall steps per layer, busy
//        groups; exit status 1 unless level 1 <= 1368, level 2 <= 843, and 32 of 32 / 30 of 32 groups are busy
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <tuple>

#include "../../python-audio-separator_amd/csrc/conv3h_walk_plan.h"

struct Busy {
  int busy, groups;
};

// walks the table as the kernel does (row and output slice from conv3h_walk_wg, strip = band * bw + (wg >> 3) % bw) and counts every tile
static int cover(int B, int tilesT, int tilesF, int mode, int nob, Conv3hWalkPlan *out, Busy *busy) {
  const Conv3hWalkPlan p = conv3h_walk_plan(B, tilesT, tilesF, 1, mode, nob);
  std::vector<int32_t> tab;
  const int stride = conv3h_walk_table(p, tab);
  if (p.nob != nob || p.ngroups != (256 / p.bw) / nob || tab.size() != (size_t)p.ngroups * stride * 4) {
    printf("plan geometry\n");
    return 1;
  }
  std::vector<int> seen((size_t)nob * B * tilesF * tilesT, 0);
  std::set<std::tuple<int, int, int>> image;           // (row, ob, strip in band) of the busy workgroups
  std::set<std::pair<int, int>> groups;                 // busy (row, ob)
  int idle = 0;
  for (int wg = 0; wg < 256; ++wg) {
    int row = -2, ob = -2;
    conv3h_walk_wg(wg, p.bw, nob, row, ob);
    if (row < 0) {
      ++idle;
      continue;
    }
    const int si = (wg >> 3) % p.bw;
    if (row >= p.ngroups || ob < 0 || ob >= nob || !image.insert({row, ob, si}).second) {
      printf("map: workgroup %d -> row %d, slice %d, strip %d\n", wg, row, ob, si);
      return 1;
    }
    groups.insert({row, ob});
    const int32_t *r = &tab[(size_t)row * stride * 4];
    if (r[0] != p.steps(row) || r[1] != (int32_t)p.units[(size_t)row].size()) {
      printf("table header of row %d\n", row);
      return 1;
    }
    for (int u = 0; u < r[1]; ++u) {
      const int32_t *e = r + 4 * (1 + u);
      const int b = e[0], strip = e[1] * p.bw + si;
      if (b < 0 || b >= B || e[2] < 0 || e[3] < 1 || e[2] + e[3] > tilesT || e[1] < 0 || e[1] * p.bw >= tilesF) {
        printf("unit %d of row %d\n", u, row);
        return 1;
      }
      if (strip >= tilesF) continue;                   // a padding strip: never stored
      for (int t = e[2]; t < e[2] + e[3]; ++t) ++seen[(((size_t)ob * B + b) * tilesF + strip) * tilesT + t];
    }
    if (r[4 * (1 + r[1]) + 3] != (1 << 30)) {
      printf("closing unit of row %d\n", row);
      return 1;
    }
  }
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != 1) {
      printf("tile %zu taken %d times\n", i, seen[i]);
      return 1;
    }
  // onto: every (row, ob, strip in band) has its workgroup, and the idle workgroups are exactly the groups beyond walkers * nob
  if ((int)image.size() != p.ngroups * nob * p.bw || idle != 256 - p.ngroups * nob * p.bw) {
    printf("map: %zu busy workgroups, %d idle for %d walkers of %d groups of %d\n", image.size(), idle, p.ngroups, nob, p.bw);
    return 1;
  }
  if (busy) *busy = Busy{(int)groups.size(), 256 / p.bw};
  if (out) *out = p;
  return 0;
}

static int check(int nob, int B, int tilesT, int tilesF) {
  for (int mode = 0; mode < 2; ++mode) {
    Conv3hWalkPlan p;
    Busy busy{};
    if (cover(B, tilesT, tilesF, mode, nob, &p, &busy) != 0) return 1;
    if (nob == 1) {                                      // today's plan and table, entry for entry
      const Conv3hWalkPlan q = conv3h_walk_plan(B, tilesT, tilesF, 1, mode);
      std::vector<int32_t> tp, tq;
      const int sp = conv3h_walk_table(p, tp), sq = conv3h_walk_table(q, tq);
      if (p.bw != q.bw || p.tps != q.tps || p.ngroups != q.ngroups || sp != sq || tp != tq) {
        printf("nob = 1 differs from the plan without merged slices\n");
        return 1;
      }
      for (int wg = 0; wg < 256; ++wg) {               // and the map is the kernel's arithmetic one: XCD wg & 7, group (wg >> 3) / bw of it
        int row, ob;
        conv3h_walk_wg(wg, p.bw, 1, row, ob);
        if (ob != 0 || row != (wg & 7) * (32 / p.bw) + (wg >> 3) / p.bw) {
          printf("nob = 1: workgroup %d -> row %d\n", wg, row);
          return 1;
        }
      }
    }
    printf("shape %d %d %d %d %d %d %d %d %d %d\n", mode, B, tilesT, tilesF, nob, p.bw, p.ngroups, p.longest(), busy.busy, busy.groups);
  }
  return 0;
}

static int bench() {
  const int shapes[3][4] = {{55, 32, 48, 2}, {55, 16, 24, 3}, {55, 8, 12, 4}};   // B, tilesT, tilesF, n: levels 1, 2, 3
  const int bound[3] = {1368, 843, 1 << 30}, want_busy[3] = {32, 30, -1};
  int bad = 0;
  for (int l = 0; l < 3; ++l) {
    const int B = shapes[l][0], tT = shapes[l][1], tF = shapes[l][2], n = shapes[l][3];
    Conv3hWalkPlan one, merged;
    Busy b1{}, bm{};
    if (cover(B, tT, tF, 1, 1, &one, &b1) != 0 || cover(B, tT, tF, 1, n, &merged, &bm) != 0) return 1;
    const int today = n * n * one.longest(), now = n * merged.longest();
    printf("level %d: today %d x %d = %d wall steps per layer (bw %d); merged %d x %d = %d (bw %d, %d of %d groups busy)\n", l + 1, n * n, one.longest(), today, one.bw, n,
           merged.longest(), now, merged.bw, bm.busy, bm.groups);
    if (now > bound[l]) {
      printf("level %d: more than %d steps\n", l + 1, bound[l]);
      ++bad;
    }
    if (want_busy[l] >= 0 && (bm.busy != want_busy[l] || bm.groups != 32)) {
      printf("level %d: %d of %d groups busy, expected %d of 32\n", l + 1, bm.busy, bm.groups, want_busy[l]);
      ++bad;
    }
  }
  return bad ? 1 : 0;
}

int main(int argc, char **argv) {
  if (argc == 2 && strcmp(argv[1], "bench") == 0) return bench();
  if (argc < 6 || (argc - 3) % 3 != 0 || strcmp(argv[1], "check") != 0) {
    fprintf(stderr, "usage: conv3h_walk_merged_host check nob B tilesT tilesF [B tilesT tilesF ...] | bench\n");
    return 2;
  }
  const int nob = atoi(argv[2]);
  for (int i = 3; i + 2 < argc; i += 3)
    if (check(nob, atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2])) != 0) return 1;
  return 0;
}
