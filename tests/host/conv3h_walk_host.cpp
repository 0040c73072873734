// Host program of tests/test_host_conv3h_walk.py: csrc/conv3h_walk_plan.h, the planner of conv3h_kernel's walk table, with no GPU.
//   conv3h_walk_host plan gran mode B tilesT tilesF [B tilesT tilesF ...]
//     -> per shape "plan B tilesT tilesF bw tps ngroups longest stride", then one line "g b band t0 tiles" per unit in walk order, then "table ok" after the device
//        table (conv3h_walk_table) has been read back against the lists: header, units, closing unit, nothing outside a row
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../python-audio-separator_amd/csrc/conv3h_walk_plan.h"

static int one(int B, int tilesT, int tilesF, int gran, int mode) {
  const Conv3hWalkPlan p = conv3h_walk_plan(B, tilesT, tilesF, gran, mode);
  std::vector<int32_t> tab;
  const int stride = conv3h_walk_table(p, tab);
  printf("plan %d %d %d %d %d %d %d %d\n", B, tilesT, tilesF, p.bw, p.tps, p.ngroups, p.longest(), stride);
  for (int g = 0; g < p.ngroups; ++g)
    for (const Conv3hUnit &u : p.units[(size_t)g]) printf("%d %d %d %d %d\n", g, u.b, u.band, u.t0, u.tiles);
  if (tab.size() != (size_t)p.ngroups * stride * 4 || p.ngroups * p.bw != 256) {
    printf("table size\n");
    return 1;
  }
  for (int g = 0; g < p.ngroups; ++g) {
    const int32_t *row = &tab[(size_t)g * stride * 4];
    const auto &l = p.units[(size_t)g];
    if (row[0] != p.steps(g) || row[1] != (int32_t)l.size() || (int)l.size() + 2 > stride) {
      printf("table header of group %d\n", g);
      return 1;
    }
    for (size_t u = 0; u < l.size(); ++u) {
      const int32_t *e = row + 4 * (1 + u);
      if (e[0] != l[u].b || e[1] != l[u].band || e[2] != l[u].t0 || e[3] != l[u].tiles) {
        printf("table unit %d of group %d\n", (int)u, g);
        return 1;
      }
    }
    if (row[4 * (1 + l.size()) + 3] != (1 << 30)) {
      printf("closing unit of group %d\n", g);
      return 1;
    }
  }
  printf("table ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 7 || (argc - 4) % 3 != 0 || strcmp(argv[1], "plan") != 0) {
    fprintf(stderr, "usage: conv3h_walk_host plan gran mode B tilesT tilesF [B tilesT tilesF ...]\n");
    return 2;
  }
  const int gran = atoi(argv[2]), mode = atoi(argv[3]);
  for (int i = 4; i + 2 < argc; i += 3)
    if (one(atoi(argv[i]), atoi(argv[i + 1]), atoi(argv[i + 2]), gran, mode) != 0) return 1;
  return 0;
}
