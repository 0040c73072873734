// The block walk of conv3h_kernel (kernels_conv3h.h) as a table, planned on the host (no HIP): which (batch item, band of strips, range of tile
// rows) every group of workgroups takes, in which order.  Included by engine_mdx.h -- the workspace set-up builds and uploads the tables of a
// pass, conv_launch hands the kernel one -- by tools/proto_conv3h.hip and, for the host test, by tests/host/conv3h_walk_host.cpp.
//
// The grid is 256 persistent workgroups: XCD x = block id & 7 holds 32 of them (block id >> 3), cut into 32 / bw GROUPS of bw workgroups.  A
// group walks UNITS one after the other: unit {b, band, t0, tiles} is tile rows t0 .. t0 + tiles - 1 of the bw adjacent strips band * bw ..
// of batch item b, workgroup i of the group on strip band * bw + i (the strips walk T together, so the halo columns they share are re-read
// from that XCD's L2; strips past tilesF are all padding and only keep the walk in step).  A unit is tiles + 1 steps: one block of four input
// rows in front that feeds only the two halo rows of the first tile, then a block per tile.  The launch lasts as long as its longest list.
//
// Mode 0 is the arithmetic walk the kernel had before the table: XCD x takes the items (b, band) x, x + 8, ..., its 32 / bw groups one
// segment of tps = tilesT bw / 32 tile rows of each; bw from a cost that charges band padding, the extra step per segment and the round-up of
// items / 8.  Mode 1 (balanced) deals whole-T units to all 256 / bw groups while whole rounds remain and cuts the leftover items, laid end to
// end, into one equal share of tile rows per group (a share touches one item, or two or three where it crosses their ends), every piece on a
// multiple of `gran` tile rows -- what the kernel's block exponent allows: 1, the exponent of a block is a function of the block alone.  Of
// the three band widths it keeps the one with the shortest longest list (the wider one on a tie) and, with gran = 1, never returns a longer one than mode 0.
//
// Merged output slices (nob > 1; a layer of 48 nob channels, one launch per INPUT slice): the groups are dealt into WALKERS of nob groups, group k
// of a walker on output slice k, all nob on the same row of the table -- the same units in the same order at the same time, so one group fetches
// a line of x from memory and the others find it in a cache.  The plan is dealt to (256 / bw) / nob lists instead of 256 / bw; groups beyond
// walkers * nob (nob = 3: two of 32 at bw = 8) stay idle.  conv3h_walk_wg is the map workgroup -> (table row, output slice), shared with the
// kernel.  Mode 0 with nob > 1 deals whole planes round robin to the walkers (no segments of T: 32 / bw groups of an XCD are not a multiple
// of every nob); on a tie of the longest list the NARROWER band wins there: bw = 8 keeps the groups of a walker on one XCD for nob = 2 and 4.
// nob = 1 is the plan described above, entry for entry.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

struct Conv3hUnit {
  int32_t b, band, t0, tiles;
};

struct Conv3hWalkPlan {
  int bw = 32, tps = 0;                    // strips per band; mode 0's tile rows per segment (0 in a balanced plan)
  int ngroups = 8;                         // lists (rows of the table): 256 / bw, group g = XCD g / (32 / bw), segment g % (32 / bw); nob > 1: the walkers, (256 / bw) / nob
  int nob = 1;                             // output slices side by side: groups per walker
  std::vector<std::vector<Conv3hUnit>> units;   // [ngroups], in walk order
  int steps(int g) const {
    int n = 0;
    for (const Conv3hUnit &u : units[(size_t)g]) n += u.tiles + 1;
    return n;
  }
  int longest() const {
    int n = 0;
    for (int g = 0; g < ngroups; ++g) n = std::max(n, steps(g));
    return n;
  }
  int max_units() const {
    size_t n = 0;
    for (const auto &l : units) n = std::max(n, l.size());
    return (int)n;
  }
};

// the band width of the arithmetic walk: whole bands on the plane's width, charged for the extra block per segment of T and for how evenly the
// (b, band) items deal out over the 8 XCDs
static inline int conv3h_walk_bw0(int B, int tilesT, int tilesF) {
  int bw = 32;
  double best = 1e30;
  for (int cand : {32, 16, 8}) {
    if ((tilesT * cand) % 32 != 0) continue;
    const int tps = tilesT * cand / 32;
    const int bands = (tilesF + cand - 1) / cand, items = B * bands;
    const double cost = (double)(bands * cand) / tilesF * (tps + 1.0) / tps * (double)((items + 7) / 8) / (items / 8.0);
    if (cost < best - 1e-9) {
      best = cost;
      bw = cand;
    }
  }
  return best > 1e29 ? 32 : bw;            // (tilesT not divisible: one segment)
}

// the arithmetic walk on bands of bw strips (tilesT bw a multiple of 32, or bw = 32)
static inline Conv3hWalkPlan conv3h_walk_arith(int B, int tilesT, int tilesF, int bw) {
  Conv3hWalkPlan p;
  p.bw = (tilesT * bw) % 32 == 0 ? bw : 32;
  p.tps = tilesT * p.bw / 32;
  const int segs = 32 / p.bw, nbands = (tilesF + p.bw - 1) / p.bw, items = B * nbands;
  p.ngroups = 8 * segs;
  p.units.assign((size_t)p.ngroups, {});
  for (int x = 0; x < 8; ++x)
    for (int seg = 0; seg < segs; ++seg)
      for (int item = x; item < items; item += 8)
        p.units[(size_t)(x * segs + seg)].push_back({item / nbands, item % nbands, seg * p.tps, p.tps});
  return p;
}
static inline Conv3hWalkPlan conv3h_walk_plan0(int B, int tilesT, int tilesF) { return conv3h_walk_arith(B, tilesT, tilesF, conv3h_walk_bw0(B, tilesT, tilesF)); }

#if defined(__HIPCC__)
#define CONV3H_WALK_HD __host__ __device__
#else
#define CONV3H_WALK_HD
#endif
// Workgroup wg of the 256 -> row of the walk table (-1: the group is idle and leaves at once) and output slice ob; its strip inside the band
// is (wg >> 3) % bw whatever nob.  Where the 32 / bw groups of an XCD are a multiple of nob, the groups of a walker sit on ONE XCD (they share
// x through its L2): nob = 2 at bw <= 16, nob = 4 at bw = 8.  Otherwise walker = g / nob, ob = g % nob over the global group index g.
CONV3H_WALK_HD static inline void conv3h_walk_wg(int wg, int bw, int nob, int &row, int &ob) {
  const int gx = 32 / bw, x = wg & 7, seg = (wg >> 3) / bw;
  if (nob < 1) nob = 1;                    // (arguments that never heard of the field: 0)
  if (gx % nob == 0) {
    row = x * (gx / nob) + seg / nob;
    ob = seg % nob;
  } else {
    const int g = x * gx + seg;
    row = g / nob;
    ob = g % nob;
    if (row >= (8 * gx) / nob) row = -1;
  }
}

static inline Conv3hWalkPlan conv3h_walk_balanced(int B, int tilesT, int tilesF, int gran, int bw, int nob = 1) {
  Conv3hWalkPlan p;
  p.bw = bw;
  p.tps = 0;
  p.nob = nob;
  p.ngroups = (256 / bw) / nob;
  p.units.assign((size_t)p.ngroups, {});
  const int G = p.ngroups, nbands = (tilesF + bw - 1) / bw, items = B * nbands;
  const int rounds = items / G, left = items - rounds * G;
  for (int r = 0; r < rounds; ++r)
    for (int g = 0; g < G; ++g) {
      const int item = r * G + g;
      p.units[(size_t)g].push_back({item / nbands, item % nbands, 0, tilesT});
    }
  // the leftover items end to end: `left * tilesT` tile rows, group g takes rows g * share .. (g + 1) * share - 1 of that line; share is a
  // multiple of gran and so is tilesT rounded up (a piece starts on a multiple of gran inside its item, the item's last piece may be shorter)
  if (left > 0) {
    const int64_t tT = ((int64_t)(tilesT + gran - 1) / gran) * gran, total = (int64_t)left * tT;
    int64_t share = (total + G - 1) / G;
    share = (share + gran - 1) / gran * gran;
    for (int g = 0; g < G; ++g) {
      int64_t lo = (int64_t)g * share;
      const int64_t hi = std::min(total, lo + share);
      while (lo < hi) {
        const int64_t i = lo / tT, t0 = lo - i * tT, t1 = std::min<int64_t>(tT, t0 + (hi - lo));
        const int item = rounds * G + (int)i;
        if (t0 < tilesT) p.units[(size_t)g].push_back({item / nbands, item % nbands, (int)t0, (int)std::min<int64_t>(t1, tilesT) - (int)t0});
        lo += t1 - t0;
      }
    }
  }
  return p;
}

// nob > 1, mode 0: whole planes round robin, walker w takes the items (b, band) w, w + walkers, ...
static inline Conv3hWalkPlan conv3h_walk_dealt(int B, int tilesT, int tilesF, int bw, int nob) {
  Conv3hWalkPlan p;
  p.bw = bw;
  p.tps = tilesT;
  p.nob = nob;
  p.ngroups = (256 / bw) / nob;
  p.units.assign((size_t)p.ngroups, {});
  const int nbands = (tilesF + bw - 1) / bw, items = B * nbands;
  for (int item = 0; item < items; ++item) p.units[(size_t)(item % p.ngroups)].push_back({item / nbands, item % nbands, 0, tilesT});
  return p;
}

// mode 0: the arithmetic walk; mode 1: balanced.  gran: a unit may start on multiples of gran tile rows only (mode 1; >= 1).  nob: output
// slices side by side (1 .. 4)
static inline Conv3hWalkPlan conv3h_walk_plan(int B, int tilesT, int tilesF, int gran, int mode, int nob = 1) {
  if (nob > 1) {
    if (gran < 1) gran = 1;
    Conv3hWalkPlan best;
    int nbest = INT32_MAX;
    for (int bw : {32, 16, 8}) {
      Conv3hWalkPlan c = mode == 0 ? conv3h_walk_dealt(B, tilesT, tilesF, bw, nob) : conv3h_walk_balanced(B, tilesT, tilesF, gran, bw, nob);
      const int n = c.longest();
      if (n <= nbest) {
        nbest = n;
        best = std::move(c);
      }
    }
    return best;
  }
  Conv3hWalkPlan best = conv3h_walk_plan0(B, tilesT, tilesF);
  if (mode == 0) return best;
  if (gran < 1) gran = 1;
  // the arithmetic walk is a candidate where its segments start on allowed rows
  int nbest = best.tps % gran == 0 || best.tps == tilesT ? best.longest() : INT32_MAX;
  for (int bw : {32, 16, 8}) {
    Conv3hWalkPlan c = conv3h_walk_balanced(B, tilesT, tilesF, gran, bw);
    const int n = c.longest();
    if (n < nbest) {
      nbest = n;
      best = std::move(c);
    }
  }
  return best;
}

// The table the kernel reads, 16-byte entries: row g (group g; nob > 1: walker g) at g * stride entries = {steps of the group, units, 0, 0}, its units {b, band, t0,
// tiles}, then one closing unit of 2^30 tile rows that the walk never leaves (the producers look four blocks ahead of the last step).
// Returns stride.
static inline int conv3h_walk_table(const Conv3hWalkPlan &p, std::vector<int32_t> &tab) {
  const int stride = p.max_units() + 2;
  tab.assign((size_t)p.ngroups * stride * 4, 0);
  for (int g = 0; g < p.ngroups; ++g) {
    int32_t *row = &tab[(size_t)g * stride * 4];
    const auto &l = p.units[(size_t)g];
    row[0] = p.steps(g);
    row[1] = (int32_t)l.size();
    for (size_t u = 0; u <= l.size(); ++u) {
      const Conv3hUnit un = u < l.size() ? l[u] : Conv3hUnit{0, 0, 0, 1 << 30};
      int32_t *e = row + 4 * (1 + u);
      e[0] = un.b;
      e[1] = un.band;
      e[2] = un.t0;
      e[3] = un.tiles;
    }
  }
  return stride;
}
