// How many items one launch takes when a list runs in batches (host only, no HIP).  Included by engine_core.h and by the
// host-only plan headers that walk a list the same way.
#pragma once

// Items per launch when nk >= 1 items run in the fewest batches of at most maxB: evened out, so that no short tail batch runs
// alone (85 items at maxB 32: 29 + 29 + 27, not 32 + 32 + 21).  The callers walk `for (j = 0; j < nk; j += per)`.
static inline int even_batches(int nk, int maxB) {
  const int nbatch = (nk + maxB - 1) / maxB;
  return (nk + nbatch - 1) / nbatch;
}
