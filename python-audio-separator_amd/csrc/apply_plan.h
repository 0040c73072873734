// The chunk plan of Demucs' apply_model (apply.py:195-260) on the host (no HIP): which chunk-forwards one call runs, in the
// reference's order -- shift 0's chunks, shift 1's chunks, ... -- for both generations.  Included by engine_ht.h and, for the
// host test, by tests/host/apply_plan_host.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

struct ApplyShift {
  int64_t offset, VL;
  int first, nk;          // range inside the global chunk list
};
struct ApplyPlan {
  int64_t stride, segment, max_shift;
  std::vector<ApplyShift> shifts;
  std::vector<int64_t> starts, clen;   // per chunk: song index of model-input sample 0, the chunk's own length
};

// offsets: `shifts` draws of random.randint(0, samplerate / 2) made by the caller (apply.py:209); shifts == 0 is the plain
// split path.  centered: the model runs a full segment with the chunk centred inside it (v4, htdemucs.py use_train_segment), so
// starts[k] moves back by the front padding; otherwise the chunk itself is the model input (v3).  false: `err` says why.
static inline bool apply_plan_build(int64_t N, int64_t segment, int64_t samplerate, int32_t shifts, const int64_t *offsets, double overlap,
                                    bool centered, ApplyPlan &p, std::string &err) {
  char msg[128];
  p.segment = segment;
  p.stride = (int64_t)((1.0 - overlap) * (double)segment);   // int((1 - overlap) * segment), apply.py:220
  if (!(p.stride >= 1 && p.stride <= segment)) {
    snprintf(msg, sizeof(msg), "overlap %g gives a bad stride", overlap);
    err = msg;
    return false;
  }
  p.max_shift = shifts > 0 ? samplerate / 2 : 0;
  p.shifts.clear();
  p.starts.clear();
  p.clen.clear();
  const int nsh = shifts > 0 ? shifts : 1;
  for (int si = 0; si < nsh; ++si) {
    ApplyShift sh;
    sh.offset = shifts > 0 ? offsets[si] : 0;
    if (!(sh.offset >= 0 && sh.offset <= p.max_shift)) {
      snprintf(msg, sizeof(msg), "shift offset %lld outside [0, %lld]", (long long)sh.offset, (long long)p.max_shift);
      err = msg;
      return false;
    }
    // view = padded_mix[offset : offset + N + max_shift - offset]; padded index q <-> song index q - max_shift
    sh.VL = N + p.max_shift - sh.offset;
    sh.first = (int)p.starts.size();
    for (int64_t off = 0; off < sh.VL; off += p.stride) {
      const int64_t clen = std::min(sh.VL - off, segment);
      p.starts.push_back(sh.offset + off - (centered ? (segment - clen) / 2 : 0) - p.max_shift);
      p.clen.push_back(clen);
    }
    sh.nk = (int)p.starts.size() - sh.first;
    p.shifts.push_back(sh);
  }
  return true;
}
