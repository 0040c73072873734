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

// ---- a pool of songs (asx_ht_demix_batch_dev / asx_hd_demix_batch_dev) -------------------------------------------------
// One global segment list, song-major; inside a song the order of its own ApplyPlan.  `shifts[song * nsh + si]` is that song's
// shift si with `first` moved into the global list (what the fold needs); stride / segment / max_shift are the same for every
// song of a call.
struct ApplyPoolSong {
  int64_t N;
  const int64_t *offsets;   // `shifts` draws of this song (unused when shifts == 0)
};
struct ApplyPoolPlan {
  int64_t stride = 0, segment = 0, max_shift = 0;
  int nsh = 1;                            // shift passes per song: max(shifts, 1)
  std::vector<int> song;                  // per segment: its song
  std::vector<int64_t> starts, clen;      // per segment, as ApplyPlan
  std::vector<ApplyShift> shifts;         // [n_songs * nsh]
};

// false (and `err`, naming the song) when the plan of any one song is rejected: the caller then enqueues nothing.
static inline bool apply_pool_build(const ApplyPoolSong *songs, int n_songs, int64_t segment, int64_t samplerate, int32_t shifts,
                                    double overlap, bool centered, ApplyPoolPlan &pp, std::string &err) {
  pp = ApplyPoolPlan();
  pp.nsh = shifts > 0 ? shifts : 1;
  pp.segment = segment;
  ApplyPlan p;
  for (int i = 0; i < n_songs; ++i) {
    std::string why;
    if (songs[i].N < 2) why = "n_samples must be >= 2";   // as the single-song entry points: the unbiased std needs two samples
    else if (shifts > 0 && !songs[i].offsets) why = "shifts > 0 needs the offsets array";
    else apply_plan_build(songs[i].N, segment, samplerate, shifts, songs[i].offsets, overlap, centered, p, why);
    if (!why.empty()) {
      err = "song " + std::to_string(i) + ": " + why;
      return false;
    }
    pp.stride = p.stride;
    pp.max_shift = p.max_shift;
    const int base = (int)pp.starts.size();
    for (ApplyShift sh : p.shifts) {
      sh.first += base;
      pp.shifts.push_back(sh);
    }
    pp.starts.insert(pp.starts.end(), p.starts.begin(), p.starts.end());
    pp.clen.insert(pp.clen.end(), p.clen.begin(), p.clen.end());
    pp.song.insert(pp.song.end(), p.starts.size(), i);
  }
  return true;
}
