// The plan of a VR separation on the host (no HIP): frames and output length of one song (VRSeparator.loading_mix,
// vr_separator.py:255-291, and make_padding, spec_utils.py:86-96), and for a pool of songs (asx_vr_separate_batch_dev) every
// song's share of the pooled slabs plus the flat patch lists the shared net passes walk.  Included by engine_vr.h and, for the
// host test, by tests/host/vr_pool_host.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "batching.h"

// what the plan needs of a committed net: per band (index 0 = band 1) the hop and the rational ratio up / down that brings band
// d + 1's wave to band d's rate (unused for the top band); the patch geometry; the rows high_end_process mirrors
struct VrPlanBand {
  int64_t up = 1, down = 1;
  int hl = 1;
};
struct VrPlanCfg {
  std::vector<VrPlanBand> band;
  int window_size = 0, offset = 0, max_batch = 0;
  int top_n_fft = 0, top_crop_stop = 0, pre_filter_start = 0, pre_filter_stop = 0;
};

// target_sr / orig_sr in lowest terms, as scipy.signal.resample_poly reduces it
static inline void vr_plan_ratio(int orig_sr, int target_sr, int64_t &up, int64_t &down) {
  int a = target_sr, b = orig_sr;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  up = target_sr / a;
  down = orig_sr / a;
}

static inline int64_t vr_plan_resampled_len(int64_t up, int64_t down, int64_t n_in) {   // ceil(n * up / down)
  const int64_t t = n_in * up;
  return t / down + (t % down ? 1 : 0);
}

// frames of the combined spectrogram (the shortest band decides) and output length for n samples at the top band's rate
static inline void vr_plan_frames(const VrPlanCfg &c, int64_t n_samples, int *T, int64_t *n_out) {
  const int NB = (int)c.band.size();
  int64_t len = n_samples;
  int Tmin = 0;
  for (int d = NB - 1; d >= 0; --d) {
    if (d < NB - 1) len = vr_plan_resampled_len(c.band[d].up, c.band[d].down, len);
    const int t = (int)(1 + len / c.band[d].hl);
    Tmin = d == NB - 1 ? t : std::min(Tmin, t);
  }
  *T = Tmin;
  *n_out = (int64_t)c.band[NB - 1].hl * (Tmin - 1);
}

// make_padding's roi (spec_utils.py:86-96).  Its `roi == 0 -> window_size` branch is kept for the arithmetic's sake only: the engine
// refuses window_size <= 2 * offset when the net is committed, so no kernel ever runs with it.
static inline int vr_plan_roi(const VrPlanCfg &c) {
  const int roi = c.window_size - 2 * c.offset;
  return roi == 0 ? c.window_size : roi;
}

// input_high_end_h (vr_separator.py:287): bins above the top band's crop + the pre-filter ramp
static inline int vr_plan_high_end_rows(const VrPlanCfg &c) { return (c.top_n_fft / 2 - c.top_crop_stop) + (c.pre_filter_stop - c.pre_filter_start); }

// "" when a song of n_samples can be separated, else the reason (the text of the single-song call's refusal)
static inline std::string vr_plan_check(const VrPlanCfg &c, int64_t n_samples, bool high_end, int T) {
  if (T < 2) return "input too short: " + std::to_string(T) + " frames";
  if (high_end) {
    const int h = vr_plan_high_end_rows(c);
    if (!(h > 0 && h <= c.top_n_fft / 2 && c.pre_filter_start - 10 - h >= 0))
      return "high_end_process: " + std::to_string(h) + " mirrored rows do not fit below pre_filter_start - 10";
    const int t_top = (int)(1 + n_samples / c.band.back().hl);
    if (t_top != T)
      return "high_end_process needs the top band's frame count (" + std::to_string(t_top) + ") to equal the combined spectrogram's (" +
             std::to_string(T) + ")";
  }
  return "";
}

// ---- a pool of songs ---------------------------------------------------------------------------------------------------
// Song i owns frames [frame0, frame0 + T) of every pooled slab, songs laid end to end: its spectrogram is the 2 * T * (bins + 1)
// complex values from 2 * frame0 * (bins + 1) of the X slab, its mask the same range of floats of the M slab, its mirrored high
// end the 2 * T * he_rows complex values from 2 * frame0 * he_rows of the HE slab, its per-frame minima and merge weights
// [frame0, frame0 + T) of theirs; its peak is slot i.
struct VrPoolSongIn {
  bool has_wave;
  int64_t n_samples;
};
struct VrPoolSong {
  int T = 0, patches = 0;   // patches = T / roi + 1 in the plain pass, one more in the TTA pass
  int64_t n_out = 0, frame0 = 0;
};
struct VrPoolPatch {
  int song, k;
};
// a run of consecutive patches of one song inside one pass: patches [k0, k0 + count) sit in slots [slot0, slot0 + count)
struct VrPoolRun {
  int song, k0, slot0, count;
};
struct VrPoolPlan {
  int roi = 0, he_rows = 0;        // he_rows: 0 unless high_end_process
  int64_t frames = 0;              // of the whole pool
  std::vector<VrPoolSong> song;
  std::vector<VrPoolPatch> plain, tta;   // song-major, a song's patches in order
};

// false (and `err`, naming the song) when any one song is rejected: the caller then enqueues nothing.
static inline bool vr_pool_build(const VrPlanCfg &c, const VrPoolSongIn *songs, int n_songs, bool high_end, VrPoolPlan &pp, std::string &err) {
  pp = VrPoolPlan();
  pp.roi = vr_plan_roi(c);
  pp.he_rows = high_end ? vr_plan_high_end_rows(c) : 0;
  pp.song.resize((size_t)std::max(n_songs, 0));
  for (int i = 0; i < n_songs; ++i) {
    std::string why;
    VrPoolSong &ps = pp.song[i];
    if (!songs[i].has_wave) why = "null wave pointer";
    else if (songs[i].n_samples < 1) why = "n_samples must be positive";
    else {
      vr_plan_frames(c, songs[i].n_samples, &ps.T, &ps.n_out);
      why = vr_plan_check(c, songs[i].n_samples, high_end, ps.T);
    }
    if (!why.empty()) {
      err = "song " + std::to_string(i) + ": " + why;
      return false;
    }
    ps.patches = ps.T / pp.roi + 1;
    ps.frame0 = pp.frames;
    pp.frames += ps.T;
    for (int k = 0; k < ps.patches; ++k) pp.plain.push_back(VrPoolPatch{i, k});
    for (int k = 0; k < ps.patches + 1; ++k) pp.tta.push_back(VrPoolPatch{i, k});
  }
  return true;
}

// patches per net pass for a list of `total` patches
static inline int vr_pool_per_pass(const VrPlanCfg &c, int total) { return even_batches(total, c.max_batch > 0 ? c.max_batch : 4); }

// the runs of the pass that takes patches [j0, j0 + B) of `list`
static inline void vr_pool_runs(const std::vector<VrPoolPatch> &list, int j0, int B, std::vector<VrPoolRun> &runs) {
  runs.clear();
  for (int b = 0; b < B; ++b) {
    const VrPoolPatch &p = list[(size_t)j0 + b];
    if (!runs.empty() && runs.back().song == p.song && runs.back().k0 + runs.back().count == p.k) ++runs.back().count;
    else runs.push_back(VrPoolRun{p.song, p.k, b, 1});
  }
}
