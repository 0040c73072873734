// The plan of a pooled ensemble (asx_ensemble_batch_dev) on the host (no HIP): per (file, stem group) job the contributors that
// take part given their peaks, the padded length, the frame count and the output length -- the rules EnsembleSeparator's per-file
// loop applies with asx_ensemble_slot_dev + asx_ensemble_dev -- and every job's first workgroup / first frame in the grids of the
// pooled launches.  Included by engine_ens.h and, for the host test, by tests/host/ens_pool_host.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

constexpr int ENS_PLAN_MAX_K = 8;
constexpr int ENS_PLAN_HOP = 1024, ENS_PLAN_NFFT = 2048, ENS_PLAN_BLOCK = 256;
constexpr int ENS_PLAN_MAX_JOBS = 8191;   // 8 contributors each: the peak launch has one grid row per contributor (65,535 rows at most)

// algorithm numbers of include/asx.h (kernels_ens.h carries the same enum)
static inline bool ens_plan_is_wave(int alg) { return alg >= 0 && alg <= 3; }
static inline bool ens_plan_is_uvr(int alg) { return alg == 8 || alg == 9; }
static inline bool ens_plan_is_pick(int alg) { return alg == 10; }   // ensemble_wav

struct EnsPlanJobIn {
  int k = 0;
  int64_t n[ENS_PLAN_MAX_K] = {};
  float peak_after[ENS_PLAN_MAX_K] = {};   // what asx_ensemble_slot_dev reports for the contributor
};

struct EnsPlanJob {
  int live = 0;
  int who[ENS_PLAN_MAX_K] = {};   // the contributors that take part, in their order
  int64_t n_max = 0;              // the longest of them
  int T = 0;                      // 1 + n_max / 1024: frames of the centred STFT
  int64_t n_out = 0;              // samples per channel of the result; 0: none
  // shares of the pooled grids: workgroups of 256 over the 2 * n_out values of a result formed per sample (wave algorithms,
  // ensemble_wav's row copy, a lone contributor's slot image), frames of a spectral combine, workgroups of its fold over n_out
  int64_t wave_blocks = 0, wave_blk0 = 0;
  int64_t frames = 0, frame0 = 0;
  int64_t fold_blocks = 0, fold_blk0 = 0;
  bool pick = false;              // takes part in ensemble_wav's sums and argmin
};

struct EnsPoolPlan {
  std::vector<EnsPlanJob> job;
  int64_t wave_blocks = 0, frames = 0, fold_blocks = 0;
  int picks = 0;
};

// "" or why the job list cannot be planned (naming the job)
static inline std::string ens_pool_check(const EnsPlanJobIn *jobs, int n_jobs, int alg) {
  if (n_jobs < 0) return "n_jobs must be >= 0";
  if (n_jobs > ENS_PLAN_MAX_JOBS) return std::to_string(n_jobs) + " jobs in one call (at most " + std::to_string(ENS_PLAN_MAX_JOBS) + ")";
  if (alg < 0 || alg > 10) return "unknown ensemble algorithm " + std::to_string(alg);
  for (int j = 0; j < n_jobs; ++j) {
    if (jobs[j].k < 1 || jobs[j].k > ENS_PLAN_MAX_K)
      return "job " + std::to_string(j) + ": " + std::to_string(jobs[j].k) + " contributors (1 .. " + std::to_string(ENS_PLAN_MAX_K) + " are built)";
    for (int c = 0; c < jobs[j].k; ++c)
      if (jobs[j].n[c] < 0 || jobs[j].n[c] > ((int64_t)1 << 38))
        return "job " + std::to_string(j) + ": contributor " + std::to_string(c) + " has n = " + std::to_string(jobs[j].n[c]) + " (0 .. 2^38)";
  }
  return "";
}

// A contributor whose peak after normalisation is below `silent_below` is left out (write_audio writes no file for it, so the
// Ensembler never sees it); the rest are padded to the longest of THEM.  One contributor left: its slot image is the result.
static inline void ens_pool_build(const EnsPlanJobIn *jobs, int n_jobs, int alg, double silent_below, EnsPoolPlan &pp) {
  pp = EnsPoolPlan();
  pp.job.resize((size_t)(n_jobs > 0 ? n_jobs : 0));
  for (int j = 0; j < n_jobs; ++j) {
    EnsPlanJob &p = pp.job[j];
    for (int c = 0; c < jobs[j].k; ++c) {
      if ((double)jobs[j].peak_after[c] < silent_below) continue;   // the comparison write_audio makes (float32 peak, float64 bound)
      p.who[p.live++] = c;
      if (jobs[j].n[c] > p.n_max) p.n_max = jobs[j].n[c];
    }
    p.wave_blk0 = pp.wave_blocks;
    p.frame0 = pp.frames;
    p.fold_blk0 = pp.fold_blocks;
    if (p.live == 0) {
      p.n_max = 0;
      continue;
    }
    p.T = (int)(1 + p.n_max / ENS_PLAN_HOP);
    const bool per_sample = p.live == 1 || ens_plan_is_wave(alg) || ens_plan_is_pick(alg);
    if (per_sample) {
      p.n_out = p.n_max;
      p.wave_blocks = (2 * p.n_out + ENS_PLAN_BLOCK - 1) / ENS_PLAN_BLOCK;
      p.pick = p.live >= 2 && ens_plan_is_pick(alg);
    } else if (ens_plan_is_uvr(alg) && p.T < 2) {
      p.n_out = 0;   // one frame and no length argument: the reference's istft returns [2, 0]
    } else {
      p.n_out = ens_plan_is_uvr(alg) ? (int64_t)ENS_PLAN_HOP * (p.T - 1) : p.n_max;
      p.frames = p.T;
      p.fold_blocks = (p.n_out + ENS_PLAN_BLOCK - 1) / ENS_PLAN_BLOCK;
    }
    pp.wave_blocks += p.wave_blocks;
    pp.frames += p.frames;
    pp.fold_blocks += p.fold_blocks;
    pp.picks += p.pick ? 1 : 0;
  }
}
