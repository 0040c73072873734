// The plan of a pooled sinc conversion (asx_resample_sinc_batch_dev) on the host (no HIP): the checks of the job list, per job the
// frames the library really generates -- python-samplerate's int(n_in * ratio), less the frame a one-channel call drops at the end of
// its input (engine_vr.h resample_sinc_dev) -- and every job's first workgroup in the grid of the pooled launch, 256 output frames per
// workgroup.  Included by engine_vr.h and, for the host test, by tests/host/sinc_pool_plan_host.cpp.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

constexpr int SINC_PLAN_BLOCK = 256;
constexpr int SINC_PLAN_MAX_JOBS = 65535;
constexpr int SINC_PLAN_MAX_CHANNELS = 65535;              // grid.y of the launch
constexpr int64_t SINC_PLAN_MAX_FRAMES = (int64_t)1 << 40;   // n_in * ratio stays far inside the integers a double holds exactly

struct SincPlanJobIn {
  const void *x = nullptr, *y = nullptr;
  int64_t n_in = 0, n_out = 0;
  int channels = 0;
};

struct SincPlanJob {
  int64_t n_gen = 0;     // output frames the converter computes; [n_gen, n_out) are zero
  int64_t blocks = 0;    // ceil(n_out / 256)
  int64_t blk0 = 0;      // first workgroup (x) of the job
};

struct SincPoolPlan {
  std::vector<SincPlanJob> job;
  int64_t blocks = 0;    // grid.x
  int max_channels = 0;  // grid.y
};

// frames of src_simple for n_in input frames: int(n_in * ratio); `one_channel`: the call's end-of-input test drops the last of them
// when n_in * ratio is an integer (the frame would need input up to the very end)
static inline int64_t sinc_plan_generated(int64_t n_in, double ratio, bool one_channel) {
  const double t = (double)n_in * ratio;
  int64_t n_gen = (int64_t)t;
  if (one_channel && (double)n_gen == t && n_gen > 0) --n_gen;
  return n_gen;
}

// "" or why the job list cannot be planned (naming the job)
static inline std::string sinc_pool_check(const SincPlanJobIn *jobs, int n_jobs, double ratio) {
  if (n_jobs < 0) return "n_jobs must be >= 0";
  if (n_jobs > 0 && jobs == nullptr) return "null job list";
  if (n_jobs > SINC_PLAN_MAX_JOBS) return std::to_string(n_jobs) + " jobs in one call (at most " + std::to_string(SINC_PLAN_MAX_JOBS) + ")";
  if (!(ratio > 1.0 / 256 && ratio < 256.0)) {   // (a NaN too)
    char r[40];
    snprintf(r, sizeof(r), "%g", ratio);
    return std::string("ratio ") + r + " outside libsamplerate's (1/256, 256)";
  }
  int64_t blocks = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const SincPlanJobIn &g = jobs[j];
    const std::string who = "job " + std::to_string(j) + ": ";
    if (g.x == nullptr || g.y == nullptr) return who + "null input or output";
    if (g.n_in < 1 || g.n_in > SINC_PLAN_MAX_FRAMES) return who + "n_in = " + std::to_string(g.n_in) + " (1 .. 2^40)";
    if (g.n_out < 1 || g.n_out > SINC_PLAN_MAX_FRAMES) return who + "n_out = " + std::to_string(g.n_out) + " (1 .. 2^40)";
    if (g.channels < 1 || g.channels > SINC_PLAN_MAX_CHANNELS)
      return who + std::to_string(g.channels) + " channels (1 .. " + std::to_string(SINC_PLAN_MAX_CHANNELS) + ")";
    blocks += (g.n_out + SINC_PLAN_BLOCK - 1) / SINC_PLAN_BLOCK;
    if (blocks >= ((int64_t)1 << 31)) return who + "the jobs up to this one make " + std::to_string(blocks) + " workgroups (2^31 - 1 at most)";
  }
  return "";
}

// of a checked list
static inline void sinc_pool_build(const SincPlanJobIn *jobs, int n_jobs, double ratio, bool mono_calls, SincPoolPlan &pp) {
  pp = SincPoolPlan();
  pp.job.resize((size_t)(n_jobs > 0 ? n_jobs : 0));
  for (int j = 0; j < n_jobs; ++j) {
    SincPlanJob &p = pp.job[j];
    const int64_t n_gen = sinc_plan_generated(jobs[j].n_in, ratio, mono_calls || jobs[j].channels == 1);
    p.n_gen = n_gen < jobs[j].n_out ? n_gen : jobs[j].n_out;
    p.blocks = (jobs[j].n_out + SINC_PLAN_BLOCK - 1) / SINC_PLAN_BLOCK;
    p.blk0 = pp.blocks;
    pp.blocks += p.blocks;
    if (jobs[j].channels > pp.max_channels) pp.max_channels = jobs[j].channels;
  }
}
