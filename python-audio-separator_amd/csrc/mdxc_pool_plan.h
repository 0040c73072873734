// The chunk plans of the MDXC plugin's two demix loops on the host (no HIP): the TFC branch (mdxc_separator.py:361-402 -- front
// zeros, pad, Tensor.unfold) and the Roformer branch (:298-341 -- starts 0, step, ... < N with the tail re-anchored to N - C), for
// one song and for a pool of songs (asx_mdxc_demix_batch_dev / asx_rof_demix_batch_dev): every song's first pooled chunk and the
// passes that cut the pooled list.  Included by asx.hip -- asx_mdxc_plan, asx_rof_plan and every demix call are these functions -- by the fold kernels
// (the chunk range of a sample) and, for the host test, by tests/host/mdxc_pool_host.cpp.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "batching.h"

#if defined(__HIPCC__)
#define MDXC_PLAN_HD __host__ __device__
#else
#define MDXC_PLAN_HD
#endif

// ---- TFC branch ----------------------------------------------------------------------------------------------------------
struct MdxcTfcPlan {
  int64_t n_samples = 0, chunk_size = 0, step = 0, pad = 0, padded_len = 0;
  int64_t front = 0;   // zeros in front: chunk_size - step
  int n_chunks = 0;
};

// "" or why the geometry / the song cannot be planned
static inline std::string mdxc_tfc_plan(int hop, int dim_t, int64_t N, int overlap, MdxcTfcPlan &p) {
  if (N < 1 || overlap < 1) return "n_samples and overlap must be >= 1";
  p = MdxcTfcPlan();
  p.n_samples = N;
  p.chunk_size = (int64_t)hop * (dim_t - 1);
  p.step = p.chunk_size / overlap;                           // hop_size (mdxc_separator.py:364)
  if (p.step < 1) return "overlap larger than chunk_size";
  int64_t r = (N - p.chunk_size) % p.step;                   // Python floor-mod (:368)
  if (r < 0) r += p.step;
  p.pad = p.step - r;
  p.front = p.chunk_size - p.step;                           // zeros in front (:371)
  p.padded_len = p.front + N + p.pad + p.chunk_size - p.step;
  p.n_chunks = (int)((p.padded_len - p.chunk_size) / p.step + 1);   // Tensor.unfold (:374)
  return "";
}

// ---- Roformer branch -----------------------------------------------------------------------------------------------------
// chunks of a song: i = 0, step, ... < N
MDXC_PLAN_HD static inline int64_t rof_plan_count(int64_t N, int64_t step) { return (N + step - 1) / step; }

// start of chunk k: k * step, re-anchored to N - C when the chunk would run past the end (:323-336).  Every chunk behind the
// first re-anchored one is re-anchored too (they all start at N - C), so the regular chunks are k < rof_plan_regular().
MDXC_PLAN_HD static inline int64_t rof_plan_start(int64_t k, int64_t step, int64_t N, int64_t C) {
  const int64_t i = k * step;
  return i + C > N ? N - C : i;
}
MDXC_PLAN_HD static inline int64_t rof_plan_regular(int64_t N, int64_t C, int64_t step) { return (N - C) / step + 1; }

static inline std::string rof_plan_check(int64_t N, int64_t C, int64_t step) {
  if (N < C)
    return "mix (" + std::to_string(N) + " samples) shorter than one chunk (" + std::to_string(C) + "): not supported on the Roformer path";
  if (step < 1 || step > C) return "step must be in [1, chunk_size]";
  return "";
}

static inline std::string rof_plan_starts(int64_t N, int64_t C, int64_t step, std::vector<int64_t> &starts) {
  starts.clear();
  const std::string why = rof_plan_check(N, C, step);
  if (!why.empty()) return why;
  const int64_t nk = rof_plan_count(N, step);
  for (int64_t k = 0; k < nk; ++k) starts.push_back(rof_plan_start(k, step, N, C));
  return "";
}

// The chunks that cover sample i of a song of N samples in nk chunks, in increasing k: the regular ones [k_lo, k_hi] (start
// k * step), then the re-anchored ones [r_lo, r_hi] (start N - C); either range is empty when lo > hi.  At most C / step + 1
// regular and C / step re-anchored chunks: bounded by the geometry, whatever the song's or a pool's chunk count.
struct RofFoldRange {
  int64_t k_lo, k_hi, r_lo, r_hi;
};
MDXC_PLAN_HD static inline RofFoldRange rof_fold_range(int64_t i, int64_t N, int64_t C, int64_t step, int64_t nk) {
  RofFoldRange r;
  const int64_t nreg = rof_plan_regular(N, C, step);
  r.k_lo = i - C >= 0 ? (i - C) / step + 1 : 0;             // ceil((i - C + 1) / step)
  r.k_hi = i / step;
  if (r.k_hi > nreg - 1) r.k_hi = nreg - 1;
  r.r_lo = nreg;
  r.r_hi = i >= N - C ? nk - 1 : nreg - 1;
  return r;
}

// ---- a pool of songs -----------------------------------------------------------------------------------------------------
// The chunks of all songs stand one after the other in song order; song i owns pooled chunks [chunk0[i], chunk0[i + 1]).
struct MdxcPoolPlan {
  int64_t chunk_size = 0, step = 0, front = 0;
  int overlap = 0;                         // TFC branch: the fold's divisor
  std::vector<int> chunk0 = {0};           // n_songs + 1 entries
  std::vector<MdxcTfcPlan> tfc;            // TFC branch: per song
  std::vector<std::vector<int64_t>> starts;   // Roformer branch: per song
  int total() const { return chunk0.back(); }
};

static inline std::string mdxc_pool_add(MdxcPoolPlan &pp, int64_t n_chunks) {
  const int64_t total = (int64_t)pp.chunk0.back() + n_chunks;
  if (total >= ((int64_t)1 << 30)) return std::to_string(total) + " chunks in one pool";
  pp.chunk0.push_back((int)total);
  return "";
}

// One more song behind the ones `pp` holds: "" or why not, `pp` then unchanged.  A single-song call is these on an empty plan.
static inline std::string mdxc_pool_push_tfc(MdxcPoolPlan &pp, int hop, int dim_t, int overlap, int64_t N) {
  MdxcTfcPlan p;
  std::string why = mdxc_tfc_plan(hop, dim_t, N, overlap, p);
  if (why.empty()) why = mdxc_pool_add(pp, p.n_chunks);
  if (!why.empty()) return why;
  pp.tfc.push_back(p);
  pp.chunk_size = p.chunk_size;
  pp.step = p.step;
  pp.front = p.front;
  pp.overlap = overlap;
  return "";
}

static inline std::string mdxc_pool_push_rof(MdxcPoolPlan &pp, int hop, int dim_t, int64_t step, int64_t N) {
  std::vector<int64_t> st;
  std::string why = rof_plan_starts(N, (int64_t)hop * (dim_t - 1), step, st);
  if (why.empty()) why = mdxc_pool_add(pp, (int64_t)st.size());
  if (!why.empty()) return why;
  pp.starts.push_back(st);
  pp.chunk_size = (int64_t)hop * (dim_t - 1);
  pp.step = step;
  return "";
}

// false (and `err`, naming the song) when any one song is rejected: the caller then enqueues nothing.
static inline bool mdxc_pool_build_tfc(int hop, int dim_t, int overlap, const int64_t *Ns, int n_songs, MdxcPoolPlan &pp, std::string &err) {
  pp = MdxcPoolPlan();
  err.clear();
  for (int i = 0; i < n_songs && err.empty(); ++i) {
    const std::string why = mdxc_pool_push_tfc(pp, hop, dim_t, overlap, Ns[i]);
    if (!why.empty()) err = "song " + std::to_string(i) + ": " + why;
  }
  return err.empty();
}

static inline bool mdxc_pool_build_rof(int hop, int dim_t, int64_t step, const int64_t *Ns, int n_songs, MdxcPoolPlan &pp, std::string &err) {
  pp = MdxcPoolPlan();
  err.clear();
  for (int i = 0; i < n_songs && err.empty(); ++i) {
    const std::string why = Ns[i] < 1 ? std::string("n_samples must be >= 1") : mdxc_pool_push_rof(pp, hop, dim_t, step, Ns[i]);
    if (!why.empty()) err = "song " + std::to_string(i) + ": " + why;
  }
  return err.empty();
}

// chunks per net pass for a pool of `total` chunks (8 when max_batch is 0, as the single-song calls)
static inline int mdxc_pool_per_pass(int total, int max_batch) { return even_batches(total, max_batch > 0 ? max_batch : 8); }
