// A pool of songs on the MDXC plugin's two demix loops (asx_mdxc_demix_batch_dev / asx_rof_demix_batch_dev; the single-song
// calls run a pool of one -- these are the plugin's only table and fold kernels): the chunks of all songs stand one after the other in one chunk buffer [total, S, 2, C] and go through the STFT / net / iSTFT launches in passes that
// may straddle songs (stft_pool_kernel reads chunk b from ITS song, kernels_fft.h PoolChunks).  Per-song are only the tables
// below, built on the device from launch arguments (no host copy: the call stays stream-ordered), and the two folds.
#pragma once
#include "kernels_fft.h"      // POOL_GROUP
#include "mdxc_pool_plan.h"   // rof_plan_start, rof_fold_range
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asx {

struct MdxcPoolSong {         // fold table, one entry per song
  const float *chunks;        // the song's chunks [n_chunks, S, 2, C] inside the pooled chunk buffer
  float *out;                 // [S, 2, N] (Roformer: [n_out, 2, N])
  int64_t N;
  int64_t blk0;               // first workgroup (x) of the song in the fold's grid
  int64_t n_chunks;
};

struct MdxcPoolGroup {        // up to POOL_GROUP songs, by value in the launch arguments
  const float *mix[POOL_GROUP];
  float *out[POOL_GROUP];
  int64_t n[POOL_GROUP];
  int64_t blk0[POOL_GROUP];
  int chunk0[POOL_GROUP + 1];      // first pooled chunk of each song (+ the end of the last)
  int n_songs, song0;              // songs in this group, pool index of its first
};

// chunk j of the pool: its song (base pointer, length) and its start -- TFC branch (rof == 0): k * step in the song's padded domain
// (the launch's `trim` is the front zeros); Roformer branch: k * step or the re-anchored N - C, trim 0.  Thread i < n_songs also
// writes the fold entry of song song0 + i.  chunk_floats = S * 2 * C.
__global__ __launch_bounds__(256) void mdxc_pool_table_kernel(MdxcPoolGroup g, int64_t step, int64_t C, int rof, int64_t chunk_floats,
                                                              const float *chunk_buf, const float **__restrict__ wave,
                                                              int64_t *__restrict__ n_song, int64_t *__restrict__ starts,
                                                              MdxcPoolSong *__restrict__ songs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < g.n_songs) {
    MdxcPoolSong ps;
    ps.chunks = chunk_buf + (int64_t)g.chunk0[i] * chunk_floats;
    ps.out = g.out[i];
    ps.N = g.n[i];
    ps.blk0 = g.blk0[i];
    ps.n_chunks = g.chunk0[i + 1] - g.chunk0[i];
    songs[g.song0 + i] = ps;
  }
  const int j = g.chunk0[0] + i;
  if (j >= g.chunk0[g.n_songs]) return;
  int sg = 0;
  while (sg + 1 < g.n_songs && g.chunk0[sg + 1] <= j) ++sg;
  const int64_t N = g.n[sg];
  const int64_t k = j - g.chunk0[sg];
  wave[j] = g.mix[sg];
  n_song[j] = N;
  starts[j] = rof ? rof_plan_start(k, step, N, C) : k * step;
}

// the song whose workgroups hold blockIdx.x (MdxcPoolSong::blk0 ascending)
__device__ __forceinline__ int mdxc_pool_find(const MdxcPoolSong *__restrict__ songs, int n_songs) {
  int lo = 0, hi = n_songs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (songs[mid].blk0 <= (int64_t)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// TFC branch fold (mdxc_separator.py:398-402): accumulated[..., k*hop : k*hop+chunk] += out_k ; result = accumulated / overlap, for
// every song of a pool in one launch: grid.x = the songs' workgroups one after the other, grid.y = S * 2.  Gather form: per sample the
// sum over the covering chunks of the sample's own song in increasing k; sample i sits at padded position i + front.
__global__ __launch_bounds__(256) void mdxc_finalize_pool_kernel(const MdxcPoolSong *__restrict__ songs, int n_songs, int S, int64_t C,
                                                                 int64_t hop, int64_t front, float overlap) {
  const MdxcPoolSong sg = songs[mdxc_pool_find(songs, n_songs)];
  const int sc = blockIdx.y;  // s*2 + ch
  const int64_t N = sg.N;
  const int64_t i = ((int64_t)blockIdx.x - sg.blk0) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float *__restrict__ chunk_out = sg.chunks;
  const int64_t m = i + front;
  int64_t k_hi = m / hop;
  if (k_hi > sg.n_chunks - 1) k_hi = sg.n_chunks - 1;
  int64_t k_lo = 0;
  if (m - C >= 0) k_lo = (m - C) / hop + 1;
  float acc = 0.f;
  for (int64_t k = k_lo; k <= k_hi; ++k) acc += chunk_out[((k * S * 2) + sc) * C + (m - k * hop)];
  sg.out[(int64_t)sc * N + i] = acc / overlap;
}

// Roformer fold (mdxc_separator.py:320-343): result += x * w, counter += w, out = result / clamp(counter, 1e-10), for every song of
// a pool in one launch: grid.y = n_out * 2, out row o reads chunk stem o % S (the reference broadcasts a single-stem output over
// len(instruments) rows).  Per sample the chunks k with 0 <= i - start_k < C in increasing k -- rof_fold_range: the regular ones, then
// the re-anchored tail chunks -- so work per sample is bounded by the geometry (about 2 C / step chunks), not by the chunk count.
__global__ __launch_bounds__(256) void roformer_finalize_pool_kernel(const MdxcPoolSong *__restrict__ songs, int n_songs, int S, int64_t C,
                                                                     int64_t step, const float *__restrict__ window) {
  const MdxcPoolSong sg = songs[mdxc_pool_find(songs, n_songs)];
  const int oc = blockIdx.y;  // o*2 + ch
  const int o = oc >> 1, ch = oc & 1;
  const int s = o % S;
  const int64_t N = sg.N;
  const int64_t i = ((int64_t)blockIdx.x - sg.blk0) * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const float *__restrict__ chunk_out = sg.chunks;
  const RofFoldRange r = rof_fold_range(i, N, C, step, sg.n_chunks);
  float acc = 0.f, cnt = 0.f;
  for (int64_t k = r.k_lo; k <= r.k_hi; ++k) {
    const int64_t j = i - k * step;
    const float w = window[j];
    acc += chunk_out[((k * S + s) * 2 + ch) * C + j] * w;
    cnt += w;
  }
  const int64_t jt = i - (N - C);
  for (int64_t k = r.r_lo; k <= r.r_hi; ++k) {
    const float w = window[jt];
    acc += chunk_out[((k * S + s) * 2 + ch) * C + jt] * w;
    cnt += w;
  }
  sg.out[(int64_t)oc * N + i] = acc / fmaxf(cnt, 1e-10f);
}

}  // namespace asx
