// Phase fix ("phase swapper") on stems in HBM: the STFT magnitudes of a target stem on phases blended towards a source stem's.
// librosa STFT(2048, hop) of both (the frames ens_frame_spectrum_of forms), per frame and bin k with z = S conj(T):
//   delta = atan2(Im z, Re z)   (0 where z == 0);   O_k = T_k (cos(w_k delta) + j sin(w_k delta))
// and librosa's istft(O, length = n): the structure of ens_invert_song_frame / ens_invert_song_fold (kernels_ens.h) -- one workgroup
// per (frame, channel) transforms both frames, combines them per bin in LDS and inverse-transforms the result into [2, T, n_fft];
// one fold launch divides the overlap-added frames by the window-sum-square.  No spectrogram is ever written to HBM.  The bin
// weights w are a table of n_fft / 2 + 1 floats the host made: no cutoff frequency is known here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asx {

// One job of asx_phase_fix_dev / asx_phase_fix_batch_dev.  Its inverse frames are [2, T, n_fft] from frame0 * 2 * n_fft of the workspace;
// frame0 / fold_blk0: its first frame / fold workgroup in the launch (ascending over the jobs of a pooled call, 0 in the single form).
struct PhaseJob {
  const float *target;   // planar [2, n] or rows [n, 2]
  const float *source;   // planar [2, n_src] or rows [n_src, 2]; read as zeros from n_src on, never beyond n
  float *out;            // planar [2, n] or rows [n, 2]
  int64_t n, n_src;
  int64_t frame0, fold_blk0;
  int32_t T, target_rows, source_rows, out_rows;
};

__device__ __forceinline__ float phase_stem_value(const float *__restrict__ x, int64_t n, int rows, int ch, int64_t q) {
  return rows ? x[2 * q + ch] : x[(int64_t)ch * n + q];
}

// T[b] <- T[b] rotated by w[b] * delta_b towards S[b], b = 0 .. nh, in LDS.  Every product is rounded on its own (contraction off), so
// S = -T gives Im z = fl(S_i T_r) - fl(S_r T_i) = +0 exactly and delta = +pi in every bin: the tie rule.  An angle of zero (w = 0, or
// delta = 0: S = T, a silent source, a bin where z underflows to zero) leaves T as it is, bit for bit.
__device__ __forceinline__ void phase_fix_bins(float2 *T, const float2 *S, const float *__restrict__ w, int nh) {
#pragma clang fp contract(off)
  for (int b = threadIdx.x; b <= nh; b += blockDim.x) {
    const float2 t = T[b], s = S[b];
    const float re = s.x * t.x + s.y * t.y;
    const float im = s.y * t.x - s.x * t.y;
    const float delta = (re == 0.f && im == 0.f) ? 0.f : atan2f(im, re);
    const float ang = w[b] * delta;
    if (ang != 0.f) {
      float sn, cs;
      sincosf(ang, &sn, &cs);
      T[b] = make_float2(t.x * cs - t.y * sn, t.x * sn + t.y * cs);
    }
  }
  __syncthreads();
}

// frame t of channel ch of one job -> frames[ch, t, :].  LDS: bufA, bufB (nh each), X, Y (nh + 1 each) -- ens_invert_frame's footprint.
__device__ __forceinline__ void phase_fix_job_frame(const PhaseJob &jb, int t, int ch, int hop, const float *__restrict__ weights,
                                                    float *__restrict__ frames, const float *__restrict__ window,
                                                    const float2 *__restrict__ tw, const FftPlan &p, float2 *lds) {
  const int nh = p.nh;
  float2 *bufA = lds, *bufB = lds + nh, *X = lds + 2 * nh, *Y = X + (nh + 1);
  ens_frame_spectrum_of([&](int64_t q) { return phase_stem_value(jb.target, jb.n, jb.target_rows, ch, q); }, jb.n, t, hop, window, tw, p,
                        bufA, bufB, X);
  ens_frame_spectrum_of([&](int64_t q) { return q < jb.n_src ? phase_stem_value(jb.source, jb.n_src, jb.source_rows, ch, q) : 0.f; },
                        jb.n, t, hop, window, tw, p, bufA, bufB, Y);
  phase_fix_bins(X, Y, weights, nh);
  // (ens_inverse_frame drops the imaginary parts of bins 0 and nh: only their real parts enter the inverse transform)
  ens_inverse_frame(X, frames + ((jb.frame0 * 2 + (int64_t)ch * jb.T) + t) * p.n_fft, window, tw, p, bufA, bufB, 1.0f);
}

// ens_pool_fold_kernel's fold for length = n (the covering frames added in ascending order over the window-sum-square formed here in
// float64 and rounded once), written in the job's output layout
__device__ __forceinline__ void phase_fix_job_fold(const PhaseJob &jb, int64_t blk, const float *__restrict__ frames,
                                                   const float *__restrict__ window, int n_fft, int hop) {
  const int64_t len = jb.n;
  const int64_t i = (blk - jb.fold_blk0) * 256 + threadIdx.x;
  if (i >= len) return;
  const int64_t m = i + n_fft / 2;
  int64_t t_lo, t_hi;
  ola_frame_range(m, n_fft, hop, jb.T, &t_lo, &t_hi);
  double ss = 0.0;
  for (int64_t t = t_lo; t <= t_hi; ++t) {
    const double w = (double)window[m - t * hop];
    ss += w * w;
  }
  const float s = (float)ss;
  const float *fr = frames + jb.frame0 * 2 * n_fft;
  const float l = ola_sample(fr, n_fft, hop, m, t_lo, t_hi, s);
  const float r = ola_sample(fr + (int64_t)jb.T * n_fft, n_fft, hop, m, t_lo, t_hi, s);
  if (jb.out_rows) {
    jb.out[2 * i] = l;
    jb.out[2 * i + 1] = r;
  } else {
    jb.out[i] = l;
    jb.out[len + i] = r;
  }
}

// one job: grid = (T, 2), then ((n + 255) / 256)
__global__ __launch_bounds__(256) void phase_fix_kernel(PhaseJob jb, int hop, const float *__restrict__ weights, float *__restrict__ frames,
                                                        const float *__restrict__ window, const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  phase_fix_job_frame(jb, (int)blockIdx.x, (int)blockIdx.y, hop, weights, frames, window, tw, p, lds);
}
__global__ __launch_bounds__(256) void phase_fix_fold_kernel(PhaseJob jb, const float *__restrict__ frames, const float *__restrict__ window,
                                                             int n_fft, int hop) {
  phase_fix_job_fold(jb, blockIdx.x, frames, window, n_fft, hop);
}

// a pool of jobs: grid = (frames of all jobs, 2), then (fold workgroups of all jobs); a workgroup finds its job in the table
__global__ __launch_bounds__(256) void phase_fix_pool_kernel(const PhaseJob *__restrict__ jobs, int n_jobs, int hop,
                                                             const float *__restrict__ weights, float *__restrict__ frames,
                                                             const float *__restrict__ window, const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  const PhaseJob &jb = jobs[ens_pool_find<PhaseJob, &PhaseJob::frame0>(jobs, n_jobs, blockIdx.x)];
  phase_fix_job_frame(jb, (int)((int64_t)blockIdx.x - jb.frame0), (int)blockIdx.y, hop, weights, frames, window, tw, p, lds);
}
__global__ __launch_bounds__(256) void phase_fix_pool_fold_kernel(const PhaseJob *__restrict__ jobs, int n_jobs, const float *__restrict__ frames,
                                                                  const float *__restrict__ window, int n_fft, int hop) {
  const PhaseJob &jb = jobs[ens_pool_find<PhaseJob, &PhaseJob::fold_blk0>(jobs, n_jobs, blockIdx.x)];
  phase_fix_job_fold(jb, blockIdx.x, frames, window, n_fft, hop);
}

}  // namespace asx
