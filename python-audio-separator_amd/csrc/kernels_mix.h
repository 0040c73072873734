// Weighted sums of stereo stems that are already in HBM (asx_mixdown_batch_dev): the mix-downs of workflow.ChainSeparator -- "instrumental
// + backing vocals" and the like.  Per frame and channel, with a source shorter than n_out read as zeros behind its end:
//   acc = fl(w_0 * x_0);  acc = fl(acc + fl(w_k * x_k)), k = 1 .. K-1 in list order
// float32, one rounding per operation: the bits of the numpy float32 restatement.  The products and sums are written with the plain
// operators under `#pragma clang fp contract(off)`, which covers what stands lexically in the kernel; __fmul_rn / __fadd_rn are inline
// functions of a header compiled under the default contraction, and their product and sum were fused into one FMA after inlining.
// One launch serves every job of a call: a workgroup finds its job in the table by its index (blk0), a lane takes a group of four frames
// of both channels.  The kernel moves 8 K bytes in and 8 out per frame and does nothing else, so it is bound by HBM traffic: every group
// of four floats that is whole and whose address is a multiple of 16 bytes moves as one 16-byte access.  The groups of a job are anchored
// so that the OUTPUT's stores are the aligned ones (`shift`, chosen by the host from the output pointer): the frames in front of the first
// whole group (the head) and behind the last one (the tail) go one float at a time, and so does a source row that is not aligned at the
// output's anchor.
#pragma once

constexpr int MIX_MAX_K = 8;   // ASX_MIX_MAX_K

struct MixDevJob {
  const float *x[MIX_MAX_K];   // planar [2, n] or rows [n, 2]; not read where n == 0
  int64_t n[MIX_MAX_K];
  float w[MIX_MAX_K];
  int32_t rows[MIX_MAX_K];
  float *out;                  // planar [2, n_out] or rows [n_out, 2]
  int64_t n_out;
  int32_t k, out_rows;
  int32_t shift;               // group g covers the frames 4 g - shift .. 4 g - shift + 3 (0 <= shift <= 3)
  int32_t blk0;                // the first workgroup of this job
};

static inline int64_t mix_groups(int64_t n_out, int shift) { return (n_out + shift + 3) / 4; }

// the shift at which the stores of whole groups are 16-byte aligned (0 where no shift makes them so: a rows output at an odd float)
static inline int mix_shift(const float *out, int out_rows) {
  const int a = (int)((((uintptr_t)out) >> 2) & 3);
  if (out_rows) return (a & 1) ? 0 : a / 2;
  return a;
}

// The job table holds generic pointers, which the compiler can only serve with flat accesses; every array of a job is in global memory,
// so the kernel says so (address space 1: global_load / global_store).
typedef float mix_f4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) float *mix_src_ptr;
typedef const __attribute__((address_space(1))) mix_f4 *mix_src_ptr4;
typedef __attribute__((address_space(1))) float *mix_out_ptr;
typedef __attribute__((address_space(1))) mix_f4 *mix_out_ptr4;

__device__ __forceinline__ bool mix_aligned16(const __attribute__((address_space(1))) float *p) { return (((uintptr_t)p) & 15) == 0; }

__global__ __launch_bounds__(256) void mixdown_kernel(const MixDevJob *__restrict__ jobs, int n_jobs) {
#pragma clang fp contract(off)
  int lo = 0, hi = n_jobs - 1;                         // the last job whose first workgroup is not behind this one
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].blk0 <= (int)blockIdx.x) lo = mid;
    else hi = mid - 1;
  }
  const MixDevJob &jb = jobs[lo];
  const int64_t n_out = jb.n_out;
  const int64_t f0 = 4 * ((int64_t)((int)blockIdx.x - jb.blk0) * 256 + threadIdx.x) - jb.shift;
  if (f0 >= n_out) return;
  float acc[8];                                        // interleaved: frame f0 + j's left at 2 j, right at 2 j + 1
  const int K = jb.k;
  for (int k = 0; k < K; ++k) {
    const mix_src_ptr x = (mix_src_ptr)jb.x[k];
    const int64_t n = jb.n[k];
    const float w = jb.w[k];
    const bool full = f0 >= 0 && f0 + 4 <= n;          // all four frames exist in this source
    float v[8];
    if (jb.rows[k]) {
      if (full && mix_aligned16(x + 2 * f0)) {
        const mix_f4 a = *(mix_src_ptr4)(x + 2 * f0), b = *(mix_src_ptr4)(x + 2 * f0 + 4);
        v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t f = f0 + j;
          const bool in = f >= 0 && f < n;
          v[2 * j] = in ? x[2 * f] : 0.f;
          v[2 * j + 1] = in ? x[2 * f + 1] : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        if (full && mix_aligned16(x + c * n + f0)) {
          const mix_f4 q = *(mix_src_ptr4)(x + c * n + f0);
          v[c] = q.x, v[2 + c] = q.y, v[4 + c] = q.z, v[6 + c] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int64_t f = f0 + j;
            v[2 * j + c] = (f >= 0 && f < n) ? x[c * n + f] : 0.f;
          }
        }
      }
    }
    if (k == 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[i] = w * v[i];
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float term = w * v[i];
        acc[i] = acc[i] + term;
      }
    }
  }
  const mix_out_ptr out = (mix_out_ptr)jb.out;
  const bool whole = f0 >= 0 && f0 + 4 <= n_out;
  if (jb.out_rows) {
    if (whole && mix_aligned16(out + 2 * f0)) {
      *(mix_out_ptr4)(out + 2 * f0) = mix_f4{acc[0], acc[1], acc[2], acc[3]};
      *(mix_out_ptr4)(out + 2 * f0 + 4) = mix_f4{acc[4], acc[5], acc[6], acc[7]};
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t f = f0 + j;
        if (f >= 0 && f < n_out) {
          out[2 * f] = acc[2 * j];
          out[2 * f + 1] = acc[2 * j + 1];
        }
      }
    }
  } else {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (whole && mix_aligned16(out + c * n_out + f0)) {
        *(mix_out_ptr4)(out + c * n_out + f0) = mix_f4{acc[c], acc[2 + c], acc[4 + c], acc[6 + c]};
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t f = f0 + j;
          if (f >= 0 && f < n_out) out[c * n_out + f] = acc[2 * j + c];
        }
      }
    }
  }
}
