// Spectral edges on the device: Ensembler.ensemble (audio_separator/separator/ensembler.py:12-160) and
// spec_utils.invert_stem (uvr_lib_v5/spec_utils.py:557-580).  Both are librosa STFT(2048, 1024) -> per-bin
// selection / averaging -> iSTFT; one workgroup per (frame, channel) transforms every input frame, combines the
// spectra in LDS and inverse-transforms the result, so no spectrogram is ever written to HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace asx {

enum { ENS_AVG_WAVE = 0, ENS_MEDIAN_WAVE = 1, ENS_MIN_WAVE = 2, ENS_MAX_WAVE = 3, ENS_AVG_FFT = 4, ENS_MEDIAN_FFT = 5,
       ENS_MIN_FFT = 6, ENS_MAX_FFT = 7, ENS_UVR_MAX_SPEC = 8, ENS_UVR_MIN_SPEC = 9, ENS_ENSEMBLE_WAV = 10 };
constexpr int ENS_ABS_BLOCKS = 256;   // partial sums per (input, channel) of ensemble_wav
constexpr int ENS_MAX_K = 8;

__device__ __forceinline__ float median_small(float *v, int K) {
  for (int i = 1; i < K; ++i) {   // insertion sort, K <= 8
    const float x = v[i];
    int j = i - 1;
    while (j >= 0 && v[j] > x) {
      v[j + 1] = v[j];
      --j;
    }
    v[j + 1] = x;
  }
  return (K & 1) ? v[K / 2] : (v[K / 2 - 1] + v[K / 2]) / 2.0f;   // np.median: mean of the two middle values
}

// avg / median / min / max of one sample over K waveforms (ensembler.py:48-64); weights only for avg.  ld(k): the sample of input k.
template <class Load>
__device__ __forceinline__ float ens_wave_combine(Load ld, int K, int alg, const double *__restrict__ weights, double wsum) {
  if (alg == ENS_AVG_WAVE) {
    float acc = 0.f;   // `ensembled += w * weight` rounds to float32 after every term (float64 product)
    for (int k = 0; k < K; ++k) acc = (float)((double)acc + (double)ld(k) * weights[k]);
    return (float)((double)acc / wsum);
  }
  if (alg == ENS_MEDIAN_WAVE) {
    float v[ENS_MAX_K];
    for (int k = 0; k < K; ++k) v[k] = ld(k);
    return median_small(v, K);
  }
  float best = ld(0), bm = fabsf(best);
  for (int k = 1; k < K; ++k) {   // np.argmin / np.argmax: the first extremum wins
    const float x = ld(k), m = fabsf(x);
    if (alg == ENS_MIN_WAVE ? m < bm : m > bm) {
      best = x;
      bm = m;
    }
  }
  return best;
}

// the same over a stack [K, 2, N]
__global__ __launch_bounds__(256) void ens_wave_kernel(const float *__restrict__ waves, int K, int64_t n2, int alg,
                                                       const double *__restrict__ weights, double wsum, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n2) return;
  out[i] = ens_wave_combine([&](int k) { return waves[(int64_t)k * n2 + i]; }, K, alg, weights, wsum);
}

// spec_utils.ensemble_wav as Ensembler.ensemble calls it (uvr_lib_v5/spec_utils.py:1245-1266, ensembler.py:71-72): every channel
// is taken whole from the input whose mean |x| over that channel is smallest (np.array_split along axis 0 of a [2, N] array:
// section c < 2 is channel c, the other 238 sections are empty).  Three deterministic steps: partial sums of |x| in float64
// (fixed strided order per block), the argmin per channel (first minimum; a NaN sum wins like in np.argmin), the row copy.
// block `bx` of `gx` over one channel of one input: its strided share of sum |x| in float64, reduced in a fixed tree.  ld(i): sample i.
template <class Load>
__device__ __forceinline__ void ens_abssum_block(Load ld, int64_t N, int bx, int gx, double *__restrict__ dst) {
  double acc = 0.0;
  for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < N; i += (int64_t)gx * 256) acc += (double)fabsf(ld(i));
  __shared__ double sh[256];
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst = sh[0];
}
__global__ __launch_bounds__(256) void ens_abssum_kernel(const float *__restrict__ waves, int64_t N, double *__restrict__ partial) {
  const int kc = blockIdx.y;                        // input * 2 + channel
  const float *x = waves + (int64_t)kc * N;
  ens_abssum_block([&](int64_t i) { return x[i]; }, N, (int)blockIdx.x, (int)gridDim.x, partial + (int64_t)kc * gridDim.x + blockIdx.x);
}
// partial [K, 2, P] -> the input channel `ch` is taken from
__device__ __forceinline__ int ens_pick_channel(const double *__restrict__ partial, int K, int P, int ch) {
  int best = 0;
  double bt = 0.0;
  for (int k = 0; k < K; ++k) {
    double t = 0.0;
    for (int b = 0; b < P; ++b) t += partial[(int64_t)(k * 2 + ch) * P + b];
    if (k == 0) {
      bt = t;
    } else if (!(bt != bt) && ((t != t) || t < bt)) {   // np.argmin: the first NaN, else the first minimum
      best = k;
      bt = t;
    }
  }
  return best;
}
__global__ void ens_pick_kernel(const double *__restrict__ partial, int K, int P, int *__restrict__ sel) {
  const int ch = threadIdx.x;
  if (ch >= 2) return;
  sel[ch] = ens_pick_channel(partial, K, P, ch);
}
__global__ __launch_bounds__(256) void ens_take_kernel(const float *__restrict__ waves, int64_t N, const int *__restrict__ sel,
                                                       float *__restrict__ out) {
  const int ch = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) out[(int64_t)ch * N + i] = waves[((int64_t)sel[ch] * 2 + ch) * N + i];
}

// The edge between an ensemble member and the Ensembler (separator.py:1286, :1335): the member's stem goes through write_audio
// (spec_utils.normalize, (x * 32767).astype(int16), common_separator.py:309-337) and comes back through librosa.load
// (int16 / 32768 as float32), and Ensembler.ensemble zero-pads it to the longest wave (ensembler.py:29-30).  One pass, no
// int16 array: stem = planar [2, n] or rows [n, 2] -> slot [2, n_max] of the stack ens_*_kernel read.  The quantiser is
// pcm16_kernel's, operation for operation (float32, one rounding each, C truncation), so slot * 32768 IS the int16 that
// kernel writes; int16 -> float and the division by 2^15 are exact.  ENS_SLOT_FLOAT32: plain copy (+ transpose) and pad.
// The file modes are the same edge for a member that writes with soundfile (write_audio_soundfile, common_separator.py:399-461):
// the slot holds what pcm_decode_kernel reads out of the bytes pcm_encode_kernel writes for the stem -- the same normalisation,
// then clip(rint((double)x * (2^(b-1) - 1))) of pcmenc_quant and the int / 2^(b-1) of the decoder (PCM_32 through double, as
// there), or the normalised float itself.  The mode numbers of the file modes are the sample format codes of those kernels.
// Every element of the slot is written: the stack needs no clearing.
enum { ENS_SLOT_PCM16 = 0, ENS_SLOT_FLOAT32 = 1, ENS_SLOT_FILE_PCM16 = 16, ENS_SLOT_FILE_PCM24 = 24, ENS_SLOT_FILE_PCM32 = 32,
       ENS_SLOT_FILE_FLOAT = 0x120 };
static inline bool ens_slot_mode_known(int mode) {
  return mode == ENS_SLOT_PCM16 || mode == ENS_SLOT_FLOAT32 || mode == ENS_SLOT_FILE_PCM16 || mode == ENS_SLOT_FILE_PCM24 ||
         mode == ENS_SLOT_FILE_PCM32 || mode == ENS_SLOT_FILE_FLOAT;
}
// the integer sample of BITS bits audio_io.write_wav (and pcm_encode_kernel) stores for the normalised x: float64 product, ties to even
template <int BITS>
__device__ __forceinline__ int ens_slot_file_int(float x) {
  constexpr double full = (double)((1ll << (BITS - 1)) - 1);
  return (int)fmin(fmax(rint((double)x * full), -full - 1.0), full);
}
// mode: any but ENS_SLOT_FLOAT32.  In every mode the last operation is a multiplication (by a power of two after an integer, by the
// normalisation's scale for ENS_SLOT_FILE_FLOAT) formed with contraction off, or no operation at all.
__device__ __forceinline__ float ens_slot_quantise(float x, float maxv, float max_peak, float min_peak, int has_min, int mode) {
#pragma clang fp contract(off)
  float scale = 1.0f;
  bool scaled = false;
  if (maxv > max_peak) {
    scale = __fdiv_rn(max_peak, maxv);
    scaled = true;
  } else if (has_min && maxv < min_peak) {
    scale = __fdiv_rn(min_peak, maxv);
    scaled = true;
  }
  if (scaled) x = x * scale;
  if (mode == ENS_SLOT_PCM16) {
    const float q = x * 32767.0f;
    return (float)(short)(int)q * (1.0f / 32768.0f);
  }
  if (mode == ENS_SLOT_FILE_PCM16) return (float)(short)ens_slot_file_int<16>(x) * (1.0f / 32768.0f);
  if (mode == ENS_SLOT_FILE_PCM24) return (float)ens_slot_file_int<24>(x) * (1.0f / 8388608.0f);
  if (mode == ENS_SLOT_FILE_PCM32) return (float)((double)ens_slot_file_int<32>(x) * (1.0 / 2147483648.0));
  return x;   // ENS_SLOT_FILE_FLOAT
}
// sample i of channel ch of a stem of n samples as its slot holds it (zero from n on)
__device__ __forceinline__ float ens_slot_value(const float *__restrict__ stem, int64_t n, int rows, int ch, int64_t i, float maxv,
                                                float max_peak, float min_peak, int has_min, int mode) {
  if (i >= n) return 0.f;
  const float x = rows ? stem[2 * i + ch] : stem[(int64_t)ch * n + i];
  return mode != ENS_SLOT_FLOAT32 ? ens_slot_quantise(x, maxv, max_peak, min_peak, has_min, mode) : x;
}
__global__ __launch_bounds__(256) void ens_slot_kernel(const float *__restrict__ stem, int64_t n, int rows,
                                                       const unsigned int *peak_bits, float max_peak, float min_peak, int has_min,
                                                       int mode, float *__restrict__ slot, int64_t n_max) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_max) return;
  const float maxv = (mode != ENS_SLOT_FLOAT32 && i < n) ? __uint_as_float(*peak_bits) : 0.f;
  slot[i] = ens_slot_value(stem, n, rows, 0, i, maxv, max_peak, min_peak, has_min, mode);
  slot[n_max + i] = ens_slot_value(stem, n, rows, 1, i, maxv, max_peak, min_peak, has_min, mode);
}

// librosa.stft frame t of one channel of n samples (centre, zero padding) -> X[0 .. nh] in LDS.  ld(q): sample q, 0 <= q < n.
template <class Load>
__device__ __forceinline__ void ens_frame_spectrum_of(Load ld, int64_t n, int t, int hop, const float *__restrict__ window,
                                                      const float2 *__restrict__ tw, const FftPlan &p, float2 *bufA, float2 *bufB,
                                                      float2 *X) {
  float *fa = reinterpret_cast<float *>(bufA);
  for (int e = threadIdx.x; e < p.n_fft; e += blockDim.x) {
    const int64_t q = (int64_t)t * hop + e - p.nh;
    fa[e] = (q >= 0 && q < n) ? ld(q) * window[e] : 0.f;
  }
  float2 *Z = fft_lds<-1>(bufA, bufB, p, tw);
  const int nh = p.nh;
  for (int k = threadIdx.x; k <= nh; k += blockDim.x) {
    const float2 zk = Z[k == nh ? 0 : k];
    float2 zc = Z[(k == 0 || k == nh) ? 0 : nh - k];
    zc.y = -zc.y;
    const float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
    const float2 D = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
    const float2 O = make_float2(D.y, -D.x);
    const float2 w = (k == nh) ? make_float2(-1.f, 0.f) : tw[k];
    X[k] = cadd(E, cmul(w, O));
  }
  __syncthreads();
}
// the same for channel ch of a wave [2, n] in memory
__device__ __forceinline__ void ens_frame_spectrum(const float *__restrict__ wave, int64_t n, int ch, int t, int hop,
                                                   const float *__restrict__ window, const float2 *__restrict__ tw,
                                                   const FftPlan &p, float2 *bufA, float2 *bufB, float2 *X) {
  const float *x = wave + (int64_t)ch * n;
  ens_frame_spectrum_of([&](int64_t q) { return x[q]; }, n, t, hop, window, tw, p, bufA, bufB, X);
}

// X[0 .. nh] in LDS -> windowed inverse frame (librosa.istft's ytmp), scaled by `sign`
__device__ __forceinline__ void ens_inverse_frame(float2 *X, float *__restrict__ dstf, const float *__restrict__ window,
                                                  const float2 *__restrict__ tw, const FftPlan &p, float2 *bufA, float2 *bufB,
                                                  float sign) {
  const int nh = p.nh;
  if (threadIdx.x == 0) {
    X[0].y = 0.f;
    X[nh].y = 0.f;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nh; k += blockDim.x) {
    const float2 xk = X[k];
    float2 xc = X[nh - k];
    xc.y = -xc.y;
    const float2 E = make_float2(0.5f * (xk.x + xc.x), 0.5f * (xk.y + xc.y));
    const float2 D = make_float2(0.5f * (xk.x - xc.x), 0.5f * (xk.y - xc.y));
    float2 w = tw[k];
    w.y = -w.y;
    const float2 O = cmul(w, D);
    bufA[k] = make_float2(E.x - O.y, E.y + O.x);
  }
  float2 *z = fft_lds<+1>(bufA, bufB, p, tw);
  const float scale = sign / (float)nh;
  float2 *dst = reinterpret_cast<float2 *>(dstf);
  const float2 *w2 = reinterpret_cast<const float2 *>(window);
  for (int m = threadIdx.x; m < nh; m += blockDim.x) {
    const float2 v = z[m];
    const float2 w = w2[m];
    dst[m] = make_float2((v.x * scale) * w.x, (v.y * scale) * w.y);
  }
}

// *_fft and uvr_*_spec ensembles (ensembler.py:120-156, spec_utils.ensembling :583-607) for frame t of channel ch: the K input
// frames are transformed, combined per bin in LDS and inverse-transformed into frames[ch, t, :] of a [2, T, n_fft] buffer.
// ld(k, q): sample q of that channel of input k.  LDS: bufA, bufB (nh each), cur (nh+1), sel (nh+1), and for the median K * (nh+1) spectra.
template <class Load>
__device__ __forceinline__ void ens_fft_frame(Load ld, int K, int64_t n, int alg, const double *__restrict__ weights, double wsum, int hop,
                                              int t, int ch, int T, float *__restrict__ frames, const float *__restrict__ window,
                                              const float2 *__restrict__ tw, const FftPlan &p, float2 *lds) {
  const int nh = p.nh;
  float2 *bufA = lds, *bufB = lds + nh, *cur = lds + 2 * nh, *sel = cur + (nh + 1), *all = sel + (nh + 1);
  for (int k = 0; k < K; ++k) {
    float2 *dst = (alg == ENS_MEDIAN_FFT) ? all + (size_t)k * (nh + 1) : cur;
    ens_frame_spectrum_of([&](int64_t q) { return ld(k, q); }, n, t, hop, window, tw, p, bufA, bufB, dst);
    if (alg == ENS_MEDIAN_FFT) continue;
    for (int b = threadIdx.x; b <= nh; b += blockDim.x) {
      const float2 x = cur[b];
      if (alg == ENS_AVG_FFT) {
        // ense_spec (complex64) += s * weight (float64 product)
        float2 a = k == 0 ? make_float2(0.f, 0.f) : sel[b];
        a.x = (float)((double)a.x + (double)x.x * weights[k]);
        a.y = (float)((double)a.y + (double)x.y * weights[k]);
        sel[b] = a;
      } else if (k == 0) {
        sel[b] = x;
      } else {
        const float2 s = sel[b];
        const float mx = hypotf(x.x, x.y), ms = hypotf(s.x, s.y);
        bool take;
        if (alg == ENS_MIN_FFT) take = mx < ms;            // np.argmin: first minimum
        else if (alg == ENS_MAX_FFT) take = mx > ms;       // np.argmax: first maximum
        else if (alg == ENS_UVR_MIN_SPEC) take = mx <= ms; // np.where(|new| <= |cur|, new, cur)
        else take = mx >= ms;
        if (take) sel[b] = x;
      }
    }
    __syncthreads();
  }
  if (alg == ENS_MEDIAN_FFT) {
    for (int b = threadIdx.x; b <= nh; b += blockDim.x) {
      float re[ENS_MAX_K], im[ENS_MAX_K];
      for (int k = 0; k < K; ++k) {
        const float2 x = all[(size_t)k * (nh + 1) + b];
        re[k] = x.x;
        im[k] = x.y;
      }
      sel[b] = make_float2(median_small(re, K), median_small(im, K));
    }
  } else if (alg == ENS_AVG_FFT) {
    for (int b = threadIdx.x; b <= nh; b += blockDim.x) {
      const float2 a = sel[b];
      sel[b] = make_float2((float)((double)a.x / wsum), (float)((double)a.y / wsum));
    }
  }
  __syncthreads();
  ens_inverse_frame(sel, frames + ((int64_t)ch * T + t) * p.n_fft, window, tw, p, bufA, bufB, 1.0f);
}

// over a stack [K, 2, n]: grid = (T, 2)
__global__ __launch_bounds__(256) void ens_fft_kernel(const float *__restrict__ waves, int K, int64_t n, int alg,
                                                      const double *__restrict__ weights, double wsum, int hop,
                                                      float *__restrict__ frames, const float *__restrict__ window,
                                                      const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  const int ch = blockIdx.y;
  ens_fft_frame([&](int k, int64_t q) { return waves[((int64_t)k * 2 + ch) * n + q]; }, K, n, alg, weights, wsum, hop, (int)blockIdx.x, ch,
                (int)gridDim.x, frames, window, tw, p, lds);
}

// invert_audio (spec_utils.py:557-571): v = Y - max(|X|, |Y|) * exp(j angle(X)); invert_stem returns -istft(v).  Frame t of one channel
// of n samples -> dst[0 .. n_fft).  ldm(q) / lds_(q): sample q of the mix / of the stem.  LDS: bufA, bufB (nh each), X, Y (nh + 1 each).
template <class LoadMix, class LoadStem>
__device__ __forceinline__ void ens_invert_frame(LoadMix ldm, LoadStem lds_, int64_t n, int t, int hop, float *__restrict__ dst,
                                                 const float *__restrict__ window, const float2 *__restrict__ tw, const FftPlan &p,
                                                 float2 *lds) {
  const int nh = p.nh;
  float2 *bufA = lds, *bufB = lds + nh, *X = lds + 2 * nh, *Y = X + (nh + 1);
  ens_frame_spectrum_of(ldm, n, t, hop, window, tw, p, bufA, bufB, X);
  ens_frame_spectrum_of(lds_, n, t, hop, window, tw, p, bufA, bufB, Y);
  for (int b = threadIdx.x; b <= nh; b += blockDim.x) {
    const float2 x = X[b], y = Y[b];
    const float xm = hypotf(x.x, x.y), ym = hypotf(y.x, y.y);
    const float mm = xm >= ym ? xm : ym;
    const float ang = atan2f(x.y, x.x);
    Y[b] = make_float2(y.x - mm * cosf(ang), y.y - mm * sinf(ang));
  }
  __syncthreads();
  ens_inverse_frame(Y, dst, window, tw, p, bufA, bufB, -1.0f);
}
// over planar mix and stem [2, n]: grid = (T, 2), frames [2, T, n_fft]
__global__ __launch_bounds__(256) void ens_invert_kernel(const float *__restrict__ mix, const float *__restrict__ stem, int64_t n,
                                                         int hop, float *__restrict__ frames, const float *__restrict__ window,
                                                         const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  const int t = blockIdx.x, ch = blockIdx.y, T = gridDim.x;
  const float *x = mix + (int64_t)ch * n, *y = stem + (int64_t)ch * n;
  ens_invert_frame([&](int64_t q) { return x[q]; }, [&](int64_t q) { return y[q]; }, n, t, hop, frames + ((int64_t)ch * T + t) * p.n_fft,
                   window, tw, p, lds);
}

// ---- a pool of (file, stem group) jobs: asx_ensemble_batch_dev ---------------------------------------------------------------
// Every stage of the combine is ONE launch over all jobs: a workgroup finds its job in the job table (its first workgroup / first
// frame in that launch's grid, ascending; a job that takes no part in a stage owns no workgroups there) and then runs the device
// functions above -- the ones the single-job kernels run.  No [K, 2, n_max] stack exists: a contributor's sample is read from
// the member's stem and goes through ens_slot_value, the function ens_slot_kernel stores the stack with, so what a combine
// reads is the float that kernel would have stored and a load would have returned (a float32 store and load change no bit, and
// no arithmetic of the combine can be contracted with the quantiser's: its last operation is a multiplication formed with
// contraction off -- exact, by a power of two, in the integer modes -- whose result is a value like a loaded one to the combine).
// The slot mode belongs to the contributor: the members of one ensemble can write the same file's stems in different formats.
struct EnsPoolSrc {
  const float *stem;   // planar [2, n] or rows [n, 2]
  int64_t n;
  int32_t rows;
  int32_t peak;        // its word of the peak array
  int32_t mode;        // ENS_SLOT_*: its member's file round trip
  int32_t pad_;
};
struct EnsPoolJob {
  EnsPoolSrc src[ENS_MAX_K];   // the contributors that take part, in order
  double w[ENS_MAX_K];         // their weights (avg_*)
  double wsum;
  float *out;                  // planar [2, n_out]
  int64_t n_max, n_out;
  int64_t wave_blk0, fold_blk0, frame0;
  int32_t K, T, pick, pad_;
};
struct EnsSlotEdge {           // the member -> Ensembler edge of the call
  const unsigned int *peaks;   // max |stem| of every contributor, float bits
  float max_peak, min_peak;
  int32_t has_min, pad_;
};

__device__ __forceinline__ float ens_pool_load(const EnsPoolSrc &s, const EnsSlotEdge &ed, int ch, int64_t i) {
  const float maxv = (s.mode != ENS_SLOT_FLOAT32 && i < s.n) ? __uint_as_float(ed.peaks[s.peak]) : 0.f;
  return ens_slot_value(s.stem, s.n, s.rows, ch, i, maxv, ed.max_peak, ed.min_peak, ed.has_min, s.mode);
}

// the last job whose first workgroup (or frame) of this stage is <= x
template <class Job, int64_t Job::*FIRST>
__device__ __forceinline__ int ens_pool_find(const Job *__restrict__ jobs, int n_jobs, int64_t x) {
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].*FIRST <= x) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// max |x| of every contributor of every job: grid = (workgroups per contributor, contributors); peaks cleared before
__global__ __launch_bounds__(256) void ens_pool_peak_kernel(const EnsPoolSrc *__restrict__ srcs, unsigned int *__restrict__ peaks) {
  const EnsPoolSrc s = srcs[blockIdx.y];
  if ((int64_t)blockIdx.x * 256 >= 2 * s.n) return;   // (the whole workgroup: nothing of this stem is in its share)
  absmax_block(s.stem, 2 * s.n, blockIdx.x, gridDim.x, peaks + s.peak);
}

// results formed per sample: the wave algorithms, ensemble_wav's row copy (sel [n_jobs, 2]) and a lone contributor's slot image
__global__ __launch_bounds__(256) void ens_pool_wave_kernel(const EnsPoolJob *__restrict__ jobs, int n_jobs, int alg, EnsSlotEdge ed,
                                                            const int *__restrict__ sel) {
  const int j = ens_pool_find<EnsPoolJob, &EnsPoolJob::wave_blk0>(jobs, n_jobs, blockIdx.x);
  const EnsPoolJob &jb = jobs[j];
  const int64_t N = jb.n_out;
  const int64_t i = ((int64_t)blockIdx.x - jb.wave_blk0) * 256 + threadIdx.x;
  if (i >= 2 * N) return;
  const int ch = i >= N ? 1 : 0;
  const int64_t q = i - (int64_t)ch * N;
  float v;
  if (jb.K == 1) v = ens_pool_load(jb.src[0], ed, ch, q);
  else if (alg == ENS_ENSEMBLE_WAV) v = ens_pool_load(jb.src[sel[2 * j + ch]], ed, ch, q);
  else v = ens_wave_combine([&](int k) { return ens_pool_load(jb.src[k], ed, ch, q); }, jb.K, alg, jb.w, jb.wsum);
  jb.out[i] = v;
}

// ensemble_wav, steps 1 and 2.  grid = (ENS_ABS_BLOCKS * n_jobs, 2 * ENS_MAX_K): the single call's ENS_ABS_BLOCKS strided partial sums
// per (input, channel) of every job, partial [n_jobs, 2 * ENS_MAX_K, ENS_ABS_BLOCKS]; then one workgroup per job.
__global__ __launch_bounds__(256) void ens_pool_abssum_kernel(const EnsPoolJob *__restrict__ jobs, EnsSlotEdge ed, double *__restrict__ partial) {
  const int j = blockIdx.x / ENS_ABS_BLOCKS, bx = blockIdx.x % ENS_ABS_BLOCKS, kc = blockIdx.y;
  const EnsPoolJob &jb = jobs[j];
  if (!jb.pick || kc >= 2 * jb.K) return;
  const int k = kc >> 1, ch = kc & 1;
  ens_abssum_block([&](int64_t i) { return ens_pool_load(jb.src[k], ed, ch, i); }, jb.n_max, bx, ENS_ABS_BLOCKS,
                   partial + ((int64_t)j * 2 * ENS_MAX_K + kc) * ENS_ABS_BLOCKS + bx);
}
__global__ void ens_pool_pick_kernel(const EnsPoolJob *__restrict__ jobs, const double *__restrict__ partial, int *__restrict__ sel) {
  const int j = blockIdx.x, ch = threadIdx.x;
  if (ch >= 2 || !jobs[j].pick) return;
  sel[2 * j + ch] = ens_pick_channel(partial + (int64_t)j * 2 * ENS_MAX_K * ENS_ABS_BLOCKS, jobs[j].K, ENS_ABS_BLOCKS, ch);
}

// *_fft and uvr_*_spec: grid = (frames of all jobs, 2); job j's inverse frames are [2, T_j, n_fft] from frame0_j * 2 * n_fft of `frames`
__global__ __launch_bounds__(256) void ens_pool_fft_kernel(const EnsPoolJob *__restrict__ jobs, int n_jobs, int alg, int hop, EnsSlotEdge ed,
                                                           float *__restrict__ frames, const float *__restrict__ window,
                                                           const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  const EnsPoolJob &jb = jobs[ens_pool_find<EnsPoolJob, &EnsPoolJob::frame0>(jobs, n_jobs, blockIdx.x)];
  const int t = (int)((int64_t)blockIdx.x - jb.frame0), ch = blockIdx.y;
  ens_fft_frame([&](int k, int64_t q) { return ens_pool_load(jb.src[k], ed, ch, q); }, jb.K, jb.n_max, alg, jb.w, jb.wsum, hop, t, ch, jb.T,
                frames + jb.frame0 * 2 * p.n_fft, window, tw, p, lds);
}

// librosa.istft's fold of every job's frames (vr_ola_kernel's sums) with the window-sum-square formed here: position m is covered by
// at most n_fft / hop frames; their squared window values are added in float64 in ascending frame order and rounded to float32
// once -- the value the single call's host table holds there (0 where no frame reaches).
__global__ __launch_bounds__(256) void ens_pool_fold_kernel(const EnsPoolJob *__restrict__ jobs, int n_jobs, const float *__restrict__ frames,
                                                            const float *__restrict__ window, int n_fft, int hop) {
  const EnsPoolJob &jb = jobs[ens_pool_find<EnsPoolJob, &EnsPoolJob::fold_blk0>(jobs, n_jobs, blockIdx.x)];
  const int64_t len = jb.n_out;
  const int64_t i = ((int64_t)blockIdx.x - jb.fold_blk0) * 256 + threadIdx.x;
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
  jb.out[i] = ola_sample(fr, n_fft, hop, m, t_lo, t_hi, s);
  jb.out[len + i] = ola_sample(fr + (int64_t)jb.T * n_fft, n_fft, hop, m, t_lo, t_hi, s);
}

// ---- invert_stem on arrays in HBM: asx_invert_stem_dev and its pooled form asx_invert_stem_batch_dev ---------------------------
// The mix is planar [2, n]; the stem is planar or rows [n, 2] and is scaled as it is read (MDXSeparator hands over
// primary * compensate); the result is rows [n_out, 2], n_out = hop * (T - 1).  Two stages -- ens_invert_frame per (frame, channel),
// then the fold -- each ONE launch: the single form passes its song by value, the pooled form finds a workgroup's song in a device
// table (its first frame / first fold workgroup of the launch, ascending; only songs of at least two frames are in it).  Both run
// ens_invert_song_frame / ens_invert_song_fold, so a song's bits do not depend on the form or on its neighbours.
struct EnsInvSong {
  const float *mix;            // planar [2, n]
  const float *stem;           // planar [2, n] or rows [n, 2]
  float *out;                  // rows [n_out, 2]
  int64_t n, n_out;
  int64_t frame0, fold_blk0;   // its first frame / fold workgroup in the launch; its inverse frames are [2, T, n_fft] from frame0 * 2 * n_fft
  int32_t T, rows;
};

// sample q of channel ch of the stem, times `scale`: numpy's float32 (primary * compensate), one rounding.  What follows is the product
// with the window -- a multiplication, so there is no addition this one could be contracted with; contraction is off all the same.
__device__ __forceinline__ float ens_invert_stem_value(const EnsInvSong &sg, int ch, int64_t q, float scale) {
#pragma clang fp contract(off)
  const float x = sg.rows ? sg.stem[2 * q + ch] : sg.stem[(int64_t)ch * sg.n + q];
  return x * scale;
}

__device__ __forceinline__ void ens_invert_song_frame(const EnsInvSong &sg, int t, int ch, float scale, int hop, float *__restrict__ frames,
                                                      const float *__restrict__ window, const float2 *__restrict__ tw, const FftPlan &p,
                                                      float2 *lds) {
  const float *x = sg.mix + (int64_t)ch * sg.n;
  ens_invert_frame([&](int64_t q) { return x[q]; }, [&](int64_t q) { return ens_invert_stem_value(sg, ch, q, scale); }, sg.n, t, hop,
                   frames + ((sg.frame0 * 2 + (int64_t)ch * sg.T) + t) * p.n_fft, window, tw, p, lds);
}

// ens_pool_fold_kernel's fold (the single host call's vr_ola_kernel sums over the window-sum-square formed here), written as rows
__device__ __forceinline__ void ens_invert_song_fold(const EnsInvSong &sg, int64_t blk, const float *__restrict__ frames,
                                                     const float *__restrict__ window, int n_fft, int hop) {
  const int64_t len = sg.n_out;
  const int64_t i = (blk - sg.fold_blk0) * 256 + threadIdx.x;
  if (i >= len) return;
  const int64_t m = i + n_fft / 2;
  int64_t t_lo, t_hi;
  ola_frame_range(m, n_fft, hop, sg.T, &t_lo, &t_hi);
  double ss = 0.0;
  for (int64_t t = t_lo; t <= t_hi; ++t) {
    const double w = (double)window[m - t * hop];
    ss += w * w;
  }
  const float s = (float)ss;
  const float *fr = frames + sg.frame0 * 2 * n_fft;
  sg.out[2 * i] = ola_sample(fr, n_fft, hop, m, t_lo, t_hi, s);
  sg.out[2 * i + 1] = ola_sample(fr + (int64_t)sg.T * n_fft, n_fft, hop, m, t_lo, t_hi, s);
}

// one song: grid = (T, 2), then ((n_out + 255) / 256)
__global__ __launch_bounds__(256) void ens_invert_dev_kernel(EnsInvSong sg, float scale, int hop, float *__restrict__ frames,
                                                             const float *__restrict__ window, const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  ens_invert_song_frame(sg, (int)blockIdx.x, (int)blockIdx.y, scale, hop, frames, window, tw, p, lds);
}
__global__ __launch_bounds__(256) void ens_invert_dev_fold_kernel(EnsInvSong sg, const float *__restrict__ frames,
                                                                  const float *__restrict__ window, int n_fft, int hop) {
  ens_invert_song_fold(sg, blockIdx.x, frames, window, n_fft, hop);
}

// a pool of songs: grid = (frames of all songs, 2), then (fold workgroups of all songs)
__global__ __launch_bounds__(256) void ens_invert_pool_kernel(const EnsInvSong *__restrict__ songs, int n_songs, float scale, int hop,
                                                              float *__restrict__ frames, const float *__restrict__ window,
                                                              const float2 *__restrict__ tw, FftPlan p) {
  extern __shared__ float2 lds[];
  const EnsInvSong &sg = songs[ens_pool_find<EnsInvSong, &EnsInvSong::frame0>(songs, n_songs, blockIdx.x)];
  ens_invert_song_frame(sg, (int)((int64_t)blockIdx.x - sg.frame0), (int)blockIdx.y, scale, hop, frames, window, tw, p, lds);
}
__global__ __launch_bounds__(256) void ens_invert_pool_fold_kernel(const EnsInvSong *__restrict__ songs, int n_songs,
                                                                   const float *__restrict__ frames, const float *__restrict__ window,
                                                                   int n_fft, int hop) {
  const EnsInvSong &sg = songs[ens_pool_find<EnsInvSong, &EnsInvSong::fold_blk0>(songs, n_songs, blockIdx.x)];
  ens_invert_song_fold(sg, blockIdx.x, frames, window, n_fft, hop);
}

}  // namespace asx
