// Writer edge of write_audio_soundfile (common_separator.py:399-461) for a stem that is still in HBM: spec_utils.normalize, then the samples
// in the file's own format, interleaved [n, 2] -- exactly the body of a WAVE file's data chunk (asx_pcm_encode_dev).
//   integer PCM of b bits: clip(rint((double)x * (2^(b-1) - 1)), -2^(b-1), 2^(b-1) - 1), ties to even: the rule of audio_io.write_wav (and
//                          libsndfile's scale factor), not pcm16_kernel's truncating float32 product
//   float32:               the normalised value
// The normalisation is normalize_kernel's: float32, one rounding per operation, the product only when the peak is outside the thresholds.
// The kernel moves 8 bytes in and 4 .. 8 out per frame and does nothing else, so it is bound by HBM traffic: a lane takes a group of four
// frames -- float4 loads on either layout where the row is 16-byte aligned -- and stores whole dwords: 16 bytes of PCM_16, 24 of PCM_24
// (four 6-byte frames: the only group size at which packed 24-bit frames end on a dword), 32 of the 4-byte formats.  The last group may hold
// fewer than four frames and goes out bytewise.
#pragma once

constexpr int PCMENC_S16 = 16, PCMENC_S24 = 24, PCMENC_S32 = 32, PCMENC_F32 = 0x120;
constexpr int PCMENC_S16_IN_32 = 0x410, PCMENC_S24_IN_32 = 0x418;   // int32 containers: the input of flac_encode_kernel<true>

static inline bool pcmenc_known(int fmt) {
  return fmt == PCMENC_S16 || fmt == PCMENC_S24 || fmt == PCMENC_S32 || fmt == PCMENC_F32 || fmt == PCMENC_S16_IN_32 || fmt == PCMENC_S24_IN_32;
}
static inline int pcmenc_frame_bytes(int fmt) { return fmt == PCMENC_S16 ? 4 : fmt == PCMENC_S24 ? 6 : 8; }

// the integer sample of `bits` bits for the normalised x
template <int BITS>
__device__ __forceinline__ int pcmenc_quant(float x) {
  constexpr double full = (double)((1ll << (BITS - 1)) - 1);
  const double q = fmin(fmax(rint((double)x * full), -full - 1.0), full);
  return (int)q;
}

// FMT: one of the codes above; ROWS: the stem is [n, 2], else planar [2, n]; VEC: the rows the group reads are 16-byte aligned
template <int FMT, bool ROWS, bool VEC>
__global__ __launch_bounds__(256) void pcm_encode_kernel(const float *__restrict__ stem, int64_t n, const unsigned int *peak_bits, float max_peak,
                                                         float min_peak, int has_min, unsigned char *__restrict__ out) {
#pragma clang fp contract(off)
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // group of frames 4 g .. 4 g + 3
  const int64_t f0 = 4 * g;
  if (f0 >= n) return;
  const float maxv = __uint_as_float(*peak_bits);
  float scale = 1.0f;
  bool scaled = false;
  if (maxv > max_peak) {
    scale = __fdiv_rn(max_peak, maxv);
    scaled = true;
  } else if (has_min && maxv < min_peak) {
    scale = __fdiv_rn(min_peak, maxv);
    scaled = true;
  }
  const int cnt = (n - f0) < 4 ? (int)(n - f0) : 4;
  float v[8];                                          // interleaved: frame j's left at 2 j, right at 2 j + 1
  if (cnt == 4 && VEC) {
    if (ROWS) {
      const float4 a = *reinterpret_cast<const float4 *>(stem + 2 * f0), b = *reinterpret_cast<const float4 *>(stem + 2 * f0 + 4);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
      const float4 l = *reinterpret_cast<const float4 *>(stem + f0), r = *reinterpret_cast<const float4 *>(stem + n + f0);
      v[0] = l.x, v[2] = l.y, v[4] = l.z, v[6] = l.w, v[1] = r.x, v[3] = r.y, v[5] = r.z, v[7] = r.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool in = j < cnt;
      v[2 * j] = in ? (ROWS ? stem[2 * (f0 + j)] : stem[f0 + j]) : 0.f;
      v[2 * j + 1] = in ? (ROWS ? stem[2 * (f0 + j) + 1] : stem[n + f0 + j]) : 0.f;
    }
  }
  if (scaled) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = v[j] * scale;
  }
  constexpr int FB = FMT == PCMENC_S16 ? 4 : FMT == PCMENC_S24 ? 6 : 8;   // bytes per frame
  uint32_t w[8];                                       // the group's bytes as little-endian dwords: FB of them
  if (FMT == PCMENC_F32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = __float_as_uint(v[j]);
  } else if (FMT == PCMENC_S32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (uint32_t)pcmenc_quant<32>(v[j]);
  } else if (FMT == PCMENC_S24_IN_32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (uint32_t)pcmenc_quant<24>(v[j]);
  } else if (FMT == PCMENC_S16_IN_32) {
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = (uint32_t)pcmenc_quant<16>(v[j]);
  } else if (FMT == PCMENC_S16) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      w[j] = ((uint32_t)pcmenc_quant<16>(v[2 * j]) & 0xffffu) | ((uint32_t)pcmenc_quant<16>(v[2 * j + 1]) << 16);
  } else {                                             // packed 24-bit: four samples s0 .. s3 fill three dwords
    uint32_t s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = (uint32_t)pcmenc_quant<24>(v[j]) & 0xffffffu;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      w[3 * h] = s[4 * h] | (s[4 * h + 1] << 24);
      w[3 * h + 1] = (s[4 * h + 1] >> 8) | (s[4 * h + 2] << 16);
      w[3 * h + 2] = (s[4 * h + 2] >> 16) | (s[4 * h + 3] << 8);
    }
  }
  unsigned char *o = out + f0 * FB;                    // 4 FB bytes per group: 16-byte aligned at 16 and 32, 8-byte at 24 (out is 16-byte aligned)
  if (cnt == 4) {
    if (FB == 4) {
      *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (FB == 6) {
      *reinterpret_cast<uint2 *>(o) = make_uint2(w[0], w[1]);
      *reinterpret_cast<uint2 *>(o + 8) = make_uint2(w[2], w[3]);
      *reinterpret_cast<uint2 *>(o + 16) = make_uint2(w[4], w[5]);
    } else {
      *reinterpret_cast<uint4 *>(o) = make_uint4(w[0], w[1], w[2], w[3]);
      *reinterpret_cast<uint4 *>(o + 16) = make_uint4(w[4], w[5], w[6], w[7]);
    }
  } else {                                             // the stream's last one to three frames
    const int nbytes = cnt * FB;
    for (int b = 0; b < nbytes; ++b) o[b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
  }
}

template <int FMT>
static void pcm_encode_launch(const float *stem, int64_t n, int rows, const unsigned int *pk, float max_peak, float min_peak, int has_min,
                              unsigned char *out, hipStream_t s) {
  const unsigned nb = (unsigned)(((n + 3) / 4 + 255) / 256);
  // planar: the right row begins n floats behind the left one
  const bool vec = (((uintptr_t)stem) & 15) == 0 && (rows || (n & 3) == 0);
  if (rows) {
    if (vec) hipLaunchKernelGGL((pcm_encode_kernel<FMT, true, true>), dim3(nb), dim3(256), 0, s, stem, n, pk, max_peak, min_peak, has_min, out);
    else hipLaunchKernelGGL((pcm_encode_kernel<FMT, true, false>), dim3(nb), dim3(256), 0, s, stem, n, pk, max_peak, min_peak, has_min, out);
  } else {
    if (vec) hipLaunchKernelGGL((pcm_encode_kernel<FMT, false, true>), dim3(nb), dim3(256), 0, s, stem, n, pk, max_peak, min_peak, has_min, out);
    else hipLaunchKernelGGL((pcm_encode_kernel<FMT, false, false>), dim3(nb), dim3(256), 0, s, stem, n, pk, max_peak, min_peak, has_min, out);
  }
}
