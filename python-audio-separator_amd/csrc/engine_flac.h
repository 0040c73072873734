// Engine side of the FLAC encoder (included by asx.hip only): the plan of a stream, pure host, and the three launches of
// kernels_flac.h -- encode into fixed-stride slots, scan the frame sizes, compact -- on the engine's scratch.
#pragma once

struct FlacPlan {
  int64_t n_blocks = 0;
  int32_t stride = 0;        // bytes per frame slot (worst case of a full block, rounded up to 16)
  int64_t max_bytes = 0;     // worst case of the compacted frames
  int64_t scratch_bytes = 0; // slots + offsets
};

// empty string, or why the stream is refused.  pcm: the int32 form (asx_flac_encode_pcm*), whose side channel is bps + 1 bits wide
static std::string flac_plan_make(int64_t n, int channels, int bps, int block_size, FlacPlan &p, bool pcm = false) {
  char buf[200];
  if (channels != 2) {
    snprintf(buf, sizeof buf, "%d channels (the encoder writes stereo streams only)", channels);
    return buf;
  }
  if (bps != 16 && bps != 24) {
    snprintf(buf, sizeof buf, pcm ? "%d bits per sample (int32 samples of 16 or 24 bits)" : "%d bits per sample (16, or 24 = the 16-bit value shifted left by 8)",
             bps);
    return buf;
  }
  if (block_size < flac::MIN_BLOCK || block_size > flac::MAX_BLOCK) {
    snprintf(buf, sizeof buf, "block size %d outside %d .. %d (the streamable subset's range at rates up to 48 kHz)", block_size, flac::MIN_BLOCK,
             flac::MAX_BLOCK);
    return buf;
  }
  if (n < 1) return "no samples";
  p.n_blocks = (n + block_size - 1) / block_size;
  if (p.n_blocks >= ((int64_t)1 << 31)) return "more than 2^31 - 1 frames";
  const int side = pcm ? bps + 1 : flac::SIDE_BITS;
  p.stride = flac::frame_stride(block_size, side);
  const int64_t last = n - (p.n_blocks - 1) * block_size;
  p.max_bytes = (p.n_blocks - 1) * flac::worst_frame_bytes(block_size, side) + flac::worst_frame_bytes(last, side);
  p.scratch_bytes = p.n_blocks * (int64_t)p.stride + (p.n_blocks + 1) * 8;
  return "";
}

// PCM: `pcm` is int32 [n, 2] (samples of bps real bits), else int16 [n, 2]
template <bool PCM>
static int flac_encode_launch(asx_engine *e, const void *pcm, int64_t n, int sample_rate, int bps, int block_size, const FlacPlan &p,
                              uint8_t *out, int32_t *frame_bytes, int64_t *total, hipStream_t s) {
  CHK(e->flac_frames.ensure((size_t)p.n_blocks * (size_t)p.stride));
  CHK(e->flac_off.ensure((size_t)(p.n_blocks + 1) * 8));
  flac::Stream st{};
  st.pcm = static_cast<const int32_t *>(pcm);
  st.n = n;
  st.block_size = block_size;
  st.bps = bps;
  flac::sample_rate_code(sample_rate, &st.sr_code, &st.sr_extra_bits, &st.sr_extra);
  st.stride = p.stride;
  st.frames = reinterpret_cast<uint8_t *>(e->flac_frames.p);
  st.frame_bytes = frame_bytes;
  int64_t *off = reinterpret_cast<int64_t *>(e->flac_off.p);
  if (e->prof) {             // with the profile on, lane 0 of every block stamps its shader clock: asx_counter "flac_block_cycles" / "flac_crc16_cycles"
    CHK(e->flac_cycles.ensure(16));
    HIPCHK(hipMemsetAsync(e->flac_cycles.p, 0, 16, s));
    st.cycles = reinterpret_cast<unsigned long long *>(e->flac_cycles.p);
  }
  grant_lds(&flac::flac_encode_kernel<PCM>, flac::lds_bytes(PCM));
  CHK(timed(e, ASX_PROF_MISC, 0.0, (PCM ? 8.0 : 4.0) * (double)n, s, [&]() {
    hipLaunchKernelGGL(flac::flac_encode_kernel<PCM>, dim3((unsigned)p.n_blocks), dim3(flac::NT), flac::lds_bytes(PCM), s, st);
  }));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 12.0 * (double)p.n_blocks, s, [&]() {
    hipLaunchKernelGGL(flac::flac_scan_kernel, dim3(1), dim3(flac::SCAN_THREADS), 0, s, frame_bytes, p.n_blocks, off);
  }));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 2.0 * (double)p.max_bytes, s, [&]() {
    hipLaunchKernelGGL(flac::flac_compact_kernel, dim3((unsigned)p.n_blocks), dim3(flac::COMPACT_THREADS), 0, s, st.frames, p.stride, frame_bytes, off, out);
  }));
  HIPCHK(hipMemcpyAsync(total, off + p.n_blocks, 8, hipMemcpyDeviceToHost, s));
  unsigned long long cyc[2] = {0, 0};
  if (st.cycles) HIPCHK(hipMemcpyAsync(cyc, st.cycles, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  e->flac_block_cycles += (long long)cyc[0];
  e->flac_crc16_cycles += (long long)cyc[1];
  return ASX_OK;
}
