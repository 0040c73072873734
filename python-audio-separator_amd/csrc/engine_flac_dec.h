// Engine side of the FLAC decoder (included by asx.hip only): the launches of kernels_flac_dec.h around the chain walk of flac_dec_plan.h.
// scan: flac_sync_kernel, the candidate count to the host (the slots [candidate][2][max_blocksize] are sized by it: at the list's capacity
// they would be terabytes), flac_frame_kernel, the records to the host, the walk, the chain's frames back to the device.  finish:
// flac_finish_kernel over those frames.
#pragma once

static int flac_decode_scan_launch(asx_engine *e, const uint8_t *audio, int64_t nbytes, const flacdec::Info &I, const FlacDecPlan &plan,
                                   int64_t *n_samples, int64_t *n_frames, int64_t *bytes_consumed, hipStream_t s) {
  static_assert(sizeof(FlacDecRec) == flacdec::REC_WORDS * 4, "the record as the kernel writes it");
  e->flacdec_n_samples = -1;
  CHK(e->flacdec_list.ensure(16 + (size_t)plan.max_candidates * 4));
  uint32_t *count = reinterpret_cast<uint32_t *>(e->flacdec_list.p);
  uint32_t *cand = count + 4;
  HIPCHK(hipMemsetAsync(count, 0, 16, s));
  const unsigned nb = (unsigned)std::min<int64_t>((nbytes + flacdec::SYNC_THREADS - 1) / flacdec::SYNC_THREADS, 8192);
  CHK(timed(e, ASX_PROF_MISC, 0.0, (double)nbytes, s, [&]() {
    hipLaunchKernelGGL(flacdec::flac_sync_kernel, dim3(nb), dim3(flacdec::SYNC_THREADS), 0, s, audio, nbytes, I, count, cand, (uint32_t)plan.max_candidates);
  }));
  uint32_t nc = 0;
  HIPCHK(hipMemcpyAsync(&nc, count, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  REQUIRE((int64_t)nc <= plan.max_candidates, "asx_flac_decode_scan_dev: %u frame headers in %lld bytes", nc, (long long)nbytes);
  FlacDecChain chain;
  if (nc > 0) {
    const size_t rec_bytes = ((size_t)nc * sizeof(FlacDecRec) + 15) / 16 * 16;
    CHK(e->flacdec_slots.ensure(rec_bytes + (size_t)nc * (size_t)plan.slot_bytes));
    e->flacdec_slot_off = rec_bytes;
    int32_t *recs = reinterpret_cast<int32_t *>(e->flacdec_slots.p);
    int32_t *slots = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(e->flacdec_slots.p) + rec_bytes);
    const int lds = flacdec::lds_bytes(I.max_blocksize);
    grant_lds(&flacdec::flac_frame_kernel, lds);
    CHK(timed(e, ASX_PROF_MISC, 0.0, (double)nbytes, s, [&]() {
      hipLaunchKernelGGL(flacdec::flac_frame_kernel, dim3(nc), dim3(flacdec::NT), lds, s, audio, (uint32_t)nbytes, I, cand, slots, recs);
    }));
    std::vector<FlacDecRec> host(nc);
    HIPCHK(hipMemcpyAsync(host.data(), recs, (size_t)nc * sizeof(FlacDecRec), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    flac_dec_chain(host.data(), (int64_t)nc, nbytes, chain);
    e->flacdec_accept_host.resize(chain.links.size());
    for (size_t i = 0; i < chain.links.size(); ++i) {
      const FlacDecRec &r = host[(size_t)chain.links[i].index];
      e->flacdec_accept_host[i] = flacdec::Accept{chain.links[i].index, r.blocksize, r.assignment, 0, chain.links[i].out};
    }
    if (!chain.links.empty()) {
      const size_t bytes = chain.links.size() * sizeof(flacdec::Accept);
      CHK(e->flacdec_accept.ensure(bytes));
      HIPCHK(hipMemcpyAsync(e->flacdec_accept.p, e->flacdec_accept_host.data(), bytes, hipMemcpyHostToDevice, s));
    }
  }
  e->flacdec_n_samples = chain.n_samples;
  e->flacdec_n_frames = chain.n_frames;
  e->flacdec_channels = I.channels;
  e->flacdec_bps = I.bps;
  e->flacdec_max_bs = I.max_blocksize;
  *n_samples = chain.n_samples;
  if (n_frames) *n_frames = chain.n_frames;
  if (bytes_consumed) *bytes_consumed = chain.bytes_consumed;
  return ASX_OK;
}

static int flac_decode_finish_launch(asx_engine *e, float *mix, int64_t n, float *peak, hipStream_t s) {
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p) + 1;   // asx_pcm_decode_dev's word
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const int32_t *slots = reinterpret_cast<const int32_t *>(reinterpret_cast<const unsigned char *>(e->flacdec_slots.p) + e->flacdec_slot_off);
  const float scale = 1.0f / (float)(1 << (e->flacdec_bps - 1));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 16.0 * (double)n, s, [&]() {
    hipLaunchKernelGGL(flacdec::flac_finish_kernel, dim3((unsigned)e->flacdec_n_frames), dim3(flacdec::FINISH_THREADS), 0, s, slots,
                       reinterpret_cast<const flacdec::Accept *>(e->flacdec_accept.p), (int)e->flacdec_max_bs, (int)e->flacdec_channels, scale, n, mix, pk);
  }));
  if (peak) {
    HIPCHK(hipMemcpyAsync(peak, pk, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return ASX_OK;
}
