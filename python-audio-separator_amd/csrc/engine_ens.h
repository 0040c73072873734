// Spectral edges: Ensembler.ensemble and spec_utils.invert_stem on the engine (kernels_ens.h).  Included by asx.hip.
#pragma once
#include "ens_pool_plan.h"

// pinned host staging of the pooled call's tables: what an asynchronous copy reads must stay put until the copy has run
struct PinBuf {
  void *p = nullptr;
  size_t bytes = 0;
  int ensure(size_t n) {
    if (n <= bytes) return ASX_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
    HIPCHK(hipHostMalloc(&p, n, hipHostMallocDefault));
    bytes = n;
    return ASX_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

struct EnsCtx {
  FftPlan plan{};
  DevBuf window, tw, frames, wss, dweights, din, din2, dout, partial, sel;
  // asx_ensemble_batch_dev: contributor table, peaks, job table, ensemble_wav's sums and choices; their host staging and the event
  // behind the last copy out of it
  DevBuf psrcs, ppeaks, pjobs, ppartial, psel;
  DevBuf isongs;   // asx_invert_stem_batch_dev: song table (staged like the job table)
  PinBuf stage;
  hipEvent_t staged = nullptr;
  bool ready = false;
};

static void ens_destroy(EnsCtx *c) {
  for (DevBuf *b : {&c->window, &c->tw, &c->frames, &c->wss, &c->dweights, &c->din, &c->din2, &c->dout, &c->partial, &c->sel, &c->psrcs,
                    &c->ppeaks, &c->pjobs, &c->ppartial, &c->psel, &c->isongs})
    b->release();
  if (c->staged) {
    (void)hipEventSynchronize(c->staged);
    (void)hipEventDestroy(c->staged);
  }
  c->stage.release();
  delete c;
}

static int ens_ctx(asx_engine *e) {
  if (!e->ens) e->ens = new EnsCtx();
  EnsCtx &c = *e->ens;
  if (c.ready) return ASX_OK;
  const int n_fft = 2048;
  REQUIRE(make_plan(n_fft, &c.plan), "n_fft 2048 plan");
  std::vector<float> w;
  host_window(n_fft, w);
  CHK(ht_up(c.window, w));
  std::vector<float> tw((size_t)n_fft * 2);
  for (int j = 0; j < n_fft; ++j) {
    const double ang = -2.0 * M_PI * (double)j / (double)n_fft;
    tw[2 * j] = (float)cos(ang);
    tw[2 * j + 1] = (float)sin(ang);
  }
  CHK(ht_up(c.tw, tw));
  const int lds = (int)(((size_t)c.plan.nh * 2 + (size_t)(c.plan.nh + 1) * (2 + ENS_MAX_K)) * sizeof(float2));
  // median_fft needs 65,584 B of dynamic LDS at K = 4 and 98,384 B at K = 8: a refused raise is an error here, not a failed launch later.
  // Per engine (= per device), so not through the process-wide grant_lds record.
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&ens_fft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&ens_invert_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&ens_pool_fft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  // The invert kernels on device arrays hold two spectra: 32,784 B, inside the limit every device starts with.  They need no raise on
  // any device, so the process-wide record of grant_lds, which the raises above must avoid, does them no harm: the grant goes through
  // the one guarded path and changes nothing.  Should their LDS ever pass the default limit, they need a per-engine raise as above.
  const int inv_lds = (int)(((size_t)c.plan.nh * 2 + (size_t)(c.plan.nh + 1) * 2) * sizeof(float2));
  grant_lds(&ens_invert_dev_kernel, inv_lds);
  grant_lds(&ens_invert_pool_kernel, inv_lds);
  c.ready = true;
  return ASX_OK;
}

// librosa.istft fold of frames [2, T, 2048] -> out [2, len] (len = N for length=N, hop*(T-1) otherwise); len = 0 writes nothing
static int ens_fold(asx_engine *e, int T, int64_t len, float *out, hipStream_t s) {
  if (len <= 0) return ASX_OK;
  EnsCtx &c = *e->ens;
  const int nf = c.plan.n_fft, hop = 1024;
  std::vector<float> w;
  host_window(nf, w);
  const size_t cover = (size_t)nf + (size_t)hop * (T - 1);
  std::vector<double> ss(std::max(cover, (size_t)len + nf), 0.0);   // zero beyond the frames: those samples stay 0
  for (int t = 0; t < T; ++t)
    for (int k = 0; k < nf; ++k) ss[(size_t)t * hop + k] += (double)w[k] * (double)w[k];
  std::vector<float> ssf(ss.begin(), ss.end());
  CHK(c.wss.ensure(ssf.size() * 4));
  HIPCHK(hipMemcpyAsync(c.wss.p, ssf.data(), ssf.size() * 4, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return timed(e, ASX_PROF_OLA, 0.0, 4.0 * 2 * (T * (double)nf + 2.0 * len), s, [&]() {
    hipLaunchKernelGGL(vr_ola_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, c.frames.f(), c.wss.f(), nf, hop, T, len, 0,
                       (const float *)nullptr, out);
  });
}

static int ens_ensemble_dev(asx_engine *e, const float *waves, int K, int64_t N, int alg, const double *weights_host, float *out,
                            int64_t *n_out, hipStream_t s) {
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  REQUIRE(K >= 2 && K <= ENS_MAX_K, "ensemble of %d inputs (2 .. %d are built)", K, ENS_MAX_K);
  REQUIRE(alg >= ENS_AVG_WAVE && alg <= ENS_ENSEMBLE_WAV, "unknown ensemble algorithm %d", alg);
  if (alg == ENS_ENSEMBLE_WAV) {
    CHK(c.partial.ensure((size_t)K * 2 * ENS_ABS_BLOCKS * 8));
    CHK(c.sel.ensure(16));
    *n_out = N;
    return timed(e, ASX_PROF_MISC, 0.0, 4.0 * (K + 2) * 2 * N, s, [&]() {
      hipLaunchKernelGGL(ens_abssum_kernel, dim3(ENS_ABS_BLOCKS, K * 2), dim3(256), 0, s, waves, N, reinterpret_cast<double *>(c.partial.p));
      hipLaunchKernelGGL(ens_pick_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<const double *>(c.partial.p), K, ENS_ABS_BLOCKS,
                         reinterpret_cast<int *>(c.sel.p));
      hipLaunchKernelGGL(ens_take_kernel, dim3((unsigned)((N + 255) / 256), 2), dim3(256), 0, s, waves, N,
                         reinterpret_cast<const int *>(c.sel.p), out);
    });
  }
  std::vector<double> w(K, 1.0);
  if (weights_host) w.assign(weights_host, weights_host + K);
  double wsum = 0.0;
  for (double v : w) wsum += v;
  CHK(c.dweights.ensure((size_t)K * 8));
  HIPCHK(hipMemcpyAsync(c.dweights.p, w.data(), (size_t)K * 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  const double *dw = reinterpret_cast<const double *>(c.dweights.p);
  if (alg <= ENS_MAX_WAVE) {
    const int64_t n2 = 2 * N;
    *n_out = N;
    return timed(e, ASX_PROF_MISC, 0.0, 4.0 * (K + 1) * n2, s, [&]() {
      hipLaunchKernelGGL(ens_wave_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, s, waves, K, n2, alg, dw, wsum, out);
    });
  }
  const int hop = 1024, nh = c.plan.nh;
  const int T = (int)(1 + N / hop);
  if (alg >= ENS_UVR_MAX_SPEC && T < 2) {   // one frame, no length argument: the reference's istft returns [2, 0]
    *n_out = 0;
    return ASX_OK;
  }
  CHK(c.frames.ensure((size_t)2 * T * c.plan.n_fft * 4));
  const size_t lds = ((size_t)nh * 2 + (size_t)(nh + 1) * (2 + (alg == ENS_MEDIAN_FFT ? K : 0))) * sizeof(float2);
  CHK(timed(e, ASX_PROF_STFT, 0.0, 4.0 * ((double)K * 2 * N + 2.0 * T * c.plan.n_fft), s, [&]() {
    hipLaunchKernelGGL(ens_fft_kernel, dim3(T, 2), dim3(256), lds, s, waves, K, N, alg, dw, wsum, hop, c.frames.f(), c.window.f(),
                       reinterpret_cast<const float2 *>(c.tw.p), c.plan);
  }));
  *n_out = alg >= ENS_UVR_MAX_SPEC ? (int64_t)hop * (T - 1) : N;   // spectrogram_to_wave_no_mp has no length argument
  return ens_fold(e, T, *n_out, out, s);
}

static int ens_invert_dev(asx_engine *e, const float *mix, const float *stem, int64_t N, float *out, int64_t *n_out, hipStream_t s) {
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  const int hop = 1024, nh = c.plan.nh;
  const int T = (int)(1 + N / hop);
  if (T < 2) {   // fewer than 1024 samples: hop * (T - 1) = 0, the reference returns an empty [0, 2]
    *n_out = 0;
    return ASX_OK;
  }
  CHK(c.frames.ensure((size_t)2 * T * c.plan.n_fft * 4));
  const size_t lds = ((size_t)nh * 2 + (size_t)(nh + 1) * 2) * sizeof(float2);
  CHK(timed(e, ASX_PROF_STFT, 0.0, 4.0 * (4.0 * N + 2.0 * T * c.plan.n_fft), s, [&]() {
    hipLaunchKernelGGL(ens_invert_kernel, dim3(T, 2), dim3(256), lds, s, mix, stem, N, hop, c.frames.f(), c.window.f(),
                       reinterpret_cast<const float2 *>(c.tw.p), c.plan);
  }));
  *n_out = (int64_t)hop * (T - 1);
  return ens_fold(e, T, *n_out, out, s);
}

// ---- invert_stem with every array in HBM ----------------------------------------------------------------------------------
// One song of asx_invert_stem_dev / asx_invert_stem_batch_dev, checked: its frame count in *T (1: no result).  `who` names the song
// in the message ("" for the single call).
static int ens_invert_check(const char *fn, const char *who, const float *mix, const float *stem, int64_t N, int layout, const float *out,
                            int64_t capacity, int *T) {
  REQUIRE(mix && stem, "%s: %snull mix or stem", fn, who);
  REQUIRE(N >= 1 && N <= ((int64_t)1 << 38), "%s: %sn_samples %lld (1 .. 2^38)", fn, who, (long long)N);
  REQUIRE(layout == ASX_STEM_PLANAR || layout == ASX_STEM_ROWS, "%s: %sstem layout %d (0 planar [2, n], 1 rows [n, 2])", fn, who, layout);
  *T = (int)(1 + N / ENS_PLAN_HOP);
  const int64_t n_out = (int64_t)ENS_PLAN_HOP * (*T - 1);
  REQUIRE(capacity >= n_out, "%s: %soutput capacity %lld below n_out = %lld", fn, who, (long long)capacity, (long long)n_out);
  REQUIRE(out || n_out == 0, "%s: %snull output", fn, who);
  return ASX_OK;
}

static int ens_invert_stem_dev(asx_engine *e, const float *mix, const float *stem, int64_t N, int layout, float scale, float *out,
                               int64_t capacity, int64_t *n_out, hipStream_t s) {
  int T = 0;
  CHK(ens_invert_check("asx_invert_stem_dev", "", mix, stem, N, layout, out, capacity, &T));
  if (T < 2) {   // fewer than 1024 samples: nothing is launched, as in asx_invert_stem
    *n_out = 0;
    return ASX_OK;
  }
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  const int nf = c.plan.n_fft, nh = c.plan.nh, hop = ENS_PLAN_HOP;
  const EnsInvSong sg{mix, stem, out, N, (int64_t)hop * (T - 1), 0, 0, T, (int32_t)(layout == ASX_STEM_ROWS)};
  CHK(c.frames.ensure((size_t)2 * T * nf * 4));
  const size_t lds = ((size_t)nh * 2 + (size_t)(nh + 1) * 2) * sizeof(float2);
  CHK(timed(e, ASX_PROF_STFT, 0.0, 4.0 * (4.0 * N + 2.0 * T * nf), s, [&]() {
    hipLaunchKernelGGL(ens_invert_dev_kernel, dim3(T, 2), dim3(256), lds, s, sg, scale, hop, c.frames.f(), c.window.f(),
                       reinterpret_cast<const float2 *>(c.tw.p), c.plan);
  }));
  *n_out = sg.n_out;
  return timed(e, ASX_PROF_OLA, 0.0, 4.0 * 2 * (T * (double)nf + sg.n_out), s, [&]() {
    hipLaunchKernelGGL(ens_invert_dev_fold_kernel, dim3((unsigned)((sg.n_out + 255) / 256)), dim3(256), 0, s, sg, (const float *)c.frames.f(),
                       (const float *)c.window.f(), nf, hop);
  });
}

// The same for a list of songs: one table upload, then one launch per stage over the songs of at least two frames.
static int ens_invert_stem_batch_dev(asx_engine *e, asx_invert_song *songs, int n_songs, float scale, hipStream_t s) {
  const char *fn = "asx_invert_stem_batch_dev";
  REQUIRE(n_songs >= 0 && (songs || n_songs == 0), "%s: bad argument (songs %p, n_songs %d)", fn, (void *)songs, n_songs);
  std::vector<EnsInvSong> tab;
  int64_t frames = 0, fold_blocks = 0;
  for (int i = 0; i < n_songs; ++i) {   // nothing is enqueued, and no n_out written, unless every song is valid
    const asx_invert_song &g = songs[i];
    char who[32];
    snprintf(who, sizeof(who), "song %d: ", i);
    int T = 0;
    CHK(ens_invert_check(fn, who, g.mix_dev, g.stem_dev, g.n_samples, (int)g.stem_layout, g.out_dev, g.out_capacity, &T));
    if (T < 2) continue;
    const int64_t n_out = (int64_t)ENS_PLAN_HOP * (T - 1);
    tab.push_back(EnsInvSong{g.mix_dev, g.stem_dev, g.out_dev, g.n_samples, n_out, frames, fold_blocks, T, (int32_t)(g.stem_layout == ASX_STEM_ROWS)});
    frames += T;
    fold_blocks += (n_out + 255) / 256;
    REQUIRE(frames < ((int64_t)1 << 31) && fold_blocks < ((int64_t)1 << 31), "%s: the songs of one call make %lld / %lld workgroups of a stage (2^31 - 1 at most)",
            fn, (long long)frames, (long long)fold_blocks);
  }
  for (int i = 0; i < n_songs; ++i) songs[i].n_out = (int64_t)ENS_PLAN_HOP * (songs[i].n_samples / ENS_PLAN_HOP);
  if (tab.empty()) return ASX_OK;
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  const int nf = c.plan.n_fft, nh = c.plan.nh, hop = ENS_PLAN_HOP, n_tab = (int)tab.size();
  const size_t tab_bytes = tab.size() * sizeof(EnsInvSong);
  if (c.staged) HIPCHK(hipEventSynchronize(c.staged));   // the last call's copies out of the staging area have run
  else HIPCHK(hipEventCreateWithFlags(&c.staged, hipEventDisableTiming));
  CHK(c.stage.ensure(tab_bytes));
  CHK(c.isongs.ensure(tab_bytes));
  CHK(c.frames.ensure((size_t)frames * 2 * nf * 4));
  memcpy(c.stage.p, tab.data(), tab_bytes);
  HIPCHK(hipMemcpyAsync(c.isongs.p, c.stage.p, tab_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(c.staged, s));
  const EnsInvSong *ds = reinterpret_cast<const EnsInvSong *>(c.isongs.p);
  const size_t lds = ((size_t)nh * 2 + (size_t)(nh + 1) * 2) * sizeof(float2);
  CHK(timed(e, ASX_PROF_STFT, 0.0, 4.0 * 2.0 * frames * nf, s, [&]() {
    hipLaunchKernelGGL(ens_invert_pool_kernel, dim3((unsigned)frames, 2), dim3(256), lds, s, ds, n_tab, scale, hop, c.frames.f(), c.window.f(),
                       reinterpret_cast<const float2 *>(c.tw.p), c.plan);
  }));
  return timed(e, ASX_PROF_OLA, 0.0, 4.0 * 2.0 * frames * nf, s, [&]() {
    hipLaunchKernelGGL(ens_invert_pool_fold_kernel, dim3((unsigned)fold_blocks), dim3(256), 0, s, ds, n_tab, (const float *)c.frames.f(),
                       (const float *)c.window.f(), nf, hop);
  });
}

// ---- a pool of (file, stem group) jobs ------------------------------------------------------------------------------------
// What EnsembleSeparator's per-file loop does per job with asx_ensemble_slot_dev and asx_ensemble_dev, for all jobs at once: one
// launch for the peaks of all contributors, one copy and one wait for them, the live sets and the plan on the host
// (ens_pool_plan.h), one table upload, then one launch per stage (kernels_ens.h).  Nothing is launched before every argument has
// been checked.
static float ens_peak_after(float maxv, int mode, float max_peak, float min_peak, int has_min) {   // asx_ensemble_slot_dev's report
  float scale = 1.0f;
  if (mode != ASX_SLOT_FLOAT32) {   // every round trip normalises; asx_pcm_encode_dev reports the same product
    if (maxv > max_peak) scale = max_peak / maxv;
    else if (has_min && maxv < min_peak) scale = min_peak / maxv;
  }
  return maxv * scale;
}

#define ENS_SLOT_MODE_TEXT "0 pcm16 round trip, 1 float32 copy, 16 / 24 / 32 / 0x120 the soundfile writer's PCM_16 / PCM_24 / PCM_32 / FLOAT file"

// modes: [n_jobs][ENS_MAX_K], the slot mode of every contributor (asx_ensemble_batch_modes_dev), or NULL: `mode` for all of them
// (asx_ensemble_batch_dev).  `fn` names the entry point in the messages.
static int ens_ensemble_batch_dev(asx_engine *e, const char *fn, asx_ens_job *jobs, int n_jobs, const int32_t *modes, int alg, const double *weights,
                                  int n_weights, int mode, float max_peak, float min_peak, int has_min, double silent_below, hipStream_t s) {
  REQUIRE(n_jobs >= 0 && (jobs || n_jobs == 0), "%s: bad argument (jobs %p, n_jobs %d)", fn, (void *)jobs, n_jobs);
  REQUIRE(modes || ens_slot_mode_known(mode), "%s: mode %d (" ENS_SLOT_MODE_TEXT ")", fn, mode);
  auto mode_of = [&](int j, int c) { return modes ? (int)modes[(size_t)j * ENS_MAX_K + c] : mode; };
  REQUIRE(n_weights >= 0 && n_weights <= ENS_MAX_K && (weights || n_weights == 0), "%s: %d weights (0 .. %d)", fn, n_weights, ENS_MAX_K);
  std::vector<EnsPlanJobIn> in((size_t)n_jobs);
  int total_src = 0;
  int64_t longest = 0;
  for (int j = 0; j < n_jobs; ++j) {
    in[j].k = jobs[j].k;
    for (int c = 0; c < ENS_MAX_K && c < jobs[j].k; ++c) in[j].n[c] = jobs[j].n_samples[c];
  }
  const std::string why = ens_pool_check(in.data(), n_jobs, alg);
  REQUIRE(why.empty(), "%s: %s", fn, why.c_str());
  for (int j = 0; j < n_jobs; ++j) {
    const asx_ens_job &jb = jobs[j];
    int64_t n_job = 0;
    for (int c = 0; c < jb.k; ++c) {
      REQUIRE(jb.stem_dev[c] || jb.n_samples[c] == 0, "%s: job %d: contributor %d has a null stem with n = %lld", fn, j, c, (long long)jb.n_samples[c]);
      REQUIRE(jb.layout[c] == ASX_STEM_PLANAR || jb.layout[c] == ASX_STEM_ROWS, "%s: job %d: contributor %d has layout %d (0 planar [2, n], 1 rows [n, 2])",
              fn, j, c, (int)jb.layout[c]);
      REQUIRE(ens_slot_mode_known(mode_of(j, c)), "%s: job %d: contributor %d has mode %d (" ENS_SLOT_MODE_TEXT ")", fn, j, c, mode_of(j, c));
      n_job = std::max<int64_t>(n_job, jb.n_samples[c]);
    }
    REQUIRE(jb.out_dev, "%s: job %d: null output", fn, j);
    REQUIRE(jb.out_capacity >= n_job, "%s: job %d: output capacity %lld below its longest contributor (%lld)", fn, j, (long long)jb.out_capacity,
            (long long)n_job);
    total_src += jb.k;
    longest = std::max(longest, n_job);
  }
  if (n_jobs == 0) return ASX_OK;
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;

  // ---- peaks ------------------------------------------------------------------------------------------------------------
  const size_t src_bytes = (size_t)total_src * sizeof(EnsPoolSrc), peak_bytes = (size_t)total_src * 4, job_bytes = (size_t)n_jobs * sizeof(EnsPoolJob);
  if (c.staged) HIPCHK(hipEventSynchronize(c.staged));   // the last call's copies out of the staging area have run
  else HIPCHK(hipEventCreateWithFlags(&c.staged, hipEventDisableTiming));
  CHK(c.stage.ensure(src_bytes + peak_bytes + job_bytes));
  CHK(c.psrcs.ensure(src_bytes));
  CHK(c.ppeaks.ensure(peak_bytes));
  CHK(c.pjobs.ensure(job_bytes));
  EnsPoolSrc *h_src = reinterpret_cast<EnsPoolSrc *>(c.stage.p);
  EnsPoolJob *h_job = reinterpret_cast<EnsPoolJob *>(reinterpret_cast<char *>(c.stage.p) + src_bytes);   // (multiples of 8 bytes before it)
  unsigned int *h_peak = reinterpret_cast<unsigned int *>(reinterpret_cast<char *>(c.stage.p) + src_bytes + job_bytes);
  std::vector<int> first_src((size_t)n_jobs);
  for (int j = 0, q = 0; j < n_jobs; ++j) {
    first_src[j] = q;
    for (int k = 0; k < jobs[j].k; ++k, ++q) h_src[q] = EnsPoolSrc{jobs[j].stem_dev[k], jobs[j].n_samples[k], (int32_t)(jobs[j].layout[k] == ASX_STEM_ROWS), q, (int32_t)mode_of(j, k), 0};
  }
  unsigned int *d_peak = reinterpret_cast<unsigned int *>(c.ppeaks.p);
  HIPCHK(hipMemcpyAsync(c.psrcs.p, h_src, src_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(d_peak, 0, peak_bytes, s));
  if (longest > 0) {
    const unsigned nb = (unsigned)std::min<int64_t>((2 * longest + 255) / 256, 2048);
    CHK(timed(e, ASX_PROF_MISC, 0.0, 0.0, s, [&]() {
      hipLaunchKernelGGL(ens_pool_peak_kernel, dim3(nb, (unsigned)total_src), dim3(256), 0, s, reinterpret_cast<const EnsPoolSrc *>(c.psrcs.p), d_peak);
    }));
  }
  HIPCHK(hipMemcpyAsync(h_peak, d_peak, peak_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));

  // ---- live sets, plan, job table ---------------------------------------------------------------------------------------------
  for (int j = 0; j < n_jobs; ++j)
    for (int k = 0; k < jobs[j].k; ++k) {
      float maxv;
      memcpy(&maxv, &h_peak[first_src[j] + k], 4);
      in[j].peak_after[k] = jobs[j].peak_after[k] = ens_peak_after(maxv, mode_of(j, k), max_peak, min_peak, has_min);
    }
  EnsPoolPlan pp;
  ens_pool_build(in.data(), n_jobs, alg, silent_below, pp);
  REQUIRE(pp.wave_blocks < ((int64_t)1 << 31) && pp.frames < ((int64_t)1 << 31) && pp.fold_blocks < ((int64_t)1 << 31),
          "%s: the jobs of one call make %lld / %lld / %lld workgroups of a stage (2^31 - 1 at most)", fn, (long long)pp.wave_blocks,
          (long long)pp.frames, (long long)pp.fold_blocks);
  int k_spectral = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const EnsPlanJob &p = pp.job[j];
    EnsPoolJob &d = h_job[j];
    memset(&d, 0, sizeof(d));
    const bool weighted = weights && n_weights == p.live;   // Ensembler.ensemble: a weights list of another length means equal weights
    for (int k = 0; k < p.live; ++k) {
      d.src[k] = h_src[first_src[j] + p.who[k]];
      d.w[k] = weighted ? weights[k] : 1.0;
      d.wsum += d.w[k];
    }
    d.out = jobs[j].out_dev;
    d.n_max = p.n_max;
    d.n_out = p.n_out;
    d.wave_blk0 = p.wave_blk0;
    d.fold_blk0 = p.fold_blk0;
    d.frame0 = p.frame0;
    d.K = p.live;
    d.T = p.T;
    d.pick = p.pick ? 1 : 0;
    if (p.frames) k_spectral = std::max(k_spectral, p.live);
    jobs[j].live = p.live;
    jobs[j].n_out = p.n_out;
  }
  const int nf = c.plan.n_fft, nh = c.plan.nh, hop = ENS_PLAN_HOP;
  if (pp.frames) CHK(c.frames.ensure((size_t)pp.frames * 2 * nf * 4));
  if (pp.picks) {
    CHK(c.ppartial.ensure((size_t)n_jobs * 2 * ENS_MAX_K * ENS_ABS_BLOCKS * 8));
    CHK(c.psel.ensure((size_t)n_jobs * 2 * 4));
  }
  HIPCHK(hipMemcpyAsync(c.pjobs.p, h_job, job_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipEventRecord(c.staged, s));

  // ---- one launch per stage ---------------------------------------------------------------------------------------------------
  const EnsPoolJob *dj = reinterpret_cast<const EnsPoolJob *>(c.pjobs.p);
  const EnsSlotEdge ed{d_peak, max_peak, min_peak, has_min, 0};
  if (pp.picks)
    CHK(timed(e, ASX_PROF_MISC, 0.0, 0.0, s, [&]() {
      hipLaunchKernelGGL(ens_pool_abssum_kernel, dim3((unsigned)(ENS_ABS_BLOCKS * n_jobs), 2 * ENS_MAX_K), dim3(256), 0, s, dj, ed,
                         reinterpret_cast<double *>(c.ppartial.p));
      hipLaunchKernelGGL(ens_pool_pick_kernel, dim3((unsigned)n_jobs), dim3(64), 0, s, dj, reinterpret_cast<const double *>(c.ppartial.p),
                         reinterpret_cast<int *>(c.psel.p));
    }));
  if (pp.wave_blocks)
    CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * 256 * pp.wave_blocks, s, [&]() {
      hipLaunchKernelGGL(ens_pool_wave_kernel, dim3((unsigned)pp.wave_blocks), dim3(256), 0, s, dj, n_jobs, alg, ed, reinterpret_cast<const int *>(c.psel.p));
    }));
  if (pp.frames) {
    const size_t lds = ((size_t)nh * 2 + (size_t)(nh + 1) * (2 + (alg == ENS_MEDIAN_FFT ? k_spectral : 0))) * sizeof(float2);
    CHK(timed(e, ASX_PROF_STFT, 0.0, 4.0 * 2.0 * pp.frames * nf, s, [&]() {
      hipLaunchKernelGGL(ens_pool_fft_kernel, dim3((unsigned)pp.frames, 2), dim3(256), lds, s, dj, n_jobs, alg, hop, ed, c.frames.f(), c.window.f(),
                         reinterpret_cast<const float2 *>(c.tw.p), c.plan);
    }));
    if (pp.fold_blocks)
      CHK(timed(e, ASX_PROF_OLA, 0.0, 4.0 * 2.0 * pp.frames * nf, s, [&]() {
        hipLaunchKernelGGL(ens_pool_fold_kernel, dim3((unsigned)pp.fold_blocks), dim3(256), 0, s, dj, n_jobs, (const float *)c.frames.f(), (const float *)c.window.f(),
                           nf, hop);
      }));
  }
  return ASX_OK;
}
