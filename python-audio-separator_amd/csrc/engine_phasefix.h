// asx_phase_fix_batch_dev / asx_phase_fix_dev / asx_phase_fix (kernels_phasefix.h): one model's STFT magnitudes on phases blended
// towards another's, on stems in HBM.  Included by asx.hip behind engine_ens.h (EnsCtx: plan, window, twiddles, frame workspace; PinBuf).
#pragma once
#include <algorithm>

static std::atomic<long long> g_phasefix_launches{0};   // launches of the phase_fix kernels since the process started (asx_counter "phasefix_launches")

struct PhaseCtx {
  DevBuf tab;                   // [bin weights (ASX_PHASE_BINS floats, padded to 16 bytes)][job table of a pooled call]
  PinBuf stage;                 // its pinned host image: what an asynchronous copy reads must stay put until the copy has run
  hipEvent_t staged = nullptr;  // behind the last call's launches: until then `stage` is being copied and `tab` read
};

static void phase_destroy(PhaseCtx *c) {
  c->tab.release();
  if (c->staged) {
    (void)hipEventSynchronize(c->staged);
    (void)hipEventDestroy(c->staged);
  }
  c->stage.release();
  delete c;
}

static bool phase_hop_known(int hop) { return hop == 256 || hop == 512 || hop == 1024; }

// `fn` names the entry point in the messages; `single`: asx_phase_fix_dev's form (the job travels by value, the same device functions run)
static int phase_fix_batch_dev(asx_engine *e, const char *fn, const asx_phase_job *jobs, int n_jobs, const float *bin_weights, int hop, bool single,
                               hipStream_t s) {
  // every argument of every job is judged before anything is enqueued, the engine last (so that the refusals can be told apart without a device)
  REQUIRE(n_jobs >= 0 && n_jobs <= ASX_ENS_MAX_JOBS && (jobs || n_jobs == 0), "%s: bad argument (jobs %p, n_jobs %d; 0 .. %d jobs)", fn,
          (const void *)jobs, n_jobs, ASX_ENS_MAX_JOBS);
  REQUIRE(bin_weights, "%s: null bin weights", fn);
  for (int b = 0; b < ASX_PHASE_BINS; ++b) REQUIRE(std::isfinite(bin_weights[b]), "%s: the weight of bin %d is not finite", fn, b);
  REQUIRE(phase_hop_known(hop), "%s: hop %d (256, 512 or 1024)", fn, hop);
  struct Span {
    uintptr_t lo, hi;
    int job, out;
  };
  std::vector<Span> spans;
  std::vector<PhaseJob> tab((size_t)n_jobs);
  int64_t frames = 0, fold_blocks = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const asx_phase_job &jb = jobs[j];
    REQUIRE(jb.n_samples >= 1 && jb.n_samples <= ((int64_t)1 << 38), "%s: job %d: n_samples %lld (1 .. 2^38)", fn, j, (long long)jb.n_samples);
    REQUIRE(jb.source_n_samples >= 0 && jb.source_n_samples <= ((int64_t)1 << 38), "%s: job %d: source_n_samples %lld (0 .. 2^38)", fn, j,
            (long long)jb.source_n_samples);
    REQUIRE(jb.target_dev && (((uintptr_t)jb.target_dev) & 3) == 0, "%s: job %d: the target is null or not 4-byte aligned", fn, j);
    REQUIRE(jb.source_dev || jb.source_n_samples == 0, "%s: job %d: the source is null with n = %lld", fn, j, (long long)jb.source_n_samples);
    REQUIRE((((uintptr_t)jb.source_dev) & 3) == 0, "%s: job %d: the source is not 4-byte aligned", fn, j);
    REQUIRE(jb.out_dev && (((uintptr_t)jb.out_dev) & 3) == 0, "%s: job %d: the output is null or not 4-byte aligned", fn, j);
    const int32_t layouts[3] = {jb.target_layout, jb.source_layout, jb.out_layout};
    const char *names[3] = {"target", "source", "output"};
    for (int k = 0; k < 3; ++k)
      REQUIRE(layouts[k] == ASX_STEM_PLANAR || layouts[k] == ASX_STEM_ROWS, "%s: job %d: %s layout %d (0 planar [2, n], 1 rows [n, 2])", fn, j, names[k],
              (int)layouts[k]);
    const int T = (int)(1 + jb.n_samples / hop);
    tab[j] = PhaseJob{jb.target_dev, jb.source_dev, jb.out_dev, jb.n_samples, jb.source_n_samples, frames, fold_blocks, T,
                      (int32_t)(jb.target_layout == ASX_STEM_ROWS), (int32_t)(jb.source_layout == ASX_STEM_ROWS), (int32_t)(jb.out_layout == ASX_STEM_ROWS)};
    frames += T;
    fold_blocks += (jb.n_samples + 255) / 256;
    REQUIRE(frames < ((int64_t)1 << 31) && fold_blocks < ((int64_t)1 << 31), "%s: the jobs of one call make %lld / %lld workgroups of a stage (2^31 - 1 at most)",
            fn, (long long)frames, (long long)fold_blocks);
    spans.push_back(Span{(uintptr_t)jb.target_dev, (uintptr_t)jb.target_dev + (uintptr_t)jb.n_samples * 8, j, 0});
    if (jb.source_n_samples > 0) spans.push_back(Span{(uintptr_t)jb.source_dev, (uintptr_t)jb.source_dev + (uintptr_t)jb.source_n_samples * 8, j, 0});
    spans.push_back(Span{(uintptr_t)jb.out_dev, (uintptr_t)jb.out_dev + (uintptr_t)jb.n_samples * 8, j, 1});
  }
  // an output may share no byte with an input or another output of the call (inputs may overlap: the source may be the target).  In
  // ascending order of their first bytes, a span overlaps an earlier one exactly when it starts below the furthest end seen so far.
  std::sort(spans.begin(), spans.end(), [](const Span &a, const Span &b) { return a.lo != b.lo ? a.lo < b.lo : a.out > b.out; });
  uintptr_t end_any = 0, end_out = 0;
  int job_any = -1, job_out = -1;
  for (const Span &sp : spans) {
    if (sp.out) REQUIRE(sp.lo >= end_any, "%s: job %d: the output overlaps an array of job %d", fn, sp.job, job_any);
    else REQUIRE(sp.lo >= end_out, "%s: job %d: an input overlaps the output of job %d", fn, sp.job, job_out);
    if (sp.hi > end_any) end_any = sp.hi, job_any = sp.job;
    if (sp.out && sp.hi > end_out) end_out = sp.hi, job_out = sp.job;
  }
  REQUIRE(e, "%s: null engine", fn);
  if (n_jobs == 0) return ASX_OK;
  HIPCHK(hipSetDevice(e->device));
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  if (!e->phase) {
    e->phase = new PhaseCtx();
    // two buffers and two spectra: 32,784 B, inside the limit every device starts with (the invert kernels' footprint and their path)
    const int lds = (int)(((size_t)c.plan.nh * 2 + (size_t)(c.plan.nh + 1) * 2) * sizeof(float2));
    grant_lds(&phase_fix_kernel, lds);
    grant_lds(&phase_fix_pool_kernel, lds);
  }
  PhaseCtx &pc = *e->phase;
  const int nf = c.plan.n_fft, nh = c.plan.nh;
  const size_t w_bytes = ((size_t)ASX_PHASE_BINS * 4 + 15) & ~(size_t)15, tab_bytes = single ? 0 : tab.size() * sizeof(PhaseJob);
  // the last call's copy and launches have run (on whichever stream): both tables are free.  This call itself waits for nothing of its own
  if (pc.staged) HIPCHK(hipEventSynchronize(pc.staged));
  else HIPCHK(hipEventCreateWithFlags(&pc.staged, hipEventDisableTiming));
  CHK(pc.stage.ensure(w_bytes + tab_bytes));
  CHK(pc.tab.ensure(w_bytes + tab_bytes));
  CHK(c.frames.ensure((size_t)frames * 2 * nf * 4));
  memset(pc.stage.p, 0, w_bytes);
  memcpy(pc.stage.p, bin_weights, (size_t)ASX_PHASE_BINS * 4);
  if (tab_bytes) memcpy(reinterpret_cast<char *>(pc.stage.p) + w_bytes, tab.data(), tab_bytes);
  HIPCHK(hipMemcpyAsync(pc.tab.p, pc.stage.p, w_bytes + tab_bytes, hipMemcpyHostToDevice, s));
  const float *dw = pc.tab.f();
  const PhaseJob *dj = reinterpret_cast<const PhaseJob *>(reinterpret_cast<const char *>(pc.tab.p) + w_bytes);
  const size_t lds = ((size_t)nh * 2 + (size_t)(nh + 1) * 2) * sizeof(float2);
  const float2 *tw = reinterpret_cast<const float2 *>(c.tw.p);
  double in_bytes = 0.0;
  for (const PhaseJob &jb : tab) in_bytes += 8.0 * (double)(jb.n + std::min(jb.n, jb.n_src));
  CHK(timed(e, ASX_PROF_STFT, 0.0, in_bytes * (double)nf / hop + 4.0 * 2.0 * frames * nf, s, [&]() {
    if (single)
      hipLaunchKernelGGL(phase_fix_kernel, dim3((unsigned)frames, 2), dim3(256), lds, s, tab[0], hop, dw, c.frames.f(), (const float *)c.window.f(), tw, c.plan);
    else
      hipLaunchKernelGGL(phase_fix_pool_kernel, dim3((unsigned)frames, 2), dim3(256), lds, s, dj, n_jobs, hop, dw, c.frames.f(), (const float *)c.window.f(), tw,
                         c.plan);
  }));
  CHK(timed(e, ASX_PROF_OLA, 0.0, 4.0 * 2.0 * frames * nf + in_bytes, s, [&]() {
    if (single)
      hipLaunchKernelGGL(phase_fix_fold_kernel, dim3((unsigned)fold_blocks), dim3(256), 0, s, tab[0], (const float *)c.frames.f(), (const float *)c.window.f(), nf,
                         hop);
    else
      hipLaunchKernelGGL(phase_fix_pool_fold_kernel, dim3((unsigned)fold_blocks), dim3(256), 0, s, dj, n_jobs, (const float *)c.frames.f(),
                         (const float *)c.window.f(), nf, hop);
  }));
  g_phasefix_launches.fetch_add(2);
  HIPCHK(hipEventRecord(pc.staged, s));
  return ASX_OK;
}
