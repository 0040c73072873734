// asx_mixdown_batch_dev / asx_mixdown (kernels_mix.h): weighted sums of stems in HBM, every job of a call in one launch.  Included by asx.hip
// behind engine_ens.h (PinBuf).
#pragma once

struct MixCtx {
  DevBuf tab;                   // the job table the launch reads
  PinBuf stage;                 // its pinned host image: what an asynchronous copy reads must stay put until the copy has run
  hipEvent_t staged = nullptr;  // behind the last call's launch: until then `stage` is being copied and `tab` read
};

static void mix_destroy(MixCtx *c) {
  c->tab.release();
  if (c->staged) {
    (void)hipEventSynchronize(c->staged);
    (void)hipEventDestroy(c->staged);
  }
  c->stage.release();
  delete c;
}

static int mix_batch_dev(asx_engine *e, const asx_mix_job *jobs, int n_jobs, hipStream_t s) {
  // every argument of every job is judged before anything is enqueued, the engine last (so that the refusals can be told apart without a device)
  REQUIRE(n_jobs >= 0 && (jobs || n_jobs == 0), "asx_mixdown_batch_dev: bad argument (jobs %p, n_jobs %d)", (const void *)jobs, n_jobs);
  int64_t blocks = 0;
  double bytes = 0.0;
  for (int j = 0; j < n_jobs; ++j) {
    const asx_mix_job &jb = jobs[j];
    REQUIRE(jb.k >= 1 && jb.k <= ASX_MIX_MAX_K, "asx_mixdown_batch_dev: job %d: %d sources (1 .. %d)", j, (int)jb.k, ASX_MIX_MAX_K);
    REQUIRE(jb.n_out >= 1 && jb.n_out <= ((int64_t)1 << 40), "asx_mixdown_batch_dev: job %d: n_out = %lld (1 .. 2^40)", j, (long long)jb.n_out);
    REQUIRE(jb.out && (((uintptr_t)jb.out) & 3) == 0, "asx_mixdown_batch_dev: job %d: the output is null or not 4-byte aligned", j);
    REQUIRE(jb.out_layout == ASX_STEM_PLANAR || jb.out_layout == ASX_STEM_ROWS, "asx_mixdown_batch_dev: job %d: output layout %d (0 planar [2, n], 1 rows [n, 2])",
            j, (int)jb.out_layout);
    for (int k = 0; k < jb.k; ++k) {
      const asx_mix_src &sr = jb.src[k];
      REQUIRE(sr.n >= 0 && sr.n <= ((int64_t)1 << 40), "asx_mixdown_batch_dev: job %d: source %d has n = %lld (0 .. 2^40)", j, k, (long long)sr.n);
      REQUIRE(sr.x || sr.n == 0, "asx_mixdown_batch_dev: job %d: source %d is null with n = %lld", j, k, (long long)sr.n);
      REQUIRE((((uintptr_t)sr.x) & 3) == 0, "asx_mixdown_batch_dev: job %d: source %d is not 4-byte aligned", j, k);
      REQUIRE(sr.layout == ASX_STEM_PLANAR || sr.layout == ASX_STEM_ROWS, "asx_mixdown_batch_dev: job %d: source %d has layout %d (0 planar [2, n], 1 rows [n, 2])",
              j, k, (int)sr.layout);
      REQUIRE(std::isfinite(sr.w), "asx_mixdown_batch_dev: job %d: the weight of source %d is not finite", j, k);
      bytes += 8.0 * (double)std::min<int64_t>(sr.n, jb.n_out);
    }
    blocks += (mix_groups(jb.n_out, mix_shift(jb.out, jb.out_layout == ASX_STEM_ROWS)) + 255) / 256;
    bytes += 8.0 * (double)jb.n_out;
  }
  REQUIRE(blocks < ((int64_t)1 << 31), "asx_mixdown_batch_dev: the jobs of one call make %lld workgroups (2^31 - 1 at most)", (long long)blocks);
  REQUIRE(e, "asx_mixdown_batch_dev: null engine");
  if (n_jobs == 0) return ASX_OK;
  HIPCHK(hipSetDevice(e->device));
  if (!e->mix) e->mix = new MixCtx();
  MixCtx &c = *e->mix;
  const size_t tab_bytes = (size_t)n_jobs * sizeof(MixDevJob);
  // the last call's copy and launch have run (on whichever stream): both tables are free.  This call itself waits for nothing of its own
  if (c.staged) HIPCHK(hipEventSynchronize(c.staged));
  else HIPCHK(hipEventCreateWithFlags(&c.staged, hipEventDisableTiming));
  CHK(c.stage.ensure(tab_bytes));
  CHK(c.tab.ensure(tab_bytes));
  MixDevJob *h = reinterpret_cast<MixDevJob *>(c.stage.p);
  int32_t blk = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const asx_mix_job &jb = jobs[j];
    MixDevJob &d = h[j];
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < jb.k; ++k) {
      d.x[k] = jb.src[k].x;
      d.n[k] = jb.src[k].n;
      d.w[k] = jb.src[k].w;
      d.rows[k] = jb.src[k].layout == ASX_STEM_ROWS;
    }
    d.out = jb.out;
    d.n_out = jb.n_out;
    d.k = jb.k;
    d.out_rows = jb.out_layout == ASX_STEM_ROWS;
    d.shift = mix_shift(jb.out, d.out_rows);
    d.blk0 = blk;
    blk += (int32_t)((mix_groups(jb.n_out, d.shift) + 255) / 256);
  }
  HIPCHK(hipMemcpyAsync(c.tab.p, h, tab_bytes, hipMemcpyHostToDevice, s));
  CHK(timed(e, ASX_PROF_MISC, 0.0, bytes, s, [&]() {
    hipLaunchKernelGGL(mixdown_kernel, dim3((unsigned)blk), dim3(256), 0, s, reinterpret_cast<const MixDevJob *>(c.tab.p), n_jobs);
  }));
  HIPCHK(hipEventRecord(c.staged, s));
  return ASX_OK;
}
