// Engine side of the rational polyphase converter (included by asx.hip only): the per-engine coefficient tables and the launch of
// resample_rational_kernel (kernels_resample.h) for a plan of resample_plan.h.
#pragma once

// the engine's table for a pair the plan accepts: designed in float64 and uploaded at the first call for the pair
static int rs_table(asx_engine *e, const ResamplePlan &p, const RsTable **out) {
  std::lock_guard<std::mutex> lock(e->rs_mu);
  for (const RsTable *t : e->rs_tabs)
    if (t->plan.sr_in == p.sr_in && t->plan.sr_out == p.sr_out) {
      *out = t;
      return ASX_OK;
    }
  std::vector<double> h;
  std::vector<float> tab;
  resample_plan_taps(p, h);
  resample_plan_table(p, h, tab);
  RsTable *t = new RsTable();
  t->plan = p;
  const int rc = ht_up(t->tab, tab);
  if (rc != ASX_OK) {
    t->tab.release();
    delete t;
    return rc;
  }
  e->rs_tabs.push_back(t);
  *out = t;
  return ASX_OK;
}

template <int K, bool TAPS_LDS>
static void rs_launch(const ResamplePlan &p, const float *x, int channels, int64_t n_in, const float *tab, float *y, int64_t n_out, hipStream_t s) {
  const size_t lds = (size_t)(p.span + (TAPS_LDS ? p.L * p.T : 0)) * sizeof(float);   // at most 64 KiB (RESAMPLE_MAX_LDS_FLOATS)
  const unsigned tiles = (unsigned)((n_out + p.J * K - 1) / (p.J * K));
  hipLaunchKernelGGL((resample_rational_kernel<K, TAPS_LDS>), dim3(tiles, (unsigned)channels), dim3(RS_THREADS), lds, s, x, n_in, tab, (int)p.L, (int)p.M,
                     (int)p.P, (int)p.J, (int)p.span, y, n_out);
}

// the writer-side form: the tiles cover the caller's n_out, x planar or rows (kernels_resample.h resample_rational_stem_kernel)
template <int K, bool TAPS_LDS>
static void rs_stem_launch(const ResamplePlan &p, const float *x, bool rows, int channels, int64_t n_in, const float *tab, float *y, int64_t n_out,
                           hipStream_t s) {
  const size_t lds = (size_t)(p.span + (TAPS_LDS ? p.L * p.T : 0)) * sizeof(float);   // at most 64 KiB (RESAMPLE_MAX_LDS_FLOATS)
  const dim3 grid((unsigned)((n_out + p.J * K - 1) / (p.J * K)), (unsigned)channels);
  if (rows)
    hipLaunchKernelGGL((resample_rational_stem_kernel<K, TAPS_LDS, true>), grid, dim3(RS_THREADS), lds, s, x, channels, n_in, tab, (int)p.L, (int)p.M,
                       (int)p.P, (int)p.J, (int)p.span, y, n_out);
  else
    hipLaunchKernelGGL((resample_rational_stem_kernel<K, TAPS_LDS, false>), grid, dim3(RS_THREADS), lds, s, x, channels, n_in, tab, (int)p.L, (int)p.M,
                       (int)p.P, (int)p.J, (int)p.span, y, n_out);
}

// the complement form of the same launch: y (may be null) and c = fl(fl(mix_scale mix) - fl(stem_scale y)) from one pass over the tiles
template <int K, bool TAPS_LDS>
static void rs_complement_launch(const ResamplePlan &p, const float *x, bool rows, int channels, int64_t n_in, const float *tab, float *y, int64_t n_out,
                                 const float *mix, int64_t mix_stride, float mix_scale, float stem_scale, float *c, hipStream_t s) {
  const size_t lds = (size_t)(p.span + (TAPS_LDS ? p.L * p.T : 0)) * sizeof(float);   // at most 64 KiB (RESAMPLE_MAX_LDS_FLOATS)
  const dim3 grid((unsigned)((n_out + p.J * K - 1) / (p.J * K)), (unsigned)channels);
  if (rows)
    hipLaunchKernelGGL((resample_rational_stem_kernel<K, TAPS_LDS, true, true>), grid, dim3(RS_THREADS), lds, s, x, channels, n_in, tab, (int)p.L,
                       (int)p.M, (int)p.P, (int)p.J, (int)p.span, y, n_out, mix, mix_stride, mix_scale, stem_scale, c);
  else
    hipLaunchKernelGGL((resample_rational_stem_kernel<K, TAPS_LDS, false, true>), grid, dim3(RS_THREADS), lds, s, x, channels, n_in, tab, (int)p.L,
                       (int)p.M, (int)p.P, (int)p.J, (int)p.span, y, n_out, mix, mix_stride, mix_scale, stem_scale, c);
}
