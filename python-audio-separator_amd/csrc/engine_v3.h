// TFC-TDF v3 (MDX23C) on the engine: uvr_lib_v5/tfc_tdf_v3.py:110-267 and the TFC branch of
// MDXCSeparator.demix (architectures/mdxc_separator.py:345-404).  Included by asx.hip (one TU).
//
// Pre-activation blocks: every conv / linear is preceded by norm -> act.  InstanceNorm needs
// the statistics of the whole (T, F) plane, so norm -> act is its own memory-bound pass
// (instnorm_stats_kernel + norm_act_kernel) that writes the activated tensor the MFMA kernels
// then DMA; shortcut adds, the TDF residual, the decoder concat (written in place through
// channel-slice views) and the final `x * first_conv_out` are fused or zero-copy.
// GroupNorm runs a split statistics pass (v3_gn_partial_kernel + v3_gn_finish_kernel) into the same
// per-(b, c) (mean, rstd) table; BatchNorm (eval) is folded into a per-channel scale / shift at load
// time and needs no statistics.  All norms share norm_act_kernel.
#pragma once
#include "v3_norm.h"

struct V3Norm {
  DevBuf g, b;  // affine weight / bias; BatchNorm: the folded scale / shift
  int c = 0;
};

struct V3Block {
  int in_c = 0, c = 0, f = 0;
  V3Norm n_tfc1, n_tdf0, n_tdf1, n_tfc2;
  ConvLayer tfc1, tfc2, shortcut;
  TdfLayer tdf0, tdf1;
};

struct V3Net {
  asx_v3_config cfg{};
  float act_alpha = 1.f;  // cfg.act == V3_ACT_ELU
  bool begun = false, ready = false;
  ConvLayer first, final0, final1;
  std::vector<std::vector<V3Block>> enc, dec;
  std::vector<V3Block> mid;
  std::vector<ConvLayer> ds, us;
  std::vector<V3Norm> ds_n, us_n;
  // workspace (sized for ws_batch chunks)
  int ws_batch = 0;
  DevBuf cat0, firstout, S, A, X1, X2, XB, CUR, H, HA, stats, gn_part, out_spec, frames, chunk_out, d_starts;
  std::vector<DevBuf> lvl;
};

static void v3_free_norm(V3Norm &n) {
  n.g.release();
  n.b.release();
}
static void v3_free_block(V3Block &b) {
  v3_free_norm(b.n_tfc1);
  v3_free_norm(b.n_tdf0);
  v3_free_norm(b.n_tdf1);
  v3_free_norm(b.n_tfc2);
  free_conv(b.tfc1);
  free_conv(b.tfc2);
  free_conv(b.shortcut);
  free_tdf(b.tdf0);
  free_tdf(b.tdf1);
}
static void v3_free(V3Net &n) {
  free_conv(n.first);
  free_conv(n.final0);
  free_conv(n.final1);
  for (auto &sc : n.enc)
    for (auto &b : sc) v3_free_block(b);
  for (auto &sc : n.dec)
    for (auto &b : sc) v3_free_block(b);
  for (auto &b : n.mid) v3_free_block(b);
  for (auto &c : n.ds) free_conv(c);
  for (auto &c : n.us) free_conv(c);
  for (auto &x : n.ds_n) v3_free_norm(x);
  for (auto &x : n.us_n) v3_free_norm(x);
  DevBuf *bufs[] = {&n.cat0, &n.firstout, &n.S, &n.A, &n.X1, &n.X2, &n.XB, &n.CUR, &n.H, &n.HA, &n.stats, &n.gn_part,
                    &n.out_spec, &n.frames, &n.chunk_out, &n.d_starts};
  for (auto *b : bufs) b->release();
  for (auto &l : n.lvl) l.release();
  n.ready = false;
}

static void v3_destroy(V3Net *n) {
  v3_free(*n);
  delete n;
}

// ---------------------------------------------------------------------------
// weights (reference state_dict names, tfc_tdf_v3.py)
// ---------------------------------------------------------------------------
static int v3_load_norm(asx_engine *e, V3Norm &n, const std::string &prefix, int c) {
  n.c = c;
  const int norm = e->v3->cfg.norm;
  if (norm == V3_NORM_NONE) return ASX_OK;
  const int G = v3_norm_groups(norm);
  // nn.GroupNorm refuses these at construction (tfc_tdf_v3.py:55-69)
  REQUIRE(G == 0 || c % G == 0, "%s: GroupNorm%d needs the channel count to be divisible by the number of groups, got %d channels",
          prefix.c_str(), G, c);
  const float *g, *b;
  CHK(get_tensor(e, prefix + ".weight", c, &g));
  CHK(get_tensor(e, prefix + ".bias", c, &b));
  std::vector<float> sc, sh;
  if (norm == V3_NORM_BATCH) {  // eval(): running statistics, folded (num_batches_tracked is not used)
    const float *rm, *rv;
    CHK(get_tensor(e, prefix + ".running_mean", c, &rm));
    CHK(get_tensor(e, prefix + ".running_var", c, &rv));
    sc.resize(c);
    sh.resize(c);
    v3_bn_fold(c, g, b, rm, rv, 1e-5, sc.data(), sh.data());
    g = sc.data();
    b = sh.data();
  }
  CHK(n.g.ensure((size_t)c * 4));
  CHK(n.b.ensure((size_t)c * 4));
  HIPCHK(hipMemcpy(n.g.p, g, (size_t)c * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(n.b.p, b, (size_t)c * 4, hipMemcpyHostToDevice));
  return ASX_OK;
}

static int v3_load_conv(asx_engine *e, ConvLayer &L, int kind, const std::string &name, int cin, int cout, int ntap) {
  const float *w;
  CHK(get_tensor(e, name, (int64_t)cin * cout * ntap, &w));
  CHK(conv_setup(L, kind, cin, cout, 0));
  CHK(conv_pack(L, w, nullptr, e->winograd));
  return ASX_OK;
}

static int v3_load_tfc_tdf(asx_engine *e, std::vector<V3Block> &blocks, const std::string &prefix, int in_c, int c,
                           int f) {
  const asx_v3_config &cf = e->v3->cfg;
  blocks.assign(cf.num_blocks_per_scale, V3Block());
  const int fb = f / cf.bottleneck_factor;
  for (int j = 0; j < cf.num_blocks_per_scale; ++j) {
    V3Block &b = blocks[j];
    const std::string p = prefix + ".blocks." + std::to_string(j);
    b.in_c = in_c;
    b.c = c;
    b.f = f;
    CHK(v3_load_norm(e, b.n_tfc1, p + ".tfc1.0", in_c));
    CHK(v3_load_conv(e, b.tfc1, CK_3X3, p + ".tfc1.2.weight", in_c, c, 9));
    CHK(v3_load_norm(e, b.n_tdf0, p + ".tdf.0", c));
    const float *w;
    CHK(get_tensor(e, p + ".tdf.2.weight", (int64_t)fb * f, &w));
    CHK(tdf_pack(b.tdf0, fb, f, c, w, nullptr, nullptr, nullptr));
    CHK(v3_load_norm(e, b.n_tdf1, p + ".tdf.3", c));
    CHK(get_tensor(e, p + ".tdf.5.weight", (int64_t)f * fb, &w));
    CHK(tdf_pack(b.tdf1, f, fb, c, w, nullptr, nullptr, nullptr));
    CHK(v3_load_norm(e, b.n_tfc2, p + ".tfc2.0", c));
    CHK(v3_load_conv(e, b.tfc2, CK_3X3, p + ".tfc2.2.weight", c, c, 9));
    CHK(v3_load_conv(e, b.shortcut, CK_1X1, p + ".shortcut.weight", in_c, c, 1));
    in_c = c;
  }
  return ASX_OK;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
struct V3View {
  float *p;
  int64_t bstride;  // floats between batch items
};

// norm -> act of one pre-activation block on a channel-slice view.  The core takes the configuration (norm / act as asx_v3_config
// encodes them, alpha), the affine and the two workspaces (stats: 2 B C floats; gn_part: v3_gn_splits slices of every (group, item))
// as arguments; v3_norm_act reads them from the loaded net.
static int v3_norm_act_core(asx_engine *e, int norm, int cfg_act, float alpha, const float *gam, const float *bet, const DevBuf &stats,
                            const DevBuf &gn_part, V3View x, int C, int64_t P, int B, float *y, hipStream_t s) {
  float2 *st = reinterpret_cast<float2 *>(stats.p);
  // cfg.act: 0 relu, 1 gelu, 2 elu -> kernel enum (ACT_*) 1 relu, 2 gelu, 3 elu
  const int act = cfg_act == V3_ACT_GELU ? ACT_GELU : cfg_act == V3_ACT_ELU ? ACT_ELU : ACT_RELU;
  const double bytes_r = 4.0 * B * C * (double)P;
  if (norm == V3_NORM_INSTANCE) {
    CHK(timed(e, ASX_PROF_MISC, 0.0, bytes_r, s, [&]() {
      hipLaunchKernelGGL(instnorm_stats_kernel, dim3(C, B), dim3(256), 0, s, x.p, x.bstride, C, P, 1e-5f, st);
    }));
  } else if (norm > V3_NORM_GROUP) {
    const int G = v3_norm_groups(norm);
    const int64_t len = (int64_t)(C / G) * P;
    const int ns = v3_gn_splits(B, G, len);
    REQUIRE(C % G == 0 && gn_part.bytes >= (size_t)B * G * ns * sizeof(double2), "GroupNorm%d over %d channels: workspace", G, C);
    double2 *part = reinterpret_cast<double2 *>(gn_part.p);
    CHK(timed(e, ASX_PROF_MISC, 0.0, bytes_r, s, [&]() {
      hipLaunchKernelGGL(v3_gn_partial_kernel, dim3((unsigned)ns, (unsigned)G, (unsigned)B), dim3(256), 0, s, x.p, x.bstride, C, G, P,
                         ns, part);
      hipLaunchKernelGGL(v3_gn_finish_kernel, dim3((unsigned)G, (unsigned)B), dim3(256), 0, s, part, C, G, P, ns, 1e-5f, st);
    }));
  }
  const bool has_stats = norm == V3_NORM_INSTANCE || norm > V3_NORM_GROUP;
  const unsigned gx = (unsigned)std::min<int64_t>((P / 4 + 255) / 256 + 1, 64);
  const float *gp = norm == V3_NORM_NONE ? nullptr : gam, *bp = norm == V3_NORM_NONE ? nullptr : bet;
  CHK(timed(e, ASX_PROF_MISC, 0.0, 2.0 * bytes_r, s, [&]() {
    hipLaunchKernelGGL(norm_act_kernel, dim3(gx, C, B), dim3(256), 0, s, x.p, x.bstride, C, P,
                       has_stats ? st : nullptr, gp, bp, act, alpha, y);
  }));
  return ASX_OK;
}

static int v3_norm_act(asx_engine *e, const V3Norm &n, V3View x, int C, int64_t P, int B, float *y, hipStream_t s) {
  V3Net &net = *e->v3;
  return v3_norm_act_core(e, net.cfg.norm, net.cfg.act, net.act_alpha, n.g.f(), n.b.f(), net.stats, net.gn_part, x, C, P, B, y, s);
}

// One TFC_TDF (tfc_tdf_v3.py:110-148).  x_in: view with blocks[0].in_c channels; dest: view with c channels.
static int v3_tfc_tdf(asx_engine *e, const std::vector<V3Block> &blocks, V3View x_in, V3View dest, int B, int T, int F,
                      hipStream_t s) {
  V3Net &n = *e->v3;
  const int64_t P = (int64_t)T * F;
  V3View x = x_in;
  for (size_t j = 0; j < blocks.size(); ++j) {
    const V3Block &b = blocks[j];
    const bool last = j + 1 == blocks.size();
    ConvView vs;
    vs.x_bstride = x.bstride;
    CHK(conv_launch(e, b.shortcut, x.p, nullptr, n.S.f(), B, T, F, s, vs));                    // s = shortcut(x)
    CHK(v3_norm_act(e, b.n_tfc1, x, b.in_c, P, B, n.A.f(), s));
    CHK(conv_launch(e, b.tfc1, n.A.f(), nullptr, n.X1.f(), B, T, F, s));                        // x = tfc1(x)
    CHK(v3_norm_act(e, b.n_tdf0, V3View{n.X1.f(), (int64_t)b.c * P}, b.c, P, B, n.A.f(), s));
    const int64_t M = (int64_t)B * b.c * T;
    CHK(tdf_launch(e, b.tdf0, n.A.f(), nullptr, n.H.f(), M, T, s, 0));
    const int fb = b.tdf0.n;
    CHK(v3_norm_act(e, b.n_tdf1, V3View{n.H.f(), (int64_t)b.c * T * fb}, b.c, (int64_t)T * fb, B, n.HA.f(), s));
    CHK(tdf_launch(e, b.tdf1, n.HA.f(), n.X1.f(), n.X2.f(), M, T, s, 0));                       // x = x + tdf(x)
    CHK(v3_norm_act(e, b.n_tfc2, V3View{n.X2.f(), (int64_t)b.c * P}, b.c, P, B, n.A.f(), s));
    ConvView vo;
    vo.res = n.S.f();                                                                          // x = tfc2(x) + s
    V3View out = last ? dest : V3View{n.XB.f(), (int64_t)b.c * P};
    vo.y_bstride = out.bstride;
    CHK(conv_launch(e, b.tfc2, n.A.f(), nullptr, out.p, B, T, F, s, vo));
    x = out;
  }
  return ASX_OK;
}

// conv3h_kernel's walk tables (conv3h_walk_ensure) for a forward of B chunks: v3_core_dev's walk over the levels
static int v3_walks_ensure(asx_engine *e, int B) {
  V3Net &n = *e->v3;
  const asx_v3_config &cf = n.cfg;
  auto walks = [&](const std::vector<V3Block> &bs, int t, int f) -> int {
    for (const V3Block &b : bs) {
      CHK(conv3h_walk_ensure(e, b.tfc1, B, t, f));
      CHK(conv3h_walk_ensure(e, b.tfc2, B, t, f));
    }
    return ASX_OK;
  };
  int t = e->cfg.segment_size, f = e->cfg.dim_f / cf.num_subbands;
  for (int i = 0; i < cf.num_scales; ++i, t /= 2, f /= 2) {
    CHK(walks(n.enc[i], t, f));
    CHK(walks(n.dec[cf.num_scales - 1 - i], t, f));
  }
  return walks(n.mid, t, f);
}

static int v3_ensure_workspace(asx_engine *e, int B) {
  V3Net &n = *e->v3;
  CHK(v3_walks_ensure(e, B));                          // (per batch size, not per largest batch: a table is planned for its B)
  if (B <= n.ws_batch) return ASX_OK;
  const asx_v3_config &cf = n.cfg;
  const int T = e->cfg.segment_size, k = cf.num_subbands, Fs = e->cfg.dim_f / k;
  const int dim_c = k * cf.num_channels * 2;
  const int64_t P0 = (int64_t)T * Fs;
  const int c0 = cf.num_channels_model;
  const size_t big = (size_t)B * 2 * c0 * P0 * 4;  // the level-0 decoder sees 2*c0 channels
  CHK(n.cat0.ensure((size_t)B * (dim_c + c0) * P0 * 4));
  CHK(n.firstout.ensure((size_t)B * c0 * P0 * 4));
  CHK(n.A.ensure(big));
  CHK(n.S.ensure(big / 2));
  CHK(n.X1.ensure(big / 2));
  CHK(n.X2.ensure(big / 2));
  CHK(n.XB.ensure(big / 2));
  CHK(n.CUR.ensure(big / 2));
  CHK(n.H.ensure(big / 2 / cf.bottleneck_factor + 256));
  CHK(n.HA.ensure(big / 2 / cf.bottleneck_factor + 256));
  int cmax = c0 + cf.growth * cf.num_scales;
  CHK(n.stats.ensure((size_t)B * 2 * cmax * sizeof(float2)));
  if (cf.norm > V3_NORM_GROUP) CHK(n.gn_part.ensure((size_t)B * v3_norm_groups(cf.norm) * V3_GN_MAX_SPLIT * sizeof(double2)));
  n.lvl.resize(cf.num_scales);
  int c = c0;
  int64_t P = P0;
  for (int i = 0; i < cf.num_scales; ++i) {
    CHK(n.lvl[i].ensure((size_t)B * 2 * c * P * 4));
    c += cf.growth;
    P /= 4;
  }
  // conv3h_kernel's partial sums, where a tfc1 of 96 -> 96 / 144 -> 144 channels runs it (v3_core_dev's walk over the levels)
  {
    size_t ps = 0;
    auto ps_blocks = [&](const std::vector<V3Block> &bs, int t, int f) {
      for (const V3Block &b : bs) ps = std::max(ps, std::max(conv3h_ps_need(b.tfc1, B, t, f), conv3h_ps_need(b.tfc2, B, t, f)));
    };
    int t = T, f = Fs;
    for (int i = 0; i < cf.num_scales; ++i, t /= 2, f /= 2) {
      ps_blocks(n.enc[i], t, f);
      ps_blocks(n.dec[cf.num_scales - 1 - i], t, f);
    }
    ps_blocks(n.mid, t, f);
    CHK(e->c3h_ps.ensure(ps));
  }
  CHK(n.out_spec.ensure((size_t)B * cf.num_targets * dim_c * P0 * 4));
  CHK(n.frames.ensure((size_t)B * cf.num_targets * 2 * T * e->cfg.n_fft * 4));
  n.ws_batch = B;
  return ASX_OK;
}

// spec (cws layout) is already in cat0[:, 0:dim_c]; result spec goes to out_spec [B, S*dim_c, T, Fs]
static int v3_core_dev(asx_engine *e, int B, hipStream_t s) {
  V3Net &n = *e->v3;
  const asx_v3_config &cf = n.cfg;
  const int T = e->cfg.segment_size, k = cf.num_subbands, Fs = e->cfg.dim_f / k;
  const int dim_c = k * cf.num_channels * 2;
  const int c0 = cf.num_channels_model;
  const int64_t P0 = (int64_t)T * Fs;
  const int64_t cat_bs = (int64_t)(dim_c + c0) * P0;
  {
    ConvView v;
    v.x_bstride = cat_bs;
    CHK(conv_launch(e, n.first, n.cat0.f(), nullptr, n.firstout.f(), B, T, Fs, s, v));
  }
  V3View x{n.firstout.f(), (int64_t)c0 * P0};
  int c = c0, t = T, f = Fs;
  for (int i = 0; i < cf.num_scales; ++i) {
    const int64_t P = (int64_t)t * f;
    V3View skip{n.lvl[i].f() + (int64_t)c * P, (int64_t)2 * c * P};   // second half of the decoder concat buffer
    CHK(v3_tfc_tdf(e, n.enc[i], x, skip, B, t, f, s));
    CHK(v3_norm_act(e, n.ds_n[i], skip, c, P, B, n.A.f(), s));
    CHK(conv_launch(e, n.ds[i], n.A.f(), nullptr, n.CUR.f(), B, t, f, s));
    c += cf.growth;
    t /= 2;
    f /= 2;
    x = V3View{n.CUR.f(), (int64_t)c * t * f};
  }
  CHK(v3_tfc_tdf(e, n.mid, x, V3View{n.CUR.f(), (int64_t)c * t * f}, B, t, f, s));
  for (int i = 0; i < cf.num_scales; ++i) {
    const int lv = cf.num_scales - 1 - i;
    const int64_t Pin = (int64_t)t * f;
    CHK(v3_norm_act(e, n.us_n[i], V3View{n.CUR.f(), (int64_t)c * Pin}, c, Pin, B, n.A.f(), s));
    const int co = c - cf.growth;
    const int64_t Pout = Pin * 4;
    ConvView v;
    v.y_bstride = (int64_t)2 * co * Pout;            // first half of the concat buffer (torch.cat([x, skip], 1))
    v.act = ACT_NONE;
    CHK(conv_launch(e, n.us[i], n.A.f(), nullptr, n.lvl[lv].f(), B, t, f, s, v));
    c = co;
    t *= 2;
    f *= 2;
    CHK(v3_tfc_tdf(e, n.dec[i], V3View{n.lvl[lv].f(), (int64_t)2 * c * Pout}, V3View{n.CUR.f(), (int64_t)c * Pout}, B, t,
                   f, s));
  }
  // x * first_conv_out -> cat0[:, dim_c:]   (tfc_tdf_v3.py:257-259)
  {
    const int64_t CP = (int64_t)c0 * P0;
    const unsigned gx = (unsigned)std::min<int64_t>((CP + 255) / 256, 4096);
    float *ydst = n.cat0.f() + (int64_t)dim_c * P0;
    CHK(timed(e, ASX_PROF_MISC, 0.0, 12.0 * B * CP, s, [&]() {
      hipLaunchKernelGGL(mul_into_view_kernel, dim3(gx, B), dim3(256), 0, s, n.CUR.f(), n.firstout.f(), CP, ydst,
                         cat_bs);
    }));
  }
  ConvView vf;
  vf.act = cf.act == V3_ACT_GELU ? ACT_GELU : cf.act == V3_ACT_ELU ? ACT_ELU : ACT_RELU;  // final_conv.1 is the same act module
  vf.alpha = n.act_alpha;
  CHK(conv_launch(e, n.final0, n.cat0.f(), nullptr, n.X1.f(), B, T, Fs, s, vf));
  CHK(conv_launch(e, n.final1, n.X1.f(), nullptr, n.out_spec.f(), B, T, Fs, s));
  return ASX_OK;
}

// the TFC-TDF v3 nets' STFT / iSTFT: [B, 4, T, F] planes cut into k subbands (cac2cws / cws2cac, tfc_tdf_v3.py:216-223), the forward
// writing into the first dim_c planes of a wider tensor (`bstride` floats per batch item), the inverse reading S stems per item
static StftGeom v3_stft_geom(int k, int64_t bstride, int front) {
  StftGeom g;
  g.subbands = k;
  g.out_bstride = bstride;
  g.trim = front;
  return g;
}
static IstftGeom v3_istft_geom(int k, int S, int64_t bstride) {
  IstftGeom g;
  g.subbands = k;
  g.n_inst = S;
  g.in_bstride = bstride;
  return g;
}

// chunk waves -> separated chunk waves [B, S, 2, C]; input either explicit chunks [B,2,C] (n_song < 0)
// or windows of the resident mix (song mode, front zeros = `front`); pc: a pass over a pool of songs -- chunk b is a window of ITS
// song (stft_pool_kernel), everything behind the STFT is the same code
static std::atomic<long long> g_v3_net_passes{0};   // calls of v3_chunks_dev since the process started (asx_counter "v3_net_passes")

static int v3_chunks_dev(asx_engine *e, const float *wave, const int64_t *d_starts, int64_t n_song, int front, int B,
                         float *out, hipStream_t s, const PoolChunks *pc = nullptr) {
  g_v3_net_passes.fetch_add(1);
  V3Net &n = *e->v3;
  const asx_v3_config &cf = n.cfg;
  const int T = e->cfg.segment_size, k = cf.num_subbands, Fs = e->cfg.dim_f / k;
  const int dim_c = k * cf.num_channels * 2;
  const int64_t C = (int64_t)e->cfg.hop_length * (T - 1);
  const int64_t P0 = (int64_t)T * Fs;
  CHK(v3_ensure_workspace(e, B));
  CHK(stft_launch(e, wave, d_starts, n_song, B, C, T, n.cat0.f(), v3_stft_geom(k, (int64_t)(dim_c + cf.num_channels_model) * P0, front), s,
                  pc));
  CHK(v3_core_dev(e, B, s));
  const int S = cf.num_targets;
  CHK(istft_launch(e, n.out_spec.f(), B, T, v3_istft_geom(k, S, (int64_t)S * dim_c * P0), n.frames.f(), s));
  CHK(ola_launch(e, n.frames.f(), e->d_env.f(), nullptr, B * S, T, C, out, s));
  return ASX_OK;
}

static double v3_flops(const asx_engine *e, int batch) {
  if (!e->v3 || !e->v3->begun) return 0.0;
  const asx_v3_config &cf = e->v3->cfg;
  const double T = e->cfg.segment_size, k = cf.num_subbands, Fs = e->cfg.dim_f / k;
  const double dim_c = k * cf.num_channels * 2;
  double c = cf.num_channels_model, t = T, f = Fs, fl = 2.0 * dim_c * c * T * Fs;
  auto tfc_tdf = [&](double in_c, double cc, double tt, double ff) {
    double r = 0;
    for (int j = 0; j < cf.num_blocks_per_scale; ++j) {
      r += 2.0 * in_c * cc * tt * ff;                                  // shortcut
      r += 2.0 * 9.0 * in_c * cc * tt * ff + 2.0 * 9.0 * cc * cc * tt * ff;  // tfc1, tfc2
      r += 2.0 * 2.0 * cc * tt * ff * (ff / cf.bottleneck_factor);     // two linears
      in_c = cc;
    }
    return r;
  };
  for (int i = 0; i < cf.num_scales; ++i) {
    fl += tfc_tdf(c, c, t, f);
    fl += 2.0 * 4.0 * c * (c + cf.growth) * (t / 2) * (f / 2);
    c += cf.growth;
    t /= 2;
    f /= 2;
  }
  fl += tfc_tdf(c, c, t, f);
  for (int i = 0; i < cf.num_scales; ++i) {
    fl += 2.0 * 4.0 * c * (c - cf.growth) * t * f;
    c -= cf.growth;
    t *= 2;
    f *= 2;
    fl += tfc_tdf(2 * c, c, t, f);
  }
  fl += 2.0 * (c + dim_c) * c * T * Fs + 2.0 * c * cf.num_targets * dim_c * T * Fs;
  return fl * batch;
}
