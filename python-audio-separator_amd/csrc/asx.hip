// libasx.so -- engine + C ABI (include/asx.h) of the MI355X demix path.
//
// One engine = one GPU.  The engine owns: FFT tables, the packed ConvTDFNet
// weights, and a device workspace sized for `max_batch` chunks.  The chunk loop
// of MDXSeparator.demix (mdx_separator.py:348-392) is executed as batches of
// independent chunks: STFT -> net -> iSTFT -> fold+window per batch, then one
// gather pass folds all windowed chunks into the song (result / divider).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/asx.h"
#include "knobs.h"
#include "resample_plan.h"
#include "flac_dec_plan.h"

// Raise a kernel's dynamic-LDS limit to `bytes` unless an earlier call granted as much.  Engines are driven from several host threads
// (one per bag member / rank): one lock covers the record and the attribute call, so no launch can overtake the grant it needs.
static void grant_lds(const void *kernel, int bytes) {
  static std::mutex mu;
  static std::map<const void *, int> granted;
  std::lock_guard<std::mutex> lock(mu);
  int &g = granted[kernel];
  if (bytes > g) {
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    g = bytes;
  }
}
template <class K>
static void grant_lds(K *kernel, int bytes) { grant_lds(reinterpret_cast<const void *>(kernel), bytes); }

#include "kernels_fft.h"
#include "kernels_fft3.h"
#include "kernels_net.h"
#include "kernels_gemm2.h"
#include "kernels_gemm3.h"
#include "kernels_wino.h"
#ifdef ASX_EXPERIMENTAL_KERNELS
#include "kernels_winos.h"   // weight-stationary Winograd: measured slower (profiles/NOTES.md round 4)
#endif
#include "kernels_wino6.h"
#include "kernels_conv3h.h"
#include "kernels_updown6.h"
#include "kernels_rof.h"
#include "kernels_mdxc_pool.h"
#include "kernels_ht.h"
#include "kernels_halo.h"
#include "kernels_hd.h"
#include "kernels_vr.h"
#include "kernels_ens.h"
#include "kernels_resample.h"
#include "kernels_flac.h"
#include "kernels_pcm_encode.h"
#include "kernels_flac_dec.h"
#include "kernels_mix.h"
#include "kernels_phasefix.h"

using namespace asx;

#include "engine_core.h"
#include "engine_mdx.h"

// ----------------------------------------------------------------------------
// engine options (asx_set_option / asx_get_option)
// ----------------------------------------------------------------------------
static int opt_nonneg(int32_t v) { return v < 0 ? 0 : (int)v; }
static int opt_onoff(int32_t v) { return v > 0 ? 1 : 0; }

// One entry per option: where the engine keeps it, its default from the environment (knobs.h; asx_engine_create puts it through the same
// normaliser as asx_set_option) and, for an option that selects kernels only an experimental build carries, the refusal of the default
// build for positive values other than `shipped` (a printf format of the refused value).
static const struct EngineOption {
  const char *key;
  int asx_engine::*field;
  int EngineKnobs::*knob;
  int (*norm)(int32_t);
  const char *refusal = nullptr;
  int shipped = 0;
} kOptions[] = {
    {"winograd", &asx_engine::winograd, &EngineKnobs::winograd, opt_nonneg,
     "asx_set_option: winograd = %d names a superseded kernel generation that only an experimental build carries "
     "(python build.py --experimental); this library has 0 (direct kernel) and 3 (the default)", 3},
    {"winograd_stationary", &asx_engine::winos, &EngineKnobs::winos, opt_nonneg,
     "asx_set_option: the weight-stationary Winograd kernel (measured slower) is in experimental builds only (python build.py --experimental)"},
    {"winograd_bf16x6", &asx_engine::wino6, &EngineKnobs::wino6, opt_nonneg},
    {"gemm_bf16x6", &asx_engine::gemm_bf16x6, &EngineKnobs::gemm_bf16x6, opt_onoff},   // this engine only (round 5; it was process-wide before)
    {"gemm_f16x3", &asx_engine::gemm_f16x3, &EngineKnobs::gemm_f16x3, opt_onoff},
    {"gemm_f16x1", &asx_engine::gemm_f16x1, &EngineKnobs::gemm_f16x1, opt_onoff},   // opt-in reduced precision: one fp16 product per multiply-add (include/asx.h)
    {"conv_direct_f16x3", &asx_engine::conv3h, &EngineKnobs::conv3h, opt_nonneg},
    {"conv_fuse_input", &asx_engine::conv_fuse_input, &EngineKnobs::conv_fuse_input, opt_onoff},
    {"tdf_fuse_output", &asx_engine::tdf_fuse_output, &EngineKnobs::tdf_fuse_output, opt_onoff},
    {"conv3h_partial_scratch", &asx_engine::conv3h_ps, &EngineKnobs::conv3h_ps, opt_onoff},
    {"conv3h_walk", &asx_engine::conv3h_walk, &EngineKnobs::conv3h_walk, opt_onoff},
    {"conv3h_tiled", &asx_engine::conv3h_tiled, &EngineKnobs::conv3h_tiled, opt_onoff},
    {"conv3h_merge_out", &asx_engine::conv3h_merge, &EngineKnobs::conv3h_merge, opt_nonneg},
    {"conv_down_bf16x6", &asx_engine::down6, &EngineKnobs::down6, opt_onoff},
    {"conv_up_bf16x6", &asx_engine::up6, &EngineKnobs::up6, opt_onoff},
    {"gemm_pair_images", &asx_engine::pair_images, &EngineKnobs::pair_images, opt_onoff,
     "asx_set_option: gemm_pair_images = 1 needs an experimental build (python build.py --experimental): the pair-image reader measured no "
     "faster in the nets and is not in the default library"},
};

static const EngineOption *find_option(const char *fn, const char *key) {
  for (const EngineOption &o : kOptions)
    if (!strcmp(key, o.key)) return &o;
  set_err("%s: unknown option '%s'", fn, key);
  return nullptr;
}

// ----------------------------------------------------------------------------
// C ABI
// ----------------------------------------------------------------------------
extern "C" {

int asx_abi_version(void) { return ASX_ABI_VERSION; }
const char *asx_last_error(void) { return g_err; }

int asx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int asx_engine_create(int device, const asx_mdx_config *cfg, asx_engine **out) {
  REQUIRE(cfg && out, "asx_engine_create: null argument");
  REQUIRE(cfg->n_fft >= 8 && cfg->n_fft % 2 == 0, "n_fft must be even and >= 8 (got %d)", cfg->n_fft);
  REQUIRE(cfg->hop_length > 0 && cfg->segment_size >= 2, "bad hop_length/segment_size");
  REQUIRE(cfg->dim_f > 0 && cfg->dim_f <= cfg->n_fft / 2 + 1, "dim_f %d out of range for n_fft %d", cfg->dim_f,
          cfg->n_fft);
  REQUIRE(cfg->overlap >= 0.0 && cfg->overlap < 1.0, "overlap must be in [0,1)");
  REQUIRE(cfg->win_length >= 0 && cfg->win_length <= cfg->n_fft, "win_length %d out of range for n_fft %d", cfg->win_length, cfg->n_fft);
  const int64_t C = (int64_t)cfg->hop_length * (cfg->segment_size - 1);
  REQUIRE(C > cfg->n_fft / 2, "chunk_size %lld must exceed n_fft/2 (reflect padding)", (long long)C);
  REQUIRE(C - cfg->n_fft > 0, "chunk_size %lld must exceed n_fft (gen_size > 0)", (long long)C);
  FftPlan plan{};
  REQUIRE(make_plan(cfg->n_fft, &plan), "n_fft/2 = %d must factor into {2,3,5}", cfg->n_fft / 2);
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  REQUIRE(device >= 0 && device < ndev, "device %d not available (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  (void)knobs();                                       // the process-wide knobs: read once, here at the first engine
  const EngineKnobs opts;                              // this engine's option defaults: read again for every engine
  asx_engine *e = new asx_engine();
  for (const EngineOption &o : kOptions) e->*o.field = o.norm(opts.*o.knob);
  e->device = device;
  e->cfg = *cfg;
  e->plan = plan;
  std::vector<float> w;
  host_window(cfg->n_fft, w, cfg->win_length);
  std::vector<float> tw((size_t)cfg->n_fft * 2);
  for (int j = 0; j < cfg->n_fft; ++j) {
    const double ang = -2.0 * M_PI * (double)j / (double)cfg->n_fft;
    tw[2 * j] = (float)cos(ang);
    tw[2 * j + 1] = (float)sin(ang);
  }
  std::vector<float> env;
  host_env(cfg->n_fft, cfg->hop_length, cfg->segment_size, env, cfg->win_length);
  int rc = ASX_OK;
  if ((rc = e->d_window.ensure(w.size() * 4)) == ASX_OK && (rc = e->d_tw.ensure(tw.size() * 4)) == ASX_OK &&
      (rc = e->d_env.ensure(env.size() * 4)) == ASX_OK) {
    if (hipMemcpy(e->d_window.p, w.data(), w.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->d_tw.p, tw.data(), tw.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(e->d_env.p, env.data(), env.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
      set_err("table upload failed");
      rc = ASX_ERR_HIP;
    }
  }
  if (rc == ASX_OK && cfg->n_fft == f3::NFFT && cfg->hop_length == f3::HOP && opts.fft3) {
    std::vector<float> t3((size_t)(16 * 12 + 16 * f3::NB) * 2);
    for (int r = 0; r < 16; ++r)
      for (int k = 0; k < 12; ++k) {
        const double ang = -2.0 * M_PI * (double)(k * r) / 192.0;
        t3[(size_t)(r * 12 + k) * 2] = (float)cos(ang);
        t3[(size_t)(r * 12 + k) * 2 + 1] = (float)sin(ang);
      }
    for (int r = 0; r < 16; ++r)
      for (int j = 0; j < f3::NB; ++j) {
        const double ang = -2.0 * M_PI * (double)(j * r) / (double)f3::NH;
        t3[(size_t)(16 * 12 + r * f3::NB + j) * 2] = (float)cos(ang);
        t3[(size_t)(16 * 12 + r * f3::NB + j) * 2 + 1] = (float)sin(ang);
      }
    if ((rc = e->d_tw3.ensure(t3.size() * 4)) == ASX_OK) {
      if (hipMemcpy(e->d_tw3.p, t3.data(), t3.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        set_err("table upload failed");
        rc = ASX_ERR_HIP;
      } else {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::stft3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::STFT3_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::istft3_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::ISTFT3_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::istft3p_kernel<0>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::ISTFT3P_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::istft3p_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::ISTFT3P_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::istft3p_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::ISTFT3P_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::istft3p_kernel<3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::ISTFT3P_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::stft3p_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::STFT3P_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::stft3_pool_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::STFT3_LDS_BYTES);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&f3::stft3p_pool_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  f3::STFT3P_LDS_BYTES);
        e->fft3 = true;
        e->fft3p = opts.fft3p;
        if ((rc = e->d_hann3.ensure((size_t)C * 8)) == ASX_OK) {
          hipLaunchKernelGGL(f3::hann3_table_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, nullptr, C,
                             reinterpret_cast<double *>(e->d_hann3.p));
          if (hipDeviceSynchronize() != hipSuccess) {
            set_err("hann table kernel failed");
            rc = ASX_ERR_HIP;
          }
        }
      }
    }
  }
  if (rc == ASX_OK) rc = e->d_zeros.ensure(256);
  if (rc == ASX_OK && hipMemset(e->d_zeros.p, 0, 256) != hipSuccess) {
    set_err("zero page init failed");
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&stft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)stft_lds(plan));
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&stft_pool_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)stft_lds(plan));
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&istft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)istft_lds(plan));
  }
  if (rc != ASX_OK) {
    asx_engine_destroy(e);
    return rc;
  }
  *out = e;
  return ASX_OK;
}

static void v3_destroy(V3Net *n);
static void rof_destroy(RofNet *n);
static void ht_destroy(HtNet *n);
static void hd_destroy(HdNet *n);
static void hd_drop_clones(asx_engine *e);
static void vr_destroy(VrNet *n);
static void ens_destroy(EnsCtx *c);
static void mix_destroy(MixCtx *c);
static void phase_destroy(PhaseCtx *c);
static void free_conv(ConvLayer &L) {
  L.w.release();
  L.b.release();
  L.wu.release();
  L.wu2.release();
  L.wu3.release();
  L.wus.release();
  L.wu6.release();
  L.wu6h.release();
  L.w3h.release();
  L.w1f.release();
  L.wof.release();
  L.wd6.release();
  L.wup6.release();
  L.gn_w.release();
  L.gn_b.release();
}
static void free_tdf(TdfLayer &L) {
  L.w.release();
  L.bias.release();
  L.scale.release();
  L.shift.release();
  L.gn_w.release();
  L.gn_b.release();
}
static void free_block(Block &b) {
  for (auto &c : b.tfc) free_conv(c);
  free_tdf(b.tdf0);
  free_tdf(b.tdf1);
}

void asx_engine_destroy(asx_engine *e) {
  w3_flush(e);
  if (!e) return;
  (void)hipSetDevice(e->device);
  for (auto &r : e->recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  if (e->div_ev) (void)hipEventDestroy(e->div_ev);
  e->sinc_tab.release();
  e->gstats_part.release();
  e->sinc_jobs.release();
  e->flac_frames.release();
  e->flac_cycles.release();
  e->flac_off.release();
  e->flacdec_list.release();
  e->flacdec_slots.release();
  e->flacdec_accept.release();
  for (RsTable *t : e->rs_tabs) {
    t->tab.release();
    delete t;
  }
  e->rs_tabs.clear();
  e->d_window.release();
  e->d_tw.release();
  e->d_env.release();
  e->d_tw3.release();
  e->d_hann3.release();
  e->seam3.release();
  e->d_zeros.release();
  free_conv(e->first);
  free_conv(e->final_);
  for (auto &b : e->enc) free_block(b);
  for (auto &b : e->dec) free_block(b);
  free_block(e->mid);
  for (auto &c : e->ds) free_conv(c);
  for (auto &c : e->us) free_conv(c);
  e->spec_in.release();
  e->spec_out.release();
  for (auto &r : e->R) r.release();
  e->c3h_ps.release();
  for (Conv3hWalkTab *t : e->c3h_walks) {
    t->tab.release();
    delete t;
  }
  e->c3h_walks.clear();
  e->H.release();
  e->frames.release();
  e->chunk_out.release();
  e->d_starts.release();
  e->d_nact.release();
  e->d_peak.release();
  e->d_demixed.release();
  e->d_div.release();
  for (DevBuf *b : {&e->pool_wave, &e->pool_nsong, &e->pool_songs, &e->pool_div, &e->pool_peak}) b->release();
  for (auto &sk : e->skip) sk.release();
  if (e->v3) v3_destroy(e->v3);
  if (e->rof) rof_destroy(e->rof);
  hd_drop_clones(e);
  if (e->ht) ht_destroy(e->ht);
  if (e->hd) hd_destroy(e->hd);
  if (e->vr) vr_destroy(e->vr);
  if (e->ens) ens_destroy(e->ens);
  if (e->mix) mix_destroy(e->mix);
  if (e->phase) phase_destroy(e->phase);
  delete e;
}

// ---- weights ---------------------------------------------------------------
int asx_net_begin(asx_engine *e, const asx_net_config *cfg) {
  w3_flush(e);
  REQUIRE(e && cfg, "asx_net_begin: null argument");
  REQUIRE(cfg->dim_f == e->cfg.dim_f, "net dim_f %d != engine dim_f %d", cfg->dim_f, e->cfg.dim_f);
  REQUIRE(cfg->dim_t == e->cfg.segment_size, "net dim_t %d != segment_size %d", cfg->dim_t, e->cfg.segment_size);
  REQUIRE(cfg->k == 3, "only k=3 TFC kernels are supported (got %d)", cfg->k);
  REQUIRE(cfg->dim_c > 0 && cfg->g > 0 && cfg->l > 0 && cfg->bn >= -1, "bad net hyper-parameters");
  REQUIRE(cfg->norm == 0 || (cfg->norm == 1 && cfg->g % 2 == 0), "norm must be 0 (BatchNorm, folded by the host) or 1 (GroupNorm(2, c): even g)");
  REQUIRE(cfg->num_blocks >= 1 && cfg->num_blocks % 2 == 1, "num_blocks must be odd");
  const int n = cfg->num_blocks / 2;
  REQUIRE((cfg->dim_f % (1 << n)) == 0 && (cfg->dim_t % (1 << n)) == 0,
          "dim_f and dim_t must be divisible by 2^%d", n);
  REQUIRE(cfg->bn <= 0 || ((cfg->dim_f >> n) % cfg->bn) == 0, "dim_f / 2^n must be divisible by bn");
  e->net = *cfg;
  e->host_tensors.clear();
  e->net_begun = true;
  e->net_ready = false;
  return ASX_OK;
}

int asx_net_set_tensor(asx_engine *e, const char *name, const float *host, int64_t numel) {
  REQUIRE(e && name && host && numel > 0, "asx_net_set_tensor: bad argument");
  if (!e->net_begun) {
    set_err("asx_net_set_tensor before asx_net_begin");
    return ASX_ERR_STATE;
  }
  e->host_tensors[name].assign(host, host + numel);
  return ASX_OK;
}

static int get_tensor(asx_engine *e, const std::string &name, int64_t numel, const float **out, bool optional = false) {
  auto it = e->host_tensors.find(name);
  if (it == e->host_tensors.end()) {
    if (optional) {
      *out = nullptr;
      return ASX_OK;
    }
    set_err("missing tensor '%s'", name.c_str());
    return ASX_ERR_INVALID;
  }
  if ((int64_t)it->second.size() != numel) {
    set_err("tensor '%s': expected %lld elements, got %zu", name.c_str(), (long long)numel, it->second.size());
    return ASX_ERR_INVALID;
  }
  *out = it->second.data();
  return ASX_OK;
}

// GroupNorm affine of a layer: "<name>.gn_w" / "<name>.gn_b" [c] (asx_net_config.norm == 1)
static int load_gn(asx_engine *e, const std::string &name, int c, DevBuf &gw, DevBuf &gb) {
  const float *w, *b;
  CHK(get_tensor(e, name + ".gn_w", c, &w));
  CHK(get_tensor(e, name + ".gn_b", c, &b));
  CHK(gw.ensure((size_t)c * 4));
  CHK(gb.ensure((size_t)c * 4));
  HIPCHK(hipMemcpy(gw.p, w, (size_t)c * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(gb.p, b, (size_t)c * 4, hipMemcpyHostToDevice));
  return ASX_OK;
}

static int build_block(asx_engine *e, Block &blk, const std::string &pre, int c, int t, int f) {
  const asx_net_config &n = e->net;
  const bool gn = n.norm == 1;
  blk.c = c;
  blk.t = t;
  blk.f = f;
  blk.tfc.resize(n.l);
  for (int j = 0; j < n.l; ++j) {
    const float *w, *b;
    const std::string nm = pre + ".tfc" + std::to_string(j);
    CHK(get_tensor(e, nm + ".w", (int64_t)c * c * 9, &w));
    CHK(get_tensor(e, nm + ".b", c, &b));
    CHK(conv_setup(blk.tfc[j], CK_3X3, c, c, gn ? 0 : 1));
    CHK(conv_pack(blk.tfc[j], w, b, e->winograd));
    if (gn) CHK(load_gn(e, nm, c, blk.tfc[j].gn_w, blk.tfc[j].gn_b));
  }
  if (n.bn < 0) return ASX_OK;                         // bn is None: no TDF branch (modules.py:52)
  const int fb = n.bn == 0 ? f : f / n.bn;             // bn == 0: ONE Linear(f, f) (modules.py:55-60)
  const float *w, *bias, *sc = nullptr, *sh = nullptr;
  CHK(get_tensor(e, pre + ".tdf0.w", (int64_t)fb * f, &w));
  CHK(get_tensor(e, pre + ".tdf0.bias", fb, &bias, !n.tdf_bias));
  if (!gn) {
    CHK(get_tensor(e, pre + ".tdf0.scale", c, &sc));
    CHK(get_tensor(e, pre + ".tdf0.shift", c, &sh));
  }
  CHK(tdf_pack(blk.tdf0, fb, f, c, w, bias, sc, sh));
  if (gn) CHK(load_gn(e, pre + ".tdf0", c, blk.tdf0.gn_w, blk.tdf0.gn_b));
  if (n.bn == 0) return ASX_OK;
  CHK(get_tensor(e, pre + ".tdf1.w", (int64_t)f * fb, &w));
  CHK(get_tensor(e, pre + ".tdf1.bias", f, &bias, !n.tdf_bias));
  if (!gn) {
    CHK(get_tensor(e, pre + ".tdf1.scale", c, &sc));
    CHK(get_tensor(e, pre + ".tdf1.shift", c, &sh));
  }
  CHK(tdf_pack(blk.tdf1, f, fb, c, w, bias, sc, sh));
  if (gn) CHK(load_gn(e, pre + ".tdf1", c, blk.tdf1.gn_w, blk.tdf1.gn_b));
  return ASX_OK;
}

int asx_net_commit(asx_engine *e) {
  w3_flush(e);
  REQUIRE(e, "asx_net_commit: null engine");
  if (!e->net_begun) {
    set_err("asx_net_commit before asx_net_begin");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  const asx_net_config &n = e->net;
  const int nn = n.num_blocks / 2;
  const float *w, *b;
  CHK(get_tensor(e, "first.w", (int64_t)n.g * n.dim_c, &w));
  CHK(get_tensor(e, "first.b", n.g, &b));
  const bool gn = n.norm == 1;
  CHK(conv_setup(e->first, CK_1X1, n.dim_c, n.g, gn ? 0 : 1));
  CHK(conv_pack(e->first, w, b, e->winograd));
  if (gn) CHK(load_gn(e, "first", n.g, e->first.gn_w, e->first.gn_b));
  e->enc.assign(nn, Block());
  e->dec.assign(nn, Block());
  e->ds.assign(nn, ConvLayer());
  e->us.assign(nn, ConvLayer());
  int c = n.g, t = n.dim_t, f = n.dim_f;
  for (int i = 0; i < nn; ++i) {
    CHK(build_block(e, e->enc[i], "enc" + std::to_string(i), c, t, f));
    CHK(get_tensor(e, "ds" + std::to_string(i) + ".w", (int64_t)(c + n.g) * c * 4, &w));
    CHK(get_tensor(e, "ds" + std::to_string(i) + ".b", c + n.g, &b));
    CHK(conv_setup(e->ds[i], CK_DOWN, c, c + n.g, gn ? 0 : 1));
    CHK(conv_pack(e->ds[i], w, b, e->winograd));
    if (gn) CHK(load_gn(e, "ds" + std::to_string(i), c + n.g, e->ds[i].gn_w, e->ds[i].gn_b));
    c += n.g;
    t /= 2;
    f /= 2;
  }
  CHK(build_block(e, e->mid, "mid", c, t, f));
  for (int i = 0; i < nn; ++i) {
    CHK(get_tensor(e, "us" + std::to_string(i) + ".w", (int64_t)c * (c - n.g) * 4, &w));
    CHK(get_tensor(e, "us" + std::to_string(i) + ".b", c - n.g, &b));
    CHK(conv_setup(e->us[i], CK_UP, c, c - n.g, gn ? 0 : 1));
    CHK(conv_pack(e->us[i], w, b, e->winograd));
    if (gn) CHK(load_gn(e, "us" + std::to_string(i), c - n.g, e->us[i].gn_w, e->us[i].gn_b));
    c -= n.g;
    t *= 2;
    f *= 2;
    CHK(build_block(e, e->dec[i], "dec" + std::to_string(i), c, t, f));
  }
  CHK(get_tensor(e, "final.w", (int64_t)n.dim_c * n.g, &w));
  CHK(get_tensor(e, "final.b", n.dim_c, &b));
  CHK(conv_setup(e->final_, CK_1X1, n.g, n.dim_c, 0));
  CHK(conv_pack(e->final_, w, b, e->winograd));
  e->host_tensors.clear();
  e->net_ready = true;
  return ASX_OK;
}

double asx_net_flops(const asx_engine *e, int32_t batch) {
  if (!e || !e->net_begun) return 0.0;
  const asx_net_config &d = e->net;
  const int n = d.num_blocks / 2;
  double fl = 2.0 * d.dim_c * d.g * (double)d.dim_t * d.dim_f;
  auto block = [&](double c, double t, double f) {
    const double tdf = d.bn > 0 ? 2.0 * 2.0 * c * t * f * (f / d.bn) : (d.bn == 0 ? 2.0 * c * t * f * f : 0.0);
    return d.l * 2.0 * 9.0 * c * c * t * f + tdf;
  };
  double c = d.g, t = d.dim_t, f = d.dim_f;
  for (int i = 0; i < n; ++i) {
    fl += block(c, t, f);
    fl += 2.0 * 4.0 * c * (c + d.g) * (t / 2) * (f / 2);
    c += d.g;
    t /= 2;
    f /= 2;
  }
  fl += block(c, t, f);
  for (int i = 0; i < n; ++i) {
    fl += 2.0 * 4.0 * c * (c - d.g) * t * f;
    c -= d.g;
    t *= 2;
    f *= 2;
    fl += block(c, t, f);
  }
  fl += 2.0 * d.g * d.dim_c * (double)d.dim_t * d.dim_f;
  return fl * batch;
}

}  // extern "C" (the engine headers below define templates)
#include "engine_v3.h"
#include "engine_attn.h"
#include "engine_rof.h"
#include "engine_ht.h"
#include "engine_hd.h"
#include "engine_vr.h"
#include "engine_ens.h"
#include "engine_resample.h"
#include "engine_flac.h"
#include "engine_flac_dec.h"
#include "engine_mix.h"
#include "engine_phasefix.h"
extern "C" {

// ---- plan ------------------------------------------------------------------
// torch.stft / istft `window=`: a table of n_fft floats (a window function evaluated over win_length, zero padded to n_fft at both
// ends like torch does) replacing the periodic Hann built at engine creation -- BSRoformer's `stft_window_fn` (bs_roformer.py:333, 386).
int asx_set_stft_window(asx_engine *e, const float *window_host, int32_t n) {
  REQUIRE(e && window_host, "asx_set_stft_window: null argument");
  REQUIRE(n == e->cfg.n_fft, "asx_set_stft_window: %d values for n_fft %d", n, e->cfg.n_fft);
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  e->custom_window.assign(window_host, window_host + n);
  std::vector<float> env;
  host_env(n, e->cfg.hop_length, e->cfg.segment_size, env, e->cfg.win_length, &e->custom_window);
  HIPCHK(hipMemcpy(e->d_window.p, window_host, (size_t)n * 4, hipMemcpyHostToDevice));
  CHK(e->d_env.ensure(env.size() * 4));
  HIPCHK(hipMemcpy(e->d_env.p, env.data(), env.size() * 4, hipMemcpyHostToDevice));
  if (e->rof) e->rof->win_synth.release();             // rebuilt from the new table at the next forward
  return ASX_OK;
}

int asx_plan_query(const asx_engine *e, int64_t N, uint32_t flags, asx_plan *out) {
  REQUIRE(e && out, "asx_plan_query: null argument");
  REQUIRE(N >= 1, "n_samples must be >= 1 (an empty mix raises in the reference, common_separator.py:267)");
  const bool match = (flags & ASX_FLAG_MATCH_MIX) != 0;
  // python: overlap is a float (double); 0.02 for the match-mix pass (mdx_separator.py:311)
  const double overlap = match ? 0.02 : e->cfg.overlap;
  asx_plan p{};
  p.n_samples = N;
  p.trim = e->cfg.n_fft / 2;
  p.chunk_size = (int64_t)e->cfg.hop_length * (e->cfg.segment_size - 1);
  p.gen_size = p.chunk_size - 2 * p.trim;
  p.pad = p.gen_size + p.trim - (N % p.gen_size);
  p.padded_len = p.trim + N + p.pad;
  p.step = (int64_t)((1.0 - overlap) * (double)p.chunk_size);  // int() truncation (mdx_separator.py:335)
  REQUIRE(p.step >= 1, "overlap too close to 1: step == 0");
  p.n_chunks = (int32_t)((p.padded_len + p.step - 1) / p.step);
  p.n_frames = e->cfg.segment_size;
  *out = p;
  return ASX_OK;
}

// ---- chunk batches -----------------------------------------------------------
__global__ void chunk_table_kernel(int k0, int nk, int64_t step, int64_t chunk, int64_t padded_len, int win,
                                   int64_t *__restrict__ starts, int64_t *__restrict__ nact) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nk) return;
  const int64_t st = (int64_t)(k0 + i) * step;
  const int64_t na = chunk < padded_len - st ? chunk : padded_len - st;
  starts[i] = st;
  nact[i] = win ? na : -1;
}

static bool windowed_mode(const asx_engine *e, uint32_t flags) {
  return (flags & ASX_FLAG_MATCH_MIX) ? true : (e->cfg.overlap != 0.0);
}

int asx_demix_chunks_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t k0, int32_t k1,
                         float *chunk_out_dev, uint32_t flags, void *stream) {
  REQUIRE(e && mix_dev && chunk_out_dev, "asx_demix_chunks_dev: null argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  asx_plan p;
  CHK(asx_plan_query(e, N, flags, &p));
  REQUIRE(k0 >= 0 && k1 <= p.n_chunks && k0 <= k1, "chunk range [%d,%d) outside [0,%d)", k0, k1, p.n_chunks);
  const bool match = (flags & ASX_FLAG_MATCH_MIX) != 0;
  const bool need_net = !match;
  if (need_net && !e->net_ready) {
    set_err("asx_demix: net weights not committed");
    return ASX_ERR_STATE;
  }
  const int nk = k1 - k0;
  if (nk == 0) return ASX_OK;
  const int per = even_batches(nk, pick_batch(e));
  CHK(ensure_workspace(e, per, need_net));
  if (need_net && nk % per) CHK(net_walks_ensure(e, (nk % per) * (e->cfg.enable_denoise ? 2 : 1)));   // the last, shorter pass walks its own tables
  // chunk tables, built on the device: start of chunk k = k * step, active length = min(chunk, L - start), or negative
  // for "no chunk window" (overlap == 0, mdx_separator.py:389-390).  No host copy, no host synchronisation: the call
  // only enqueues work on `stream` (hipGraph-capturable, and a gather of step k can overlap the compute of step k + 1).
  const bool win = windowed_mode(e, flags);
  CHK(e->d_starts.ensure((size_t)nk * 8));
  CHK(e->d_nact.ensure((size_t)nk * 8));
  hipLaunchKernelGGL(chunk_table_kernel, dim3((unsigned)((nk + 255) / 256)), dim3(256), 0, s, k0, nk, p.step, p.chunk_size,
                     p.padded_len, win ? 1 : 0, reinterpret_cast<int64_t *>(e->d_starts.p), reinterpret_cast<int64_t *>(e->d_nact.p));
  HIPCHK(hipGetLastError());
  const int T = e->cfg.segment_size;
  const int64_t C = p.chunk_size;
  const size_t spec_elems = (size_t)4 * T * e->cfg.dim_f;
  for (int b0 = 0; b0 < nk; b0 += per) {
    const int B = std::min(per, nk - b0);
    const int64_t *ds = reinterpret_cast<const int64_t *>(e->d_starts.p) + b0;
    const int64_t *dn = reinterpret_cast<const int64_t *>(e->d_nact.p) + b0;
    CHK(stft_launch(e, mix_dev, ds, N, B, C, T, e->spec_in.f(), 1, 3, 1.0f, s));
    const float *spec_final = e->spec_in.f();
    int combine = 0;
    if (need_net) {
      int Bn = B;
      if (e->cfg.enable_denoise) {
        // second half of the batch: the negated spectrum (mdx_separator.py:437)
        CHK(stft_launch(e, mix_dev, ds, N, B, C, T, e->spec_in.f() + (size_t)B * spec_elems, 1, 3, -1.0f, s));
        Bn = 2 * B;
        combine = B;
      }
      CHK(net_forward_dev(e, e->spec_in.f(), e->spec_out.f(), Bn, s));
      spec_final = e->spec_out.f();
    }
    CHK(istft_ola_launch(e, spec_final, B, T, combine, dn, C, chunk_out_dev + (size_t)b0 * 2 * C, s));
  }
  return ASX_OK;
}

int asx_finalize_dev(asx_engine *e, const float *chunk_out_dev, int64_t N, float *out_dev, uint32_t flags,
                     void *stream) {
  REQUIRE(e && chunk_out_dev && out_dev, "asx_finalize_dev: null argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  asx_plan p;
  CHK(asx_plan_query(e, N, flags, &p));
  const int win = windowed_mode(e, flags) ? 1 : 0;
  const double bytes = 4.0 * ((double)p.n_chunks * 2 * p.chunk_size + 2.0 * N);
  const double *hann = (e->fft3 && e->d_hann3.p) ? reinterpret_cast<const double *>(e->d_hann3.p) : nullptr;
  const bool fin4 = knobs().finalize4;
  // vector path: the divider (input-independent) comes from a table built once per plan; needs 4-sample alignment of the
  // chunk geometry and 16-byte aligned buffers
  if (fin4 && p.chunk_size % 4 == 0 && p.step % 4 == 0 && p.trim % 4 == 0 && N % 4 == 0 && p.chunk_size + (int64_t)p.trim >= 0 &&
      (((uintptr_t)chunk_out_dev | (uintptr_t)out_dev) & 15) == 0) {
    const DivKey key{N, p.n_chunks, p.chunk_size, p.step, p.padded_len, p.trim, win, hann != nullptr ? 1 : 0};
    if (!(e->div_key == key) || !e->d_div.p) {
      CHK(e->d_div.ensure((size_t)N * 4));
      CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * N, s, [&]() {
        hipLaunchKernelGGL(finalize_div_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, p.n_chunks, p.chunk_size, p.step,
                           p.padded_len, p.trim, N, win, e->d_div.f(), hann);
      }));
      e->div_key = key;
      // the table is shared by later calls: a call on a different stream must be ordered behind this build
      if (e->div_ev == nullptr) HIPCHK(hipEventCreateWithFlags(&e->div_ev, hipEventDisableTiming));
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(s, &cap);
      if (cap == hipStreamCaptureStatusNone) {
        HIPCHK(hipEventRecord(e->div_ev, s));
        e->div_stream = s;
      } else {
        e->div_stream = s;          // built inside a capture: the graph owns the ordering, nothing to wait for outside it
      }
    } else if (s != e->div_stream && e->div_ev != nullptr && hipEventQuery(e->div_ev) == hipErrorNotReady) {
      HIPCHK(hipStreamWaitEvent(s, e->div_ev, 0));
    }
    return timed(e, ASX_PROF_FINALIZE, 0.0, bytes, s, [&]() {
      hipLaunchKernelGGL(finalize4_kernel, dim3((unsigned)((N / 4 + 255) / 256), 2), dim3(256), 0, s, chunk_out_dev, p.n_chunks,
                         p.chunk_size, p.step, p.padded_len, p.trim, N, e->d_div.f(), out_dev);
    });
  }
  return timed(e, ASX_PROF_FINALIZE, 0.0, bytes, s, [&]() {
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((N + 255) / 256), 2), dim3(256), 0, s, chunk_out_dev,
                       p.n_chunks, p.chunk_size, p.step, p.padded_len, p.trim, N, win, out_dev, hann);
  });
}

int asx_demix_dev(asx_engine *e, const float *mix_dev, int64_t N, float *out_dev, uint32_t flags, void *stream) {
  REQUIRE(e && mix_dev && out_dev, "asx_demix_dev: null argument");
  HIPCHK(hipSetDevice(e->device));
  asx_plan p;
  CHK(asx_plan_query(e, N, flags, &p));
  CHK(e->chunk_out.ensure((size_t)p.n_chunks * 2 * p.chunk_size * 4));
  CHK(asx_demix_chunks_dev(e, mix_dev, N, 0, p.n_chunks, e->chunk_out.f(), flags, stream));
  CHK(asx_finalize_dev(e, e->chunk_out.f(), N, out_dev, flags, stream));
  return ASX_OK;
}

// ---- a batch of songs, their chunks pooled per launch ---------------------------------------------------------
// The demix of n songs (validated by the caller) on device buffers: one chunk list over all songs, walked in batches of up to
// pick_batch(e) chunks that may straddle songs -- the STFT / net / iSTFT launch count depends on the total chunk count only --
// then one divider build per distinct length and ONE segmented fold.  Every buffer is sized before the first launch.
static int demix_pool_dev(asx_engine *e, const float *const *mix, float *const *out, const int64_t *Ns, int n, uint32_t flags,
                          hipStream_t s) {
  const bool match = (flags & ASX_FLAG_MATCH_MIX) != 0;
  const bool need_net = !match;
  if (need_net && !e->net_ready) {
    set_err("asx_demix: net weights not committed");
    return ASX_ERR_STATE;
  }
  std::vector<asx_plan> plans((size_t)n);
  std::vector<int> chunk0((size_t)n + 1, 0);
  int64_t total = 0;
  for (int i = 0; i < n; ++i) {
    CHK(asx_plan_query(e, Ns[i], flags, &plans[i]));
    total += plans[i].n_chunks;
    REQUIRE(total < ((int64_t)1 << 30), "asx_demix_batch_dev: %lld chunks in one pool", (long long)total);
    chunk0[i + 1] = (int)total;
  }
  const int nk = (int)total;
  const asx_plan &p0 = plans[0];                       // chunk geometry (everything but N, pad, padded_len, n_chunks) is the engine's
  const int64_t C = p0.chunk_size;
  const int T = e->cfg.segment_size;
  const bool win = windowed_mode(e, flags);
  const double *hann = (e->fft3 && e->d_hann3.p) ? reinterpret_cast<const double *>(e->d_hann3.p) : nullptr;
  const int maxB = pick_batch(e);
  const int nbatch = (nk + maxB - 1) / maxB;
  const int per = (nk + nbatch - 1) / nbatch;
  // dividers: one table per distinct length, 16-byte aligned slots
  std::map<int64_t, int64_t> div_off;                  // N -> floats into pool_div
  int64_t div_floats = 0;
  for (int i = 0; i < n; ++i)
    if (div_off.emplace(Ns[i], div_floats).second) div_floats += (Ns[i] + 3) / 4 * 4;
  CHK(ensure_workspace(e, per, need_net));
  if (need_net && nk % per) CHK(net_walks_ensure(e, (nk % per) * (e->cfg.enable_denoise ? 2 : 1)));
  CHK(e->d_starts.ensure((size_t)nk * 8));
  CHK(e->d_nact.ensure((size_t)nk * 8));
  CHK(e->pool_wave.ensure((size_t)nk * 8));
  CHK(e->pool_nsong.ensure((size_t)nk * 8));
  CHK(e->pool_songs.ensure((size_t)n * sizeof(PoolSong)));
  CHK(e->pool_div.ensure((size_t)div_floats * 4));
  CHK(e->chunk_out.ensure((size_t)nk * 2 * C * 4));
  if (e->fft3) CHK(e->seam3.ensure((size_t)per * 2 * std::max(1, T / knobs().fft3_g) * 2 * 5 * f3::HOP * 4));   // istft_ola_launch's, for the largest batch
  float *chunks = e->chunk_out.f();
  const bool geom4 = knobs().finalize4 && C % 4 == 0 && p0.step % 4 == 0 && p0.trim % 4 == 0;
  // tables
  int64_t blk = 0;
  for (int g0 = 0; g0 < n; g0 += POOL_GROUP) {
    PoolGroup g{};
    g.n_songs = std::min(POOL_GROUP, n - g0);
    g.song0 = g0;
    for (int i = 0; i < g.n_songs; ++i) {
      const int sidx = g0 + i;
      g.mix[i] = mix[sidx];
      g.out[i] = out[sidx];
      g.n[i] = Ns[sidx];
      g.div_off[i] = div_off[Ns[sidx]];
      g.chunk0[i] = chunk0[sidx];
      // the vector path of asx_finalize_dev, under its conditions, per song
      g.vec[i] = (geom4 && Ns[sidx] % 4 == 0 && (((uintptr_t)(chunks + (size_t)chunk0[sidx] * 2 * C) | (uintptr_t)out[sidx]) & 15) == 0) ? 1 : 0;
      g.blk0[i] = blk;
      blk += ((g.vec[i] ? Ns[sidx] / 4 : Ns[sidx]) + 255) / 256;
    }
    g.chunk0[g.n_songs] = chunk0[g0 + g.n_songs];
    const int nthr = g.chunk0[g.n_songs] - g.chunk0[0];
    hipLaunchKernelGGL(pool_table_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, g, p0.step, C, (int)p0.trim, p0.gen_size,
                       win ? 1 : 0, chunks, e->pool_div.f(), reinterpret_cast<const float **>(e->pool_wave.p),
                       reinterpret_cast<int64_t *>(e->pool_nsong.p), reinterpret_cast<int64_t *>(e->d_starts.p),
                       reinterpret_cast<int64_t *>(e->d_nact.p), reinterpret_cast<PoolSong *>(e->pool_songs.p));
    HIPCHK(hipGetLastError());
  }
  REQUIRE(blk < ((int64_t)1 << 31), "asx_demix_batch_dev: %lld samples in one pool", (long long)blk * 256);
  // chunks
  const size_t spec_elems = (size_t)4 * T * e->cfg.dim_f;
  for (int b0 = 0; b0 < nk; b0 += per) {
    const int B = std::min(per, nk - b0);
    const int64_t *ds = reinterpret_cast<const int64_t *>(e->d_starts.p) + b0;
    const int64_t *dn = reinterpret_cast<const int64_t *>(e->d_nact.p) + b0;
    const PoolChunks pc{reinterpret_cast<const float *const *>(e->pool_wave.p) + b0, reinterpret_cast<const int64_t *>(e->pool_nsong.p) + b0};
    CHK(stft_launch(e, nullptr, ds, 0, B, C, T, e->spec_in.f(), 1, 3, 1.0f, s, &pc));
    const float *spec_final = e->spec_in.f();
    int combine = 0;
    if (need_net) {
      int Bn = B;
      if (e->cfg.enable_denoise) {
        CHK(stft_launch(e, nullptr, ds, 0, B, C, T, e->spec_in.f() + (size_t)B * spec_elems, 1, 3, -1.0f, s, &pc));
        Bn = 2 * B;
        combine = B;
      }
      CHK(net_forward_dev(e, e->spec_in.f(), e->spec_out.f(), Bn, s));
      spec_final = e->spec_out.f();
    }
    CHK(istft_ola_launch(e, spec_final, B, T, combine, dn, C, chunks + (size_t)b0 * 2 * C, s));
  }
  // fold
  for (int i = 0; i < n; ++i) {
    const auto it = div_off.find(Ns[i]);
    if (it->second < 0) continue;                      // built for an earlier song of this length
    const asx_plan &p = plans[i];
    float *dv = e->pool_div.f() + it->second;
    CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * p.n_samples, s, [&]() {
      hipLaunchKernelGGL(finalize_div_kernel, dim3((unsigned)((p.n_samples + 255) / 256)), dim3(256), 0, s, p.n_chunks, p.chunk_size, p.step,
                         p.padded_len, p.trim, p.n_samples, win ? 1 : 0, dv, hann);
    }));
    it->second = -1;
  }
  double bytes = 0.0;
  for (int i = 0; i < n; ++i) bytes += 4.0 * ((double)plans[i].n_chunks * 2 * C + 3.0 * Ns[i]);
  return timed(e, ASX_PROF_FINALIZE, 0.0, bytes, s, [&]() {
    hipLaunchKernelGGL(finalize_pool_kernel, dim3((unsigned)blk, 2), dim3(256), 0, s, reinterpret_cast<const PoolSong *>(e->pool_songs.p), n, C,
                       p0.step, (int)p0.trim);
  });
}

int asx_demix_batch_dev(asx_engine *e, const asx_song *songs, int32_t n_songs, uint32_t flags, void *stream) {
  REQUIRE(e && n_songs >= 0 && (songs || n_songs == 0), "asx_demix_batch_dev: null argument");
  if (n_songs == 0) return ASX_OK;
  std::vector<const float *> mix((size_t)n_songs);
  std::vector<float *> out((size_t)n_songs);
  std::vector<int64_t> Ns((size_t)n_songs);
  for (int i = 0; i < n_songs; ++i) {                  // nothing is enqueued unless every song is valid
    REQUIRE(songs[i].mix_dev && songs[i].out_dev, "asx_demix_batch_dev: null pointer in song %d", i);
    REQUIRE(songs[i].n_samples >= 1, "asx_demix_batch_dev: song %d: n_samples must be >= 1", i);
    mix[i] = songs[i].mix_dev;
    out[i] = songs[i].out_dev;
    Ns[i] = songs[i].n_samples;
  }
  HIPCHK(hipSetDevice(e->device));
  return demix_pool_dev(e, mix.data(), out.data(), Ns.data(), n_songs, flags, reinterpret_cast<hipStream_t>(stream));
}

int asx_demix(asx_engine *e, const float *mix_host, int64_t N, float *out_host, uint32_t flags) {
  REQUIRE(e && mix_host && out_host, "asx_demix: null argument");
  REQUIRE(N >= 1, "n_samples must be >= 1");
  HIPCHK(hipSetDevice(e->device));
  DevBuf dmix, dout;
  int rc = dmix.ensure((size_t)2 * N * 4);
  if (rc == ASX_OK) rc = dout.ensure((size_t)2 * N * 4);
  if (rc == ASX_OK && hipMemcpy(dmix.p, mix_host, (size_t)2 * N * 4, hipMemcpyHostToDevice) != hipSuccess) {
    set_err("asx_demix: H2D copy failed");
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK) rc = asx_demix_dev(e, dmix.f(), N, dout.f(), flags, nullptr);
  if (rc == ASX_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
    set_err("asx_demix: device execution failed: %s", hipGetErrorString(hipGetLastError()));
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK && hipMemcpy(out_host, dout.p, (size_t)2 * N * 4, hipMemcpyDeviceToHost) != hipSuccess) {
    set_err("asx_demix: D2H copy failed");
    rc = ASX_ERR_HIP;
  }
  dmix.release();
  dout.release();
  return rc;
}

// ---- stem algebra ------------------------------------------------------------
int asx_separate_dev(asx_engine *e, float *mix_dev, int64_t N, float max_peak, float min_peak, int32_t has_min,
                     float compensate, float *primary_dev, float *secondary_dev, void *stream) {
  REQUIRE(e && mix_dev && primary_dev && secondary_dev, "asx_separate_dev: null argument");
  REQUIRE(N >= 1, "n_samples must be >= 1");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  CHK(e->d_demixed.ensure((size_t)2 * N * 4));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p);
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const int64_t n2 = 2 * N;
  const unsigned nb = (unsigned)std::min<int64_t>((n2 + 255) / 256, 2048);
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * n2, s, [&]() {
    hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, mix_dev, n2, pk);
  }));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 8.0 * n2, s, [&]() {
    hipLaunchKernelGGL(normalize_kernel, dim3(nb), dim3(256), 0, s, mix_dev, n2, pk, max_peak, min_peak, has_min);
  }));
  CHK(asx_demix_dev(e, mix_dev, N, e->d_demixed.f(), 0, stream));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * 4 * n2, s, [&]() {
    hipLaunchKernelGGL(stems_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, e->d_demixed.f(), mix_dev, N,
                       pk, compensate, primary_dev, secondary_dev);
  }));
  return ASX_OK;
}

// asx_separate_dev per song around ONE pooled demix: each song's own peak word, in-place normalise and stem algebra
int asx_separate_batch_dev(asx_engine *e, const asx_song_stems *songs, int32_t n_songs, float max_peak, float min_peak,
                           int32_t has_min, float compensate, void *stream) {
  REQUIRE(e && n_songs >= 0 && (songs || n_songs == 0), "asx_separate_batch_dev: null argument");
  if (n_songs == 0) return ASX_OK;
  std::vector<const float *> mix((size_t)n_songs);
  std::vector<float *> dem((size_t)n_songs);
  std::vector<int64_t> Ns((size_t)n_songs), off((size_t)n_songs);
  int64_t floats = 0;
  for (int i = 0; i < n_songs; ++i) {
    REQUIRE(songs[i].mix_dev && songs[i].primary_dev && songs[i].secondary_dev, "asx_separate_batch_dev: null pointer in song %d", i);
    REQUIRE(songs[i].n_samples >= 1, "asx_separate_batch_dev: song %d: n_samples must be >= 1", i);
    Ns[i] = songs[i].n_samples;
    off[i] = floats;
    floats += (2 * Ns[i] + 3) / 4 * 4;                 // 16-byte aligned slots, like a buffer of its own
  }
  if (!e->net_ready) {
    set_err("asx_demix: net weights not committed");
    return ASX_ERR_STATE;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->pool_peak.ensure((size_t)n_songs * 4));
  CHK(e->d_demixed.ensure((size_t)floats * 4));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->pool_peak.p);
  HIPCHK(hipMemsetAsync(pk, 0, (size_t)n_songs * 4, s));
  for (int i = 0; i < n_songs; ++i) {
    const int64_t n2 = 2 * Ns[i];
    const unsigned nb = (unsigned)std::min<int64_t>((n2 + 255) / 256, 2048);
    float *m = songs[i].mix_dev;
    CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * n2, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, m, n2, pk + i); }));
    CHK(timed(e, ASX_PROF_MISC, 0.0, 8.0 * n2, s, [&]() {
      hipLaunchKernelGGL(normalize_kernel, dim3(nb), dim3(256), 0, s, m, n2, pk + i, max_peak, min_peak, has_min);
    }));
    mix[i] = m;
    dem[i] = e->d_demixed.f() + off[i];
  }
  CHK(demix_pool_dev(e, mix.data(), dem.data(), Ns.data(), n_songs, 0, s));
  for (int i = 0; i < n_songs; ++i) {
    const int64_t N = Ns[i];
    CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * 4 * 2 * N, s, [&]() {
      hipLaunchKernelGGL(stems_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, dem[i], songs[i].mix_dev, N, pk + i, compensate,
                         songs[i].primary_dev, songs[i].secondary_dev);
    }));
  }
  return ASX_OK;
}

int asx_separate(asx_engine *e, float *mix_host, int64_t N, float max_peak, float min_peak, int32_t has_min,
                 float compensate, float *primary_host, float *secondary_host) {
  REQUIRE(e && mix_host && primary_host && secondary_host, "asx_separate: null argument");
  REQUIRE(N >= 1, "n_samples must be >= 1");
  HIPCHK(hipSetDevice(e->device));
  DevBuf dmix, dp, ds;
  const size_t bytes = (size_t)2 * N * 4;
  int rc = dmix.ensure(bytes);
  if (rc == ASX_OK) rc = dp.ensure(bytes);
  if (rc == ASX_OK) rc = ds.ensure(bytes);
  if (rc == ASX_OK && hipMemcpy(dmix.p, mix_host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
    set_err("asx_separate: H2D copy failed");
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK)
    rc = asx_separate_dev(e, dmix.f(), N, max_peak, min_peak, has_min, compensate, dp.f(), ds.f(), nullptr);
  if (rc == ASX_OK && hipStreamSynchronize(nullptr) != hipSuccess) {
    set_err("asx_separate: device execution failed: %s", hipGetErrorString(hipGetLastError()));
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK && (hipMemcpy(mix_host, dmix.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(primary_host, dp.p, bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(secondary_host, ds.p, bytes, hipMemcpyDeviceToHost) != hipSuccess)) {
    set_err("asx_separate: D2H copy failed");
    rc = ASX_ERR_HIP;
  }
  dmix.release();
  dp.release();
  ds.release();
  return rc;
}

// spec_utils.normalize(wave, max_peak, min_peak) (uvr_lib_v5/spec_utils.py:99-115) on any float32 array, in place:
// maxv = |wave|.max(); > max_peak: *= max_peak / maxv; else (min_peak given and maxv < min_peak): *= min_peak / maxv.
int asx_normalize(asx_engine *e, float *wave_host, int64_t numel, float max_peak, float min_peak, int32_t has_min, float *peak_before) {
  REQUIRE(e && wave_host && numel >= 1, "asx_normalize: bad argument");
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  DevBuf d;
  int rc = d.ensure((size_t)numel * 4);
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p);
  float maxv = 0.f;
  const unsigned nb = (unsigned)std::min<int64_t>((numel + 255) / 256, 2048);
  if (rc == ASX_OK && (hipMemcpy(d.p, wave_host, (size_t)numel * 4, hipMemcpyHostToDevice) != hipSuccess ||
                       hipMemsetAsync(pk, 0, 4, nullptr) != hipSuccess)) {
    set_err("asx_normalize: H2D copy failed");
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK) {
    hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, nullptr, d.f(), numel, pk);
    hipLaunchKernelGGL(normalize_kernel, dim3(nb), dim3(256), 0, nullptr, d.f(), numel, pk, max_peak, min_peak, has_min);
    if (hipGetLastError() != hipSuccess || hipMemcpy(&maxv, pk, 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(wave_host, d.p, (size_t)numel * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      set_err("asx_normalize: device execution failed");
      rc = ASX_ERR_HIP;
    }
  }
  if (peak_before) *peak_before = maxv;
  d.release();
  return rc;
}

// the same on an array that is already in HBM (MDXCSeparator.separate normalises the mix and every stem, mdxc_separator.py:147,
// 170-190): in place, only enqueues work
int asx_normalize_dev(asx_engine *e, float *wave_dev, int64_t numel, float max_peak, float min_peak, int32_t has_min, void *stream) {
  REQUIRE(e && wave_dev && numel >= 1, "asx_normalize_dev: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p) + 2;   // its own word (0: separate / pcm16, 1: decode)
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const unsigned nb = (unsigned)std::min<int64_t>((numel + 255) / 256, 2048);
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * numel, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, wave_dev, numel, pk); }));
  return timed(e, ASX_PROF_MISC, 0.0, 8.0 * numel, s, [&]() {
    hipLaunchKernelGGL(normalize_kernel, dim3(nb), dim3(256), 0, s, wave_dev, numel, pk, max_peak, min_peak, has_min);
  });
}

// out = mix - stem (the residual stem of a single-target MDXC / Roformer model, mdxc_separator.py:406-468), float32
int asx_residual_dev(asx_engine *e, const float *mix_dev, const float *stem_dev, float *out_dev, int64_t numel, void *stream) {
  REQUIRE(e && mix_dev && stem_dev && out_dev && numel >= 1, "asx_residual_dev: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const unsigned nb = (unsigned)std::min<int64_t>((numel + 255) / 256, 4096);
  return timed(e, ASX_PROF_MISC, 0.0, 12.0 * numel, s, [&]() {
    hipLaunchKernelGGL(residual_kernel, dim3(nb), dim3(256), 0, s, mix_dev, stem_dev, numel, out_dev);
  });
}

// librosa.resample(res_type="sinc_fastest") for an arbitrary ratio (engine_vr.h resample_sinc_dev)
int asx_resample_sinc_dev(asx_engine *e, const float *x_dev, int32_t channels, int64_t n_in, double ratio, int32_t mono_calls,
                          float *y_dev, int64_t n_out, void *stream) {
  REQUIRE(e && x_dev && y_dev && channels >= 1 && channels <= 65535 && n_in >= 1 && n_out >= 1, "asx_resample_sinc_dev: bad argument");
  REQUIRE(ratio > 1.0 / 256 && ratio < 256.0, "asx_resample_sinc_dev: ratio %g outside libsamplerate's (1/256, 256)", ratio);
  HIPCHK(hipSetDevice(e->device));
  return resample_sinc_dev(e, e->sinc_tab, x_dev, channels, n_in, ratio, mono_calls, y_dev, n_out, reinterpret_cast<hipStream_t>(stream));
}

// the same for a list of jobs at one ratio in one launch (engine_vr.h resample_sinc_batch_dev; the checks: sinc_pool_plan.h)
int asx_resample_sinc_batch_dev(asx_engine *e, const asx_sinc_job *jobs, int32_t n_jobs, double ratio, int32_t mono_calls, void *stream) {
  REQUIRE(e, "asx_resample_sinc_batch_dev: null engine");
  HIPCHK(hipSetDevice(e->device));
  return resample_sinc_batch_dev(e, jobs, n_jobs, ratio, mono_calls, reinterpret_cast<hipStream_t>(stream));
}

// The rational polyphase converter (resample_plan.h, kernels_resample.h): the plan of a pair of rates, pure host
int asx_resample_rational_plan(int32_t sr_in, int32_t sr_out, int64_t n_in, int64_t *n_out, int32_t *L, int32_t *M, int32_t *taps_per_phase) {
  ResamplePlan p;
  const std::string why = resample_plan_make(sr_in, sr_out, p);
  REQUIRE(why.empty(), "asx_resample_rational_plan: %s", why.c_str());
  if (n_out) {
    const std::string bad = resample_plan_check_n(p, n_in);
    REQUIRE(bad.empty(), "asx_resample_rational_plan: %s", bad.c_str());
    *n_out = resample_plan_n_out(p, n_in);
  }
  if (L) *L = (int32_t)p.L;
  if (M) *M = (int32_t)p.M;
  if (taps_per_phase) *taps_per_phase = (int32_t)p.T;
  return ASX_OK;
}

int asx_resample_rational_dev(asx_engine *e, const float *x_dev, int32_t channels, int64_t n_in, int32_t sr_in, int32_t sr_out, float *y_dev,
                              int64_t n_out, void *stream) {
  REQUIRE(e && x_dev && y_dev, "asx_resample_rational_dev: null argument");
  REQUIRE(channels >= 1 && channels <= 65535, "asx_resample_rational_dev: %d channels (1 .. 65535)", channels);
  ResamplePlan p;
  const std::string why = resample_plan_make(sr_in, sr_out, p);
  REQUIRE(why.empty(), "asx_resample_rational_dev: %s", why.c_str());
  const std::string bad = resample_plan_check_n(p, n_in);
  REQUIRE(bad.empty(), "asx_resample_rational_dev: %s", bad.c_str());
  REQUIRE(n_out == resample_plan_n_out(p, n_in), "asx_resample_rational_dev: n_out = %lld, but %lld samples at %d Hz are %lld at %d Hz",
          (long long)n_out, (long long)n_in, sr_in, (long long)resample_plan_n_out(p, n_in), sr_out);
  REQUIRE(p.K == 8 || !p.taps_in_lds, "asx_resample_rational_dev: no kernel for the tile of %d -> %d Hz", sr_in, sr_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const RsTable *t = nullptr;
  CHK(rs_table(e, p, &t));
  const float *tab = t->tab.f();
  return timed(e, ASX_PROF_MISC, 2.0 * channels * (double)n_out * (double)p.T, 4.0 * channels * ((double)n_in + (double)n_out), s, [&]() {
    if (p.taps_in_lds) rs_launch<8, true>(p, x_dev, channels, n_in, tab, y_dev, n_out, s);
    else if (p.K == 8) rs_launch<8, false>(p, x_dev, channels, n_in, tab, y_dev, n_out, s);
    else if (p.K == 4) rs_launch<4, false>(p, x_dev, channels, n_in, tab, y_dev, n_out, s);
    else if (p.K == 2) rs_launch<2, false>(p, x_dev, channels, n_in, tab, y_dev, n_out, s);
    else rs_launch<1, false>(p, x_dev, channels, n_in, tab, y_dev, n_out, s);
  });
}

int asx_resample_rational(asx_engine *e, const float *x_host, int32_t channels, int64_t n_in, int32_t sr_in, int32_t sr_out, float *y_host,
                          int64_t n_out) {
  REQUIRE(e && x_host && y_host, "asx_resample_rational: null argument");
  REQUIRE(channels >= 1 && channels <= 65535 && n_in >= 1 && n_out >= 1, "asx_resample_rational: bad argument");
  HIPCHK(hipSetDevice(e->device));
  return host_round_trip(x_host, (size_t)channels * n_in, y_host, (size_t)channels * n_out, [&](const float *x, float *y) {
    return asx_resample_rational_dev(e, x, channels, n_in, sr_in, sr_out, y, n_out, nullptr);
  });
}

// The writer-side form of the converter: planar or rows input, the caller's n_out (include/asx.h)
int asx_resample_rational_stem_dev(asx_engine *e, const float *x_dev, int32_t layout, int32_t channels, int64_t n_in, int32_t sr_in, int32_t sr_out,
                                   float *y_dev, int64_t n_out, void *stream) {
  REQUIRE(e, "asx_resample_rational_stem_dev: null engine");
  REQUIRE(x_dev, "asx_resample_rational_stem_dev: x is null");
  REQUIRE(y_dev, "asx_resample_rational_stem_dev: y is null");
  REQUIRE(layout == 0 || layout == 1, "asx_resample_rational_stem_dev: layout = %d (0: planar [channels, n_in], 1: rows [n_in, channels])", layout);
  REQUIRE(channels >= 1 && channels <= 65535, "asx_resample_rational_stem_dev: %d channels (1 .. 65535)", channels);
  ResamplePlan p;
  const std::string why = resample_plan_make(sr_in, sr_out, p);
  REQUIRE(why.empty(), "asx_resample_rational_stem_dev: %s", why.c_str());
  const std::string bad = resample_plan_check_stem(p, n_in, n_out);
  REQUIRE(bad.empty(), "asx_resample_rational_stem_dev: %s", bad.c_str());
  REQUIRE(p.K == 8 || !p.taps_in_lds, "asx_resample_rational_stem_dev: no kernel for the tile of %d -> %d Hz", sr_in, sr_out);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const RsTable *t = nullptr;
  CHK(rs_table(e, p, &t));
  const float *tab = t->tab.f();
  const bool rows = layout == 1;
  return timed(e, ASX_PROF_MISC, 2.0 * channels * (double)n_out * (double)p.T, 4.0 * channels * ((double)n_in + (double)n_out), s, [&]() {
    if (p.taps_in_lds) rs_stem_launch<8, true>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, s);
    else if (p.K == 8) rs_stem_launch<8, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, s);
    else if (p.K == 4) rs_stem_launch<4, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, s);
    else if (p.K == 2) rs_stem_launch<2, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, s);
    else rs_stem_launch<1, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, s);
  });
}

int asx_resample_rational_stem(asx_engine *e, const float *x_host, int32_t layout, int32_t channels, int64_t n_in, int32_t sr_in, int32_t sr_out,
                               float *y_host, int64_t n_out) {
  REQUIRE(e, "asx_resample_rational_stem: null engine");
  REQUIRE(x_host, "asx_resample_rational_stem: x is null");
  REQUIRE(y_host, "asx_resample_rational_stem: y is null");
  // (checked here as well: the sizes of the staging buffers follow from them)
  REQUIRE(layout == 0 || layout == 1, "asx_resample_rational_stem: layout = %d (0: planar [channels, n_in], 1: rows [n_in, channels])", layout);
  REQUIRE(channels >= 1 && channels <= 65535, "asx_resample_rational_stem: %d channels (1 .. 65535)", channels);
  ResamplePlan p;
  const std::string why = resample_plan_make(sr_in, sr_out, p);
  REQUIRE(why.empty(), "asx_resample_rational_stem: %s", why.c_str());
  const std::string bad = resample_plan_check_stem(p, n_in, n_out);
  REQUIRE(bad.empty(), "asx_resample_rational_stem: %s", bad.c_str());
  HIPCHK(hipSetDevice(e->device));
  return host_round_trip(x_host, (size_t)channels * n_in, y_host, (size_t)channels * n_out, [&](const float *x, float *y) {
    return asx_resample_rational_stem_dev(e, x, layout, channels, n_in, sr_in, sr_out, y, n_out, nullptr);
  });
}

// The complement form of the writer-side converter: y (optional) and c = fl(fl(mix_scale mix) - fl(stem_scale y)) in one launch (include/asx.h)
static int rs_complement_check(const char *fn, asx_engine *e, const float *x, int32_t layout, int32_t channels, int64_t n_in, int32_t sr_in,
                               int32_t sr_out, const float *mix, int64_t mix_stride, float mix_scale, float stem_scale, float *c, int64_t n_out,
                               ResamplePlan &p) {
  REQUIRE(e, "%s: null engine", fn);
  REQUIRE(x, "%s: x is null", fn);
  REQUIRE(mix, "%s: mix is null", fn);
  REQUIRE(c, "%s: c is null", fn);
  REQUIRE(layout == 0 || layout == 1, "%s: layout = %d (0: planar [channels, n_in], 1: rows [n_in, channels])", fn, layout);
  REQUIRE(channels >= 1 && channels <= 65535, "%s: %d channels (1 .. 65535)", fn, channels);
  const std::string why = resample_plan_make(sr_in, sr_out, p);
  REQUIRE(why.empty(), "%s: %s", fn, why.c_str());
  const std::string bad = resample_plan_check_stem(p, n_in, n_out);
  REQUIRE(bad.empty(), "%s: %s", fn, bad.c_str());
  REQUIRE(mix_stride >= n_out && mix_stride <= ((int64_t)1 << 40), "%s: mix_stride = %lld (n_out = %lld .. 2^40)", fn, (long long)mix_stride,
          (long long)n_out);
  REQUIRE(std::isfinite(mix_scale), "%s: mix_scale is not finite", fn);
  REQUIRE(std::isfinite(stem_scale), "%s: stem_scale is not finite", fn);
  REQUIRE(p.K == 8 || !p.taps_in_lds, "%s: no kernel for the tile of %d -> %d Hz", fn, sr_in, sr_out);
  return ASX_OK;
}

int asx_resample_rational_complement_dev(asx_engine *e, const float *x_dev, int32_t layout, int32_t channels, int64_t n_in, int32_t sr_in,
                                         int32_t sr_out, const float *mix_dev, int64_t mix_stride, float mix_scale, float stem_scale,
                                         float *y_dev, float *c_dev, int64_t n_out, void *stream) {
  ResamplePlan p;
  CHK(rs_complement_check("asx_resample_rational_complement_dev", e, x_dev, layout, channels, n_in, sr_in, sr_out, mix_dev, mix_stride, mix_scale,
                          stem_scale, c_dev, n_out, p));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const RsTable *t = nullptr;
  CHK(rs_table(e, p, &t));
  const float *tab = t->tab.f();
  const bool rows = layout == 1;
  const double bytes = 4.0 * channels * ((double)n_in + (double)n_out * (y_dev ? 3.0 : 2.0));
  return timed(e, ASX_PROF_MISC, 2.0 * channels * (double)n_out * (double)p.T, bytes, s, [&]() {
    if (p.taps_in_lds)
      rs_complement_launch<8, true>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, mix_dev, mix_stride, mix_scale, stem_scale, c_dev, s);
    else if (p.K == 8)
      rs_complement_launch<8, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, mix_dev, mix_stride, mix_scale, stem_scale, c_dev, s);
    else if (p.K == 4)
      rs_complement_launch<4, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, mix_dev, mix_stride, mix_scale, stem_scale, c_dev, s);
    else if (p.K == 2)
      rs_complement_launch<2, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, mix_dev, mix_stride, mix_scale, stem_scale, c_dev, s);
    else
      rs_complement_launch<1, false>(p, x_dev, rows, channels, n_in, tab, y_dev, n_out, mix_dev, mix_stride, mix_scale, stem_scale, c_dev, s);
  });
}

int asx_resample_rational_complement(asx_engine *e, const float *x_host, int32_t layout, int32_t channels, int64_t n_in, int32_t sr_in,
                                     int32_t sr_out, const float *mix_host, int64_t mix_stride, float mix_scale, float stem_scale,
                                     float *y_host, float *c_host, int64_t n_out) {
  // (checked here as well: the sizes of the staging buffers follow from the arguments)
  ResamplePlan p;
  CHK(rs_complement_check("asx_resample_rational_complement", e, x_host, layout, channels, n_in, sr_in, sr_out, mix_host, mix_stride, mix_scale,
                          stem_scale, c_host, n_out, p));
  HIPCHK(hipSetDevice(e->device));
  DevBuf dx, dmix, dy, dc;
  BufGuard g{{&dx, &dmix, &dy, &dc}};
  CHK(to_dev(dx, x_host, (size_t)channels * n_in));
  CHK(to_dev(dmix, mix_host, (size_t)channels * mix_stride));
  if (y_host) CHK(dy.ensure((size_t)channels * n_out * 4));
  CHK(dc.ensure((size_t)channels * n_out * 4));
  CHK(asx_resample_rational_complement_dev(e, dx.f(), layout, channels, n_in, sr_in, sr_out, dmix.f(), mix_stride, mix_scale, stem_scale,
                                           y_host ? dy.f() : nullptr, dc.f(), n_out, nullptr));
  if (y_host) CHK(to_host(y_host, dy, (size_t)channels * n_out));
  return to_host(c_host, dc, (size_t)channels * n_out);
}

// the factor asx_normalize_dev would multiply wave_dev by (1 where it leaves the array alone): the peak word comes to the host, nothing else
int asx_normalize_scale_dev(asx_engine *e, const float *wave_dev, int64_t numel, float max_peak, float min_peak, int32_t has_min, float *scale,
                            void *stream) {
  REQUIRE(e, "asx_normalize_scale_dev: null engine");
  REQUIRE(wave_dev, "asx_normalize_scale_dev: wave is null");
  REQUIRE(scale, "asx_normalize_scale_dev: scale is null");
  REQUIRE(numel >= 1, "asx_normalize_scale_dev: numel = %lld (>= 1)", (long long)numel);
  REQUIRE(std::isfinite(max_peak) && (!has_min || std::isfinite(min_peak)), "asx_normalize_scale_dev: a threshold is not finite");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p) + 5;   // its own word (0 .. 4: see asx_normalize_dev and the decoders)
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const unsigned nb = (unsigned)std::min<int64_t>((numel + 255) / 256, 2048);
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * numel, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, wave_dev, numel, pk); }));
  float maxv = 0.f;
  HIPCHK(hipMemcpyAsync(&maxv, pk, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  // normalize_kernel's branches; a float32 division on the host rounds as __fdiv_rn does (the operands and the result are floats)
  float q = 1.f;
  if (maxv > max_peak) q = max_peak / maxv;
  else if (has_min && maxv < min_peak) q = min_peak / maxv;
  // a silent array under a minimum peak: the normalise would multiply by infinity.  Said here, not by whoever is handed the factor
  REQUIRE(std::isfinite(q), "asx_normalize_scale_dev: wave is silent (peak %g): min_peak / peak is not finite", (double)maxv);
  *scale = q;
  return ASX_OK;
}

// The FLAC encoder (kernels_flac.h, engine_flac.h): the plan of a stream, pure host
int asx_flac_plan(int64_t n_samples, int32_t channels, int32_t bits_per_sample, int32_t block_size, int64_t *n_blocks, int32_t *frame_stride,
                  int64_t *max_bytes, int64_t *scratch_bytes) {
  FlacPlan p;
  const std::string why = flac_plan_make(n_samples, channels, bits_per_sample, block_size, p);
  REQUIRE(why.empty(), "asx_flac_plan: %s", why.c_str());
  if (n_blocks) *n_blocks = p.n_blocks;
  if (frame_stride) *frame_stride = p.stride;
  if (max_bytes) *max_bytes = p.max_bytes;
  if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
  return ASX_OK;
}

int asx_flac_encode_dev(asx_engine *e, const int16_t *pcm16_dev, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample, int32_t block_size,
                        uint8_t *out_dev, int64_t out_capacity, int32_t *frame_bytes_dev, int64_t *total_bytes, void *stream) {
  REQUIRE(e && pcm16_dev && out_dev && frame_bytes_dev && total_bytes, "asx_flac_encode_dev: null argument");
  FlacPlan p;
  const std::string why = flac_plan_make(n_samples, 2, bits_per_sample, block_size, p);
  REQUIRE(why.empty(), "asx_flac_encode_dev: %s", why.c_str());
  REQUIRE(sample_rate >= 1 && sample_rate <= 1048575, "asx_flac_encode_dev: sample rate %d Hz (1 .. 1048575)", sample_rate);
  REQUIRE(out_capacity >= p.max_bytes, "asx_flac_encode_dev: out_capacity %lld below the plan's worst case of %lld bytes", (long long)out_capacity,
          (long long)p.max_bytes);
  REQUIRE((((uintptr_t)pcm16_dev) & 3) == 0 && (((uintptr_t)frame_bytes_dev) & 3) == 0, "asx_flac_encode_dev: pcm16 and frame_bytes must be 4-byte aligned");
  HIPCHK(hipSetDevice(e->device));
  return flac_encode_launch<false>(e, pcm16_dev, n_samples, sample_rate, bits_per_sample, block_size, p, out_dev, frame_bytes_dev, total_bytes,
                                   reinterpret_cast<hipStream_t>(stream));
}

int asx_flac_encode(asx_engine *e, const int16_t *pcm16_host, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample, int32_t block_size,
                    uint8_t *out_host, int64_t out_capacity, int32_t *frame_bytes_host, int64_t *total_bytes) {
  REQUIRE(e && pcm16_host && out_host && frame_bytes_host && total_bytes, "asx_flac_encode: null argument");
  FlacPlan p;
  const std::string why = flac_plan_make(n_samples, 2, bits_per_sample, block_size, p);
  REQUIRE(why.empty(), "asx_flac_encode: %s", why.c_str());
  REQUIRE(out_capacity >= p.max_bytes, "asx_flac_encode: out_capacity %lld below the plan's worst case of %lld bytes", (long long)out_capacity,
          (long long)p.max_bytes);
  HIPCHK(hipSetDevice(e->device));
  DevBuf din, dout, dsz;
  BufGuard g{{&din, &dout, &dsz}};
  CHK(din.ensure((size_t)n_samples * 4));
  CHK(dout.ensure((size_t)p.max_bytes));
  CHK(dsz.ensure((size_t)p.n_blocks * 4));
  HIPCHK(hipMemcpy(din.p, pcm16_host, (size_t)n_samples * 4, hipMemcpyHostToDevice));
  CHK(asx_flac_encode_dev(e, reinterpret_cast<const int16_t *>(din.p), n_samples, sample_rate, bits_per_sample, block_size,
                          reinterpret_cast<uint8_t *>(dout.p), p.max_bytes, reinterpret_cast<int32_t *>(dsz.p), total_bytes, nullptr));
  HIPCHK(hipMemcpy(out_host, dout.p, (size_t)*total_bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(frame_bytes_host, dsz.p, (size_t)p.n_blocks * 4, hipMemcpyDeviceToHost));
  return ASX_OK;
}

// The same encoder for int32 [n, 2] samples of 16 or 24 real bits (flac_encode_kernel<true>): no wasted bits, the side channel at bps + 1
int asx_flac_plan_pcm(int64_t n_samples, int32_t channels, int32_t bits_per_sample, int32_t block_size, int64_t *n_blocks, int32_t *frame_stride,
                      int64_t *max_bytes, int64_t *scratch_bytes) {
  FlacPlan p;
  const std::string why = flac_plan_make(n_samples, channels, bits_per_sample, block_size, p, true);
  REQUIRE(why.empty(), "asx_flac_plan_pcm: %s", why.c_str());
  if (n_blocks) *n_blocks = p.n_blocks;
  if (frame_stride) *frame_stride = p.stride;
  if (max_bytes) *max_bytes = p.max_bytes;
  if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
  return ASX_OK;
}

int asx_flac_encode_pcm_dev(asx_engine *e, const int32_t *pcm_dev, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample,
                            int32_t block_size, uint8_t *out_dev, int64_t out_capacity, int32_t *frame_bytes_dev, int64_t *total_bytes,
                            void *stream) {
  FlacPlan p;
  const std::string why = flac_plan_make(n_samples, 2, bits_per_sample, block_size, p, true);
  REQUIRE(why.empty(), "asx_flac_encode_pcm_dev: %s", why.c_str());
  REQUIRE(sample_rate >= 1 && sample_rate <= 1048575, "asx_flac_encode_pcm_dev: sample rate %d Hz (1 .. 1048575)", sample_rate);
  REQUIRE(e && pcm_dev && out_dev && frame_bytes_dev && total_bytes, "asx_flac_encode_pcm_dev: null argument");
  REQUIRE(out_capacity >= p.max_bytes, "asx_flac_encode_pcm_dev: out_capacity %lld below the plan's worst case of %lld bytes",
          (long long)out_capacity, (long long)p.max_bytes);
  REQUIRE((((uintptr_t)pcm_dev) & 3) == 0 && (((uintptr_t)frame_bytes_dev) & 3) == 0, "asx_flac_encode_pcm_dev: pcm and frame_bytes must be 4-byte aligned");
  HIPCHK(hipSetDevice(e->device));
  return flac_encode_launch<true>(e, pcm_dev, n_samples, sample_rate, bits_per_sample, block_size, p, out_dev, frame_bytes_dev, total_bytes,
                                  reinterpret_cast<hipStream_t>(stream));
}

int asx_flac_encode_pcm(asx_engine *e, const int32_t *pcm_host, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample, int32_t block_size,
                        uint8_t *out_host, int64_t out_capacity, int32_t *frame_bytes_host, int64_t *total_bytes) {
  FlacPlan p;
  const std::string why = flac_plan_make(n_samples, 2, bits_per_sample, block_size, p, true);
  REQUIRE(why.empty(), "asx_flac_encode_pcm: %s", why.c_str());
  REQUIRE(sample_rate >= 1 && sample_rate <= 1048575, "asx_flac_encode_pcm: sample rate %d Hz (1 .. 1048575)", sample_rate);
  REQUIRE(e && pcm_host && out_host && frame_bytes_host && total_bytes, "asx_flac_encode_pcm: null argument");
  REQUIRE(out_capacity >= p.max_bytes, "asx_flac_encode_pcm: out_capacity %lld below the plan's worst case of %lld bytes", (long long)out_capacity,
          (long long)p.max_bytes);
  const int32_t lo = -(1 << (bits_per_sample - 1)), hi = (1 << (bits_per_sample - 1)) - 1;
  for (int64_t i = 0; i < 2 * n_samples; ++i)
    REQUIRE(pcm_host[i] >= lo && pcm_host[i] <= hi, "asx_flac_encode_pcm: sample %lld = %d is outside %d bits", (long long)i, pcm_host[i],
            bits_per_sample);
  HIPCHK(hipSetDevice(e->device));
  DevBuf din, dout, dsz;
  BufGuard g{{&din, &dout, &dsz}};
  CHK(din.ensure((size_t)n_samples * 8));
  CHK(dout.ensure((size_t)p.max_bytes));
  CHK(dsz.ensure((size_t)p.n_blocks * 4));
  HIPCHK(hipMemcpy(din.p, pcm_host, (size_t)n_samples * 8, hipMemcpyHostToDevice));
  CHK(asx_flac_encode_pcm_dev(e, reinterpret_cast<const int32_t *>(din.p), n_samples, sample_rate, bits_per_sample, block_size,
                              reinterpret_cast<uint8_t *>(dout.p), p.max_bytes, reinterpret_cast<int32_t *>(dsz.p), total_bytes, nullptr));
  HIPCHK(hipMemcpy(out_host, dout.p, (size_t)*total_bytes, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(frame_bytes_host, dsz.p, (size_t)p.n_blocks * 4, hipMemcpyDeviceToHost));
  return ASX_OK;
}

// The FLAC decoder (kernels_flac_dec.h, flac_dec_plan.h, engine_flac_dec.h): which streams it takes, pure host
int asx_flac_decode_plan(int64_t audio_bytes, int32_t channels, int32_t bits_per_sample, int32_t max_blocksize, int32_t max_framesize,
                         int64_t *max_candidates, int64_t *slot_bytes, int64_t *scratch_bytes) {
  FlacDecPlan p;
  const std::string why = flac_dec_plan_make(audio_bytes, channels, bits_per_sample, max_blocksize, max_framesize, p);
  REQUIRE(why.empty(), "asx_flac_decode_plan: %s", why.c_str());
  if (max_candidates) *max_candidates = p.max_candidates;
  if (slot_bytes) *slot_bytes = p.slot_bytes;
  if (scratch_bytes) *scratch_bytes = p.scratch_bytes;
  return ASX_OK;
}

int asx_flac_decode_scan_dev(asx_engine *e, const uint8_t *audio_dev, int64_t audio_bytes, int32_t sample_rate, int32_t channels,
                             int32_t bits_per_sample, int32_t max_blocksize, int32_t max_framesize, int64_t *n_samples, int64_t *n_frames,
                             int64_t *bytes_consumed, void *stream) {
  REQUIRE(e && audio_dev && n_samples, "asx_flac_decode_scan_dev: null argument");
  FlacDecPlan p;
  const std::string why = flac_dec_plan_make(audio_bytes, channels, bits_per_sample, max_blocksize, max_framesize, p);
  REQUIRE(why.empty(), "asx_flac_decode_scan_dev: %s", why.c_str());
  REQUIRE(sample_rate >= 1 && sample_rate <= 1048575, "asx_flac_decode_scan_dev: sample rate %d Hz (1 .. 1048575)", sample_rate);
  REQUIRE((((uintptr_t)audio_dev) & 3) == 0, "asx_flac_decode_scan_dev: the audio bytes must be 4-byte aligned");
  HIPCHK(hipSetDevice(e->device));
  const flacdec::Info I{sample_rate, channels, bits_per_sample, max_blocksize, max_framesize};
  return flac_decode_scan_launch(e, audio_dev, audio_bytes, I, p, n_samples, n_frames, bytes_consumed, reinterpret_cast<hipStream_t>(stream));
}

int asx_flac_decode_finish_dev(asx_engine *e, float *mix_dev, int64_t n_samples, float *peak, void *stream) {
  REQUIRE(e && mix_dev, "asx_flac_decode_finish_dev: null argument");
  REQUIRE(e->flacdec_n_samples >= 0, "asx_flac_decode_finish_dev: no asx_flac_decode_scan_dev on this engine before it");
  REQUIRE(n_samples >= 1 && n_samples == e->flacdec_n_samples, "asx_flac_decode_finish_dev: n_samples = %lld, the scan found %lld", (long long)n_samples,
          (long long)e->flacdec_n_samples);
  REQUIRE((((uintptr_t)mix_dev) & 3) == 0, "asx_flac_decode_finish_dev: mix must be 4-byte aligned");
  HIPCHK(hipSetDevice(e->device));
  return flac_decode_finish_launch(e, mix_dev, n_samples, peak, reinterpret_cast<hipStream_t>(stream));
}

int asx_flac_decode(asx_engine *e, const uint8_t *audio_host, int64_t audio_bytes, int32_t sample_rate, int32_t channels, int32_t bits_per_sample,
                    int32_t max_blocksize, int32_t max_framesize, float *mix_host, int64_t capacity, int64_t *n_samples, int64_t *n_frames,
                    int64_t *bytes_consumed, float *peak) {
  REQUIRE(e && audio_host && n_samples && (mix_host || capacity == 0) && capacity >= 0, "asx_flac_decode: null argument");
  FlacDecPlan p;
  const std::string why = flac_dec_plan_make(audio_bytes, channels, bits_per_sample, max_blocksize, max_framesize, p);
  REQUIRE(why.empty(), "asx_flac_decode: %s", why.c_str());
  HIPCHK(hipSetDevice(e->device));
  DevBuf din, dmix;
  BufGuard g{{&din, &dmix}};
  CHK(din.ensure(((size_t)audio_bytes + 3) / 4 * 4));
  HIPCHK(hipMemcpy(din.p, audio_host, (size_t)audio_bytes, hipMemcpyHostToDevice));
  CHK(asx_flac_decode_scan_dev(e, reinterpret_cast<const uint8_t *>(din.p), audio_bytes, sample_rate, channels, bits_per_sample, max_blocksize,
                               max_framesize, n_samples, n_frames, bytes_consumed, nullptr));
  if (peak) *peak = 0.f;
  if (*n_samples == 0) return ASX_OK;
  REQUIRE(capacity >= *n_samples, "asx_flac_decode: capacity of %lld samples per row, the stream holds %lld", (long long)capacity, (long long)*n_samples);
  CHK(dmix.ensure((size_t)2 * (size_t)*n_samples * 4));
  CHK(asx_flac_decode_finish_dev(e, dmix.f(), *n_samples, peak, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(mix_host, dmix.p, (size_t)2 * (size_t)*n_samples * 4, hipMemcpyDeviceToHost));
  return ASX_OK;
}

// ---- stage hooks -------------------------------------------------------------
static int transpose_launch(const float *in, float *out, int planes, int rows, int cols, hipStream_t s) {
  hipLaunchKernelGGL(transpose_last2_kernel, dim3((cols + 31) / 32, (rows + 31) / 32, planes), dim3(32, 8), 0, s, in,
                     out, rows, cols);
  HIPCHK(hipGetLastError());
  return ASX_OK;
}

// write_audio_pydub's array work (common_separator.py:309-337): stem [2, N] planar float32 -> normalised int16 [N, 2];
// *peak_after = max |stem| after normalisation (the caller skips near-silent stems: < 1e-6, :312-315)
int asx_pcm16_dev(asx_engine *e, const float *stem_dev, int64_t N, float max_peak, float min_peak, int32_t has_min, int16_t *pcm_dev,
                  float *peak_after, void *stream) {
  REQUIRE(e && stem_dev && pcm_dev && N >= 1, "asx_pcm16_dev: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p);
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const int64_t n2 = 2 * N;
  const unsigned nb = (unsigned)std::min<int64_t>((n2 + 255) / 256, 2048);
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * n2, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, stem_dev, n2, pk); }));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 6.0 * n2, s, [&]() {
    hipLaunchKernelGGL(pcm16_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, stem_dev, N, pk, max_peak, min_peak, has_min,
                       reinterpret_cast<short *>(pcm_dev));
  }));
  if (peak_after) {
    float maxv = 0.f;
    HIPCHK(hipMemcpyAsync(&maxv, pk, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float scale = 1.0f;
    if (maxv > max_peak) scale = max_peak / maxv;
    else if (has_min && maxv < min_peak) scale = min_peak / maxv;
    *peak_after = maxv * scale;
  }
  return ASX_OK;
}

int asx_pcm16_rows_dev(asx_engine *e, const float *stem_rows_dev, int64_t N, float max_peak, float min_peak, int32_t has_min,
                       int16_t *pcm_dev, float *peak_after, void *stream) {
  REQUIRE(e && stem_rows_dev && pcm_dev && N >= 1, "asx_pcm16_rows_dev: bad argument");
  REQUIRE((((uintptr_t)stem_rows_dev) & 15) == 0 && (((uintptr_t)pcm_dev) & 7) == 0, "asx_pcm16_rows_dev: stem must be 16-byte and pcm 8-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p);
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const int64_t n2 = 2 * N;
  const unsigned nb = (unsigned)std::min<int64_t>((n2 + 255) / 256, 2048);
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * n2, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, stem_rows_dev, n2, pk); }));
  CHK(timed(e, ASX_PROF_MISC, 0.0, 6.0 * n2, s, [&]() {
    hipLaunchKernelGGL(pcm16_rows_kernel, dim3((unsigned)((n2 / 4 + 256) / 256)), dim3(256), 0, s, stem_rows_dev, n2, pk, max_peak, min_peak,
                       has_min, reinterpret_cast<short *>(pcm_dev));
  }));
  if (peak_after) {
    float maxv = 0.f;
    HIPCHK(hipMemcpyAsync(&maxv, pk, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float scale = 1.0f;
    if (maxv > max_peak) scale = max_peak / maxv;
    else if (has_min && maxv < min_peak) scale = min_peak / maxv;
    *peak_after = maxv * scale;
  }
  return ASX_OK;
}

// write_audio_soundfile's array work for a stem in HBM (kernels_pcm_encode.h): normalise, then the samples in the file's own format,
// interleaved [n, 2]; *peak_after = max |stem| after normalisation.  stem_dev is only read.
int asx_pcm_encode_dev(asx_engine *e, const float *stem_dev, int64_t n_samples, int32_t layout, float max_peak, float min_peak, int32_t has_min,
                       int32_t sample_format, void *out_dev, float *peak_after, void *stream) {
  // every argument is judged before anything is enqueued, the engine last (so that the refusals can be told apart without a device)
  REQUIRE(stem_dev && out_dev, "asx_pcm_encode_dev: null stem or output");
  REQUIRE(n_samples >= 1 && n_samples <= ((int64_t)1 << 40), "asx_pcm_encode_dev: n_samples = %lld (1 .. 2^40)", (long long)n_samples);
  REQUIRE(layout == ASX_STEM_PLANAR || layout == ASX_STEM_ROWS, "asx_pcm_encode_dev: layout %d (0 planar [2, n], 1 rows [n, 2])", (int)layout);
  REQUIRE(pcmenc_known(sample_format),
          "asx_pcm_encode_dev: sample format %d (16, 24, 32 = integer PCM bits, 0x120 = IEEE float32, 0x410 / 0x418 = 16 / 24 bits in int32)",
          (int)sample_format);
  REQUIRE((((uintptr_t)stem_dev) & 3) == 0 && (((uintptr_t)out_dev) & 15) == 0, "asx_pcm_encode_dev: stem must be 4-byte and the output 16-byte aligned");
  REQUIRE(e, "asx_pcm_encode_dev: null engine");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p) + 4;   // its own word (0: separate / pcm16, 1: decode, 2: normalize_dev, 3: ensemble slot)
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const int64_t n2 = 2 * n_samples;
  const unsigned nb = (unsigned)std::min<int64_t>((n2 + 255) / 256, 2048);
  unsigned char *out = reinterpret_cast<unsigned char *>(out_dev);
  const int rows = layout == ASX_STEM_ROWS;
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * n2, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, stem_dev, n2, pk); }));
  CHK(timed(e, ASX_PROF_MISC, 0.0, (8.0 + pcmenc_frame_bytes(sample_format)) * n_samples, s, [&]() {
    switch (sample_format) {
      case PCMENC_S16: pcm_encode_launch<PCMENC_S16>(stem_dev, n_samples, rows, pk, max_peak, min_peak, has_min, out, s); break;
      case PCMENC_S24: pcm_encode_launch<PCMENC_S24>(stem_dev, n_samples, rows, pk, max_peak, min_peak, has_min, out, s); break;
      case PCMENC_S32: pcm_encode_launch<PCMENC_S32>(stem_dev, n_samples, rows, pk, max_peak, min_peak, has_min, out, s); break;
      case PCMENC_F32: pcm_encode_launch<PCMENC_F32>(stem_dev, n_samples, rows, pk, max_peak, min_peak, has_min, out, s); break;
      case PCMENC_S16_IN_32: pcm_encode_launch<PCMENC_S16_IN_32>(stem_dev, n_samples, rows, pk, max_peak, min_peak, has_min, out, s); break;
      default: pcm_encode_launch<PCMENC_S24_IN_32>(stem_dev, n_samples, rows, pk, max_peak, min_peak, has_min, out, s); break;
    }
  }));
  if (peak_after) {
    float maxv = 0.f;
    HIPCHK(hipMemcpyAsync(&maxv, pk, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float scale = 1.0f;
    if (maxv > max_peak) scale = max_peak / maxv;
    else if (has_min && maxv < min_peak) scale = min_peak / maxv;
    *peak_after = maxv * scale;
  }
  return ASX_OK;
}

int asx_pcm_encode(asx_engine *e, const float *stem_host, int64_t n_samples, int32_t layout, float max_peak, float min_peak, int32_t has_min,
                   int32_t sample_format, void *out_host, float *peak_after) {
  REQUIRE(stem_host && out_host, "asx_pcm_encode: null stem or output");
  REQUIRE(n_samples >= 1 && n_samples <= ((int64_t)1 << 40), "asx_pcm_encode: n_samples = %lld (1 .. 2^40)", (long long)n_samples);
  REQUIRE(layout == ASX_STEM_PLANAR || layout == ASX_STEM_ROWS, "asx_pcm_encode: layout %d (0 planar [2, n], 1 rows [n, 2])", (int)layout);
  REQUIRE(pcmenc_known(sample_format),
          "asx_pcm_encode: sample format %d (16, 24, 32 = integer PCM bits, 0x120 = IEEE float32, 0x410 / 0x418 = 16 / 24 bits in int32)",
          (int)sample_format);
  REQUIRE(e, "asx_pcm_encode: null engine");
  HIPCHK(hipSetDevice(e->device));
  DevBuf ds, dp;
  BufGuard g{{&ds, &dp}};
  const size_t bytes = (size_t)n_samples * (size_t)pcmenc_frame_bytes(sample_format);
  CHK(to_dev(ds, stem_host, (size_t)2 * n_samples));
  CHK(dp.ensure(bytes));
  CHK(asx_pcm_encode_dev(e, ds.f(), n_samples, layout, max_peak, min_peak, has_min, sample_format, dp.p, peak_after, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_host, dp.p, bytes, hipMemcpyDeviceToHost));
  return ASX_OK;
}

int asx_pcm_decode_dev(asx_engine *e, const void *raw_dev, int64_t frames, int32_t channels, int32_t sample_format, float *mix_dev,
                       float *peak, void *stream) {
  REQUIRE(e && raw_dev && mix_dev && frames >= 1, "asx_pcm_decode_dev: bad argument");
  REQUIRE(channels >= 1 && channels <= 64, "asx_pcm_decode_dev: %d channels", channels);
  REQUIRE(sample_format == 16 || sample_format == 24 || sample_format == 32 || sample_format == 0x120,
          "asx_pcm_decode_dev: sample format %d (16, 24, 32 = integer PCM bits, 0x120 = IEEE float32)", sample_format);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p) + 1;   // its own word: asx_separate_dev uses word 0
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const unsigned nb = (unsigned)std::min<int64_t>((frames + 255) / 256, 4096);
  CHK(timed(e, ASX_PROF_MISC, 0.0, (double)frames * (channels * (sample_format & 0xff) / 8 + 8.0), s, [&]() {
    hipLaunchKernelGGL(pcm_decode_kernel, dim3(nb), dim3(256), 0, s, reinterpret_cast<const unsigned char *>(raw_dev), frames, (int)channels,
                       (int)sample_format, mix_dev, pk);
  }));
  if (peak) {
    HIPCHK(hipMemcpyAsync(peak, pk, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  return ASX_OK;
}

int asx_pcm16(asx_engine *e, const float *stem_host, int64_t N, float max_peak, float min_peak, int32_t has_min, int16_t *pcm_host,
              float *peak_after) {
  REQUIRE(e && stem_host && pcm_host && N >= 1, "asx_pcm16: bad argument");
  HIPCHK(hipSetDevice(e->device));
  DevBuf ds, dp;
  BufGuard g{{&ds, &dp}};
  CHK(to_dev(ds, stem_host, (size_t)2 * N));
  CHK(dp.ensure((size_t)2 * N * 2));
  CHK(asx_pcm16_dev(e, ds.f(), N, max_peak, min_peak, has_min, reinterpret_cast<int16_t *>(dp.p), peak_after, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(pcm_host, dp.p, (size_t)2 * N * 2, hipMemcpyDeviceToHost));
  return ASX_OK;
}

int asx_resample_sinc(asx_engine *e, const float *x_host, int32_t channels, int64_t n_in, double ratio, int32_t mono_calls,
                      float *y_host, int64_t n_out) {
  REQUIRE(e && x_host && y_host && channels >= 1 && n_in >= 1 && n_out >= 1, "asx_resample_sinc: bad argument");
  HIPCHK(hipSetDevice(e->device));
  return host_round_trip(x_host, (size_t)channels * n_in, y_host, (size_t)channels * n_out, [&](const float *x, float *y) {
    return asx_resample_sinc_dev(e, x, channels, n_in, ratio, mono_calls, y, n_out, nullptr);
  });
}

int asx_stft(asx_engine *e, const float *wave_host, int32_t B, int64_t C, float *spec_host) {
  REQUIRE(e && wave_host && spec_host && B > 0, "asx_stft: bad argument");
  REQUIRE(C > e->cfg.n_fft / 2, "asx_stft: n_time %lld must exceed n_fft/2 (reflect padding)", (long long)C);
  HIPCHK(hipSetDevice(e->device));
  const int T = (int)(C / e->cfg.hop_length) + 1;
  const size_t ns = (size_t)B * 4 * e->cfg.dim_f * T;
  return host_round_trip(wave_host, (size_t)B * 2 * C, spec_host, ns, [&](const float *w, float *spec) {
    return stft_launch(e, w, nullptr, -1, B, C, T, spec, 0, 0, 1.0f, nullptr);
  });
}

int asx_istft(asx_engine *e, const float *spec_host, int32_t B, int32_t T, float *wave_host) {
  REQUIRE(e && spec_host && wave_host && B > 0 && T >= 1, "asx_istft: bad argument");
  HIPCHK(hipSetDevice(e->device));
  const int n = e->cfg.n_fft, hop = e->cfg.hop_length;
  const int64_t C = (int64_t)hop * (T - 1);
  REQUIRE(C > 0, "asx_istft: need at least 2 frames");
  const size_t ns = (size_t)B * 4 * e->cfg.dim_f * T;
  DevBuf dsp, dfr, denv, dout;
  BufGuard g{{&dsp, &dfr, &denv, &dout}};
  CHK(to_dev(dsp, spec_host, ns));
  CHK(dfr.ensure((size_t)B * 2 * T * n * 4));
  CHK(dout.ensure((size_t)B * 2 * C * 4));
  std::vector<float> env;
  host_env(n, hop, T, env, e->cfg.win_length, &e->custom_window);
  CHK(to_dev(denv, env.data(), env.size()));
  CHK(istft_launch(e, dsp.f(), B, T, 0, 0, dfr.f(), nullptr));
  CHK(ola_launch(e, dfr.f(), denv.f(), nullptr, B, T, C, dout.f(), nullptr));
  CHK(to_host(wave_host, dout, (size_t)B * 2 * C));
  return ASX_OK;
}

int asx_net_forward(asx_engine *e, const float *spec_host, int32_t B, float *out_host) {
  REQUIRE(e && spec_host && out_host && B > 0, "asx_net_forward: bad argument");
  if (!e->net_ready) {
    set_err("asx_net_forward: net weights not committed");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  const int T = e->net.dim_t, Fq = e->net.dim_f, dc = e->net.dim_c;
  REQUIRE(dc == 4, "asx_net_forward: dim_c must be 4");
  const bool den = e->cfg.enable_denoise;
  e->cfg.enable_denoise = 0;  // size the workspace for exactly B
  int rc = ensure_workspace(e, B, true);
  e->cfg.enable_denoise = den;
  CHK(rc);
  const size_t ns = (size_t)B * dc * Fq * T;
  return host_round_trip(spec_host, ns, out_host, ns, [&](const float *in, float *out) -> int {
    // reference layout [B,4,F,T] -> engine layout [B,4,T,F]
    CHK(transpose_launch(in, e->spec_in.f(), B * dc, Fq, T, nullptr));
    CHK(net_forward_dev(e, e->spec_in.f(), e->spec_out.f(), B, nullptr));
    return transpose_launch(e->spec_out.f(), out, B * dc, T, Fq, nullptr);
  });
}

int asx_run_model(asx_engine *e, const float *wave_host, int32_t B, float *out_host, uint32_t flags) {
  REQUIRE(e && wave_host && out_host && B > 0, "asx_run_model: bad argument");
  HIPCHK(hipSetDevice(e->device));
  const bool match = (flags & ASX_FLAG_MATCH_MIX) != 0;
  if (!match && !e->net_ready) {
    set_err("asx_run_model: net weights not committed");
    return ASX_ERR_STATE;
  }
  const int T = e->cfg.segment_size;
  const int64_t C = (int64_t)e->cfg.hop_length * (T - 1);
  CHK(ensure_workspace(e, B, !match));
  DevBuf dw, dout;
  BufGuard g{{&dw, &dout}};
  CHK(to_dev(dw, wave_host, (size_t)B * 2 * C));
  CHK(dout.ensure((size_t)B * 2 * C * 4));
  const size_t spec_elems = (size_t)4 * T * e->cfg.dim_f;
  CHK(stft_launch(e, dw.f(), nullptr, -1, B, C, T, e->spec_in.f(), 1, 3, 1.0f, nullptr));
  const float *spec_final = e->spec_in.f();
  int combine = 0;
  if (!match) {
    int Bn = B;
    if (e->cfg.enable_denoise) {
      CHK(stft_launch(e, dw.f(), nullptr, -1, B, C, T, e->spec_in.f() + (size_t)B * spec_elems, 1, 3, -1.0f, nullptr));
      Bn = 2 * B;
      combine = B;
    }
    CHK(net_forward_dev(e, e->spec_in.f(), e->spec_out.f(), Bn, nullptr));
    spec_final = e->spec_out.f();
  }
  CHK(istft_ola_launch(e, spec_final, B, T, combine, nullptr, C, dout.f(), nullptr));
  CHK(to_host(out_host, dout, (size_t)B * 2 * C));
  return ASX_OK;
}

// ---- single-layer hooks --------------------------------------------------------
int asx_op_conv(asx_engine *e, const char *op, const float *x_host, int32_t B, int32_t cin, int32_t t, int32_t f,
                const float *w_host, const float *b_host, int32_t cout, const float *aux_host, int32_t relu,
                float *y_host) {
  REQUIRE(e && op && x_host && w_host && y_host && B > 0 && cin > 0 && cout > 0 && t > 0 && f > 0,
          "asx_op_conv: bad argument");
  HIPCHK(hipSetDevice(e->device));
  int kind;
  int to = t, fo = f;
  // "conv3x3_to_tiled" / "conv3x3_tiled" / "conv3x3_from_tiled": the 3x3 layer with its output / both / its input in conv3h_kernel's tile
  // order (Conv3hCfg::tl_off per 48-channel slice), the raw buffer handed to or taken from the host -- an error where conv3h_kernel does not take the layer
  ConvView view;
  if (!strcmp(op, "conv3x3")) kind = CK_3X3;
  else if (!strcmp(op, "conv3x3_to_tiled") || !strcmp(op, "conv3x3_tiled") || !strcmp(op, "conv3x3_from_tiled")) {
    kind = CK_3X3;
    view.x_tiled = strcmp(op, "conv3x3_to_tiled") != 0;
    view.y_tiled = strcmp(op, "conv3x3_from_tiled") != 0;
  } else if (!strcmp(op, "down")) {
    kind = CK_DOWN;
    to = t / 2;
    fo = f / 2;
  } else if (!strcmp(op, "conv1x1")) kind = CK_1X1;
  else if (!strcmp(op, "up")) {
    kind = CK_UP;
    to = 2 * t;
    fo = 2 * f;
    REQUIRE(aux_host, "asx_op_conv(up): skip tensor required");
  } else {
    set_err("asx_op_conv: unknown op '%s'", op);
    return ASX_ERR_INVALID;
  }
  ConvLayer L;
  DevBuf dx, dy, dskip;
  BufGuard g{{&dx, &dy, &dskip, &L.w, &L.b, &L.wu, &L.wu2, &L.wu3, &L.wus, &L.wu6, &L.wu6h, &L.w3h, &L.wd6, &L.wup6}};
  CHK(conv_setup(L, kind, cin, cout, relu ? 1 : 0));
  CHK(conv_pack(L, w_host, b_host, e->winograd));
  CHK(to_dev(dx, x_host, (size_t)B * cin * t * f));
  const size_t ny = (size_t)B * cout * to * fo;
  CHK(dy.ensure(ny * 4));
  HIPCHK(hipMemset(dy.p, 0xff, ny * 4));  // NaN canary: every output element must be written
  if (kind == CK_UP) CHK(to_dev(dskip, aux_host, ny));
  CHK(e->c3h_ps.ensure(conv3h_ps_need(L, B, t, f)));   // (the nets size it with their workspaces; to_host below waits before anything else can regrow it)
  CHK(conv3h_walk_ensure(e, L, B, t, f));
  CHK(conv_launch(e, L, dx.f(), dskip.f(), dy.f(), B, t, f, nullptr, view));
  CHK(to_host(y_host, dy, ny));
  return ASX_OK;
}

int asx_op_tdf(asx_engine *e, const float *x_host, int32_t B, int32_t c, int32_t t, int32_t k, const float *w_host,
               const float *bias_host, int32_t n, const float *scale_host, const float *shift_host,
               const float *res_host, float *y_host) {
  REQUIRE(e && x_host && w_host && scale_host && shift_host && y_host && B > 0 && c > 0 && t > 0 && k > 0 && n > 0,
          "asx_op_tdf: bad argument");
  HIPCHK(hipSetDevice(e->device));
  TdfLayer L;
  DevBuf dx, dy, dres;
  BufGuard g{{&dx, &dy, &dres, &L.w, &L.bias, &L.scale, &L.shift}};
  CHK(tdf_pack(L, n, k, c, w_host, bias_host, scale_host, shift_host));
  const int64_t M = (int64_t)B * c * t;
  CHK(to_dev(dx, x_host, (size_t)M * k));
  CHK(dy.ensure((size_t)M * n * 4));
  HIPCHK(hipMemset(dy.p, 0xff, (size_t)M * n * 4));
  if (res_host) CHK(to_dev(dres, res_host, (size_t)M * n));
  const int rc = tdf_launch(e, L, dx.f(), res_host ? dres.f() : nullptr, dy.f(), M, t, nullptr);
  const int rc2 = rc == ASX_OK ? to_host(y_host, dy, (size_t)M * n) : rc;   // synchronises: the launch is done with the image
  w3_drop(e, L.w.p);                                   // the temporary layer's split image goes with its weight buffer
  return rc2;
}

// x + tdf1(tdf0(x)): the two linears of a TDF block with a bottleneck, launched the way the net launches them (tdf_pair_launch: the bottleneck
// activations as a pair image when option "gemm_pair_images" and the shapes allow).  h_host (optional): the bottleneck activations as fp32 --
// decoded from the pair image when one was written
int asx_op_tdf_block(asx_engine *e, const float *x_host, int32_t B, int32_t c, int32_t t, int32_t f, const float *w0_host, const float *scale0_host,
                     const float *shift0_host, int32_t n8, const float *w1_host, const float *scale1_host, const float *shift1_host, float *y_host,
                     float *h_host) {
  REQUIRE(e && x_host && w0_host && w1_host && scale0_host && shift0_host && scale1_host && shift1_host && y_host && B > 0 && c > 0 && t > 0 &&
              f > 0 && n8 > 0,
          "asx_op_tdf_block: bad argument");
  HIPCHK(hipSetDevice(e->device));
  TdfLayer L0, L1;
  DevBuf dx, dy, dh, dhe;
  BufGuard g{{&dx, &dy, &dh, &dhe, &L0.w, &L0.bias, &L0.scale, &L0.shift, &L1.w, &L1.bias, &L1.scale, &L1.shift}};
  CHK(tdf_pack(L0, n8, f, c, w0_host, nullptr, scale0_host, shift0_host));
  CHK(tdf_pack(L1, f, n8, c, w1_host, nullptr, scale1_host, shift1_host));
  const int64_t M = (int64_t)B * c * t;
  CHK(to_dev(dx, x_host, (size_t)M * f));
  CHK(dy.ensure((size_t)M * f * 4));
  CHK(dh.ensure((size_t)M * n8 * 4 + 256));
  CHK(dhe.ensure((size_t)M * ((n8 + 127) / 128) * 4 + 256));
  HIPCHK(hipMemset(dy.p, 0xff, (size_t)M * f * 4));
  HIPCHK(hipMemset(dh.p, 0xff, (size_t)M * n8 * 4));
  HIPCHK(hipMemset(dhe.p, 0xff, (size_t)M * ((n8 + 127) / 128) * 4));
  const long long ps0 = g_tdf3ps_launches.load();
  int rc = tdf_pair_launch(e, L0, L1, dx.f(), dh.f(), reinterpret_cast<int *>(dhe.p), dy.f(), M, t, nullptr);
  if (rc == ASX_OK) rc = to_host(y_host, dy, (size_t)M * f);   // synchronises: the launches are done with the images
  if (rc == ASX_OK && h_host) {
    rc = to_host(h_host, dh, (size_t)M * n8);
    if (rc == ASX_OK && g_tdf3ps_launches.load() != ps0) {
      // pair image -> fp32 on the host: groups of four columns as h0..h3 l0..l3, exponent per (row, column tile of the first linear)
      TdfDmaArgs d0;
      tdf_fill_args(e, L0, dx.f(), nullptr, dh.f(), M, t, 1, d0);
      const int cols = tdf3_tile_cols(e, d0), nsp = (n8 + cols - 1) / cols;
      std::vector<int> ex((size_t)M * nsp);
      HIPCHK(hipMemcpy(ex.data(), dhe.p, ex.size() * 4, hipMemcpyDeviceToHost));
      std::vector<uint16_t> raw(8);
      for (int64_t r = 0; r < M; ++r)
        for (int g4 = 0; g4 < n8 / 4; ++g4) {
          float *grp = h_host + r * n8 + g4 * 4;
          memcpy(raw.data(), grp, 16);
          for (int i = 0; i < 4; ++i) grp[i] = ldexpf(conv3h_f16_f(raw[i]) + conv3h_f16_f(raw[4 + i]), -ex[(size_t)r * nsp + (g4 * 4) / cols]);
        }
    }
  }
  w3_drop(e, L0.w.p);
  w3_drop(e, L1.w.p);
  return rc;
}

// single attention launches through the engines' launch code (engine_attn.h); the output is uploaded first, so the caller sees exactly which
// elements the kernel wrote
int asx_op_attention(asx_engine *e, const float *qkv_host, const float *gate_host, int64_t M, int32_t B, int32_t T, int32_t Fb, int32_t axis,
                     int32_t heads, int32_t gate_ld, int32_t exact, const char *variant, float *out_host, int32_t *resolved) {
  REQUIRE(e && qkv_host && gate_host && out_host && B > 0 && T > 0 && Fb > 0 && (axis == 0 || axis == 1) && heads > 0 && gate_ld >= heads &&
              M >= (int64_t)B * T * Fb,
          "asx_op_attention: bad argument");
  int v;
  CHK(attn_variant_parse(variant, &v));
  HIPCHK(hipSetDevice(e->device));
  AttnArgs a{};
  const int64_t nseq = rof_attn_geometry(a, B, T, Fb, axis == 0);
  if (v == AV_AUTO) v = rof_attn_variant(e, a.len);
  REQUIRE((v >= AV_ATTN2 && v <= AV_ATTN6H_QW2) || v == AV_ATTN6S || v == AV_ATTN6S_QW2, "asx_op_attention: '%s' is not a Roformer attention variant", k_attn_variant_names[v]);
  const int inner = heads * 64;
  DevBuf dqkv, dgate, dout;
  BufGuard g{{&dqkv, &dgate, &dout}};
  CHK(to_dev(dqkv, qkv_host, (size_t)M * 3 * inner));
  CHK(to_dev(dgate, gate_host, (size_t)M * gate_ld));
  CHK(to_dev(dout, out_host, (size_t)M * inner));
  a.qkv = dqkv.f();
  a.gate = dgate.f();
  a.out = dout.f();
  a.heads = heads;
  a.gate_ld = gate_ld;
  a.scale = 1.0f / sqrtf(64.0f);
  a.exact = exact ? 1 : 0;
  CHK(rof_attn_launch(e, v, a, nseq, nullptr));
  HIPCHK(hipGetLastError());
  CHK(to_host(out_host, dout, (size_t)M * inner));
  if (resolved) *resolved = v;
  return ASX_OK;
}

int asx_op_mha(asx_engine *e, const float *q_host, int64_t ldq, const float *k_host, int64_t ldk, const float *v_host, int64_t ldv,
               const float *decay_host, int64_t ldd, int32_t B, int32_t nq, int32_t nk, int32_t heads, int32_t dh, int32_t exact, const char *variant,
               float *out_host, int64_t ldo, int32_t *resolved) {
  REQUIRE(e && q_host && k_host && v_host && out_host && B > 0 && nq > 0 && nk > 0 && heads > 0 && dh > 0,
          "asx_op_mha: bad argument");
  const int64_t hd = (int64_t)heads * dh;
  REQUIRE(ldq >= hd && ldk >= hd && ldv >= hd && ldo >= hd, "asx_op_mha: leading dimensions must be at least heads * dh = %lld", (long long)hd);
  REQUIRE(!decay_host || (ldd >= 4 * (int64_t)heads && nq == nk), "asx_op_mha: decay logits need nq == nk and ldd >= 4 * heads");
  int v;
  CHK(attn_variant_parse(variant, &v));
  HIPCHK(hipSetDevice(e->device));
  MhaArgs a{};
  a.ldq = ldq;
  a.ldk = ldk;
  a.ldv = ldv;
  a.ldo = ldo;
  a.ldd = ldd;
  a.nq = nq;
  a.nk = nk;
  a.scale = 1.0f / sqrtf((float)dh);
  a.exact = exact ? 1 : 0;
  static const float dummy = 0.f;
  a.decay = decay_host ? &dummy : nullptr;   // the rules and checks below look only at whether it is set
  if (v == AV_AUTO) {
    v = decay_host ? hd_attn_variant(a, dh) : ht_mha_variant(e, a, nq, dh);
    REQUIRE(v != AV_AUTO, "asx_op_mha: no attention kernel is built for dh %d", dh);
  }
  if (v == AV_HD_LOCAL)
    REQUIRE(decay_host && heads == 4 && hd_local_ok(dh) && ldo == hd,
            "asx_op_mha: 'hd_local' takes decay logits, 4 heads, dh 4 / 8 / 12 / 24 and ldo == heads * dh");
  else
    REQUIRE(v >= AV_MHA && v <= AV_MHA6H_WIDE && mha_variant_ok(v, a, dh), "asx_op_mha: variant '%s' is not built for these arguments (dh %d)",
            k_attn_variant_names[v], dh);
  DevBuf dq, dk, dv, dd, dout;
  BufGuard g{{&dq, &dk, &dv, &dd, &dout}};
  CHK(to_dev(dout, out_host, (size_t)B * nq * ldo));
  if (v == AV_HD_LOCAL) {
    // the engine's LocalState layout: one matrix [B * T, 3 H + 16] of query | key | content | decay logits
    const int H = (int)hd, ld = 3 * H + 16;
    const int64_t rows = (int64_t)B * nq;
    std::vector<float> qkvd((size_t)rows * ld, 0.f);
    for (int64_t r = 0; r < rows; ++r) {
      float *dst = qkvd.data() + r * ld;
      memcpy(dst, q_host + r * ldq, H * 4);
      memcpy(dst + H, k_host + r * ldk, H * 4);
      memcpy(dst + 2 * H, v_host + r * ldv, H * 4);
      memcpy(dst + 3 * H, decay_host + r * ldd, 16 * 4);
    }
    CHK(to_dev(dq, qkvd.data(), qkvd.size()));
    hd_local_launch(dq.f(), ld, nq, H, dout.f(), B, nullptr);
  } else {
    CHK(to_dev(dq, q_host, (size_t)B * nq * ldq));
    CHK(to_dev(dk, k_host, (size_t)B * nk * ldk));
    CHK(to_dev(dv, v_host, (size_t)B * nk * ldv));
    if (decay_host) CHK(to_dev(dd, decay_host, (size_t)B * nq * ldd));
    a.q = dq.f();
    a.k = dk.f();
    a.v = dv.f();
    a.out = dout.f();
    a.decay = decay_host ? dd.f() : nullptr;
    mha_launch(e, v, a, B, heads, dh, nullptr);
  }
  HIPCHK(hipGetLastError());
  CHK(to_host(out_host, dout, (size_t)B * nq * ldo));
  if (resolved) *resolved = v;
  return ASX_OK;
}

// single launches of the recurrent kernels through the engines' launch code (engine_hd.h, engine_vr.h); outputs are uploaded first
int asx_op_hd_lstm_layer(asx_engine *e, const float *xp_host, const float *whh_host, int32_t N, int32_t H, int32_t steps, float *out_host,
                         float *c_host) {
  REQUIRE(e && xp_host && whh_host && out_host && N > 0 && H > 0 && steps > 0, "asx_op_hd_lstm_layer: bad argument");
  REQUIRE(H % 16 == 0, "asx_op_hd_lstm_layer: the hidden size must be a multiple of 16, got %d", H);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dxp, dwhh, dout, dhb, dcst;
  BufGuard g{{&dxp, &dwhh, &dout, &dhb, &dcst}};
  const size_t rows = (size_t)steps * N;
  CHK(to_dev(dxp, xp_host, rows * 8 * H));
  CHK(to_dev(dwhh, whh_host, (size_t)8 * H * H));
  CHK(to_dev(dout, out_host, rows * 2 * H));
  CHK(dhb.ensure((size_t)4 * N * H * 4));
  CHK(dcst.ensure((size_t)2 * N * H * 4));
  CHK(hd_lstm_recurrence(e, dxp.f(), dwhh.f(), dhb.f(), dcst.f(), dout.f(), N, H, steps, nullptr));
  CHK(to_host(out_host, dout, rows * 2 * H));
  if (c_host) CHK(to_host(c_host, dcst, (size_t)2 * N * H));
  return ASX_OK;
}

int asx_op_hd_lstm_frames(asx_engine *e, int32_t dir, float *h_host, int32_t B, int32_t T, int32_t H, int32_t ntot, int32_t n_off,
                          float *rows_host, int32_t *steps_out, int32_t *nfr_out) {
  REQUIRE(e && h_host && rows_host && (dir == 0 || dir == 1) && B > 0 && T > 0 && H > 0 && n_off >= 0, "asx_op_hd_lstm_frames: bad argument");
  int steps, nfr;
  hd_lstm_framing(T, steps, nfr);
  REQUIRE((int64_t)n_off + (int64_t)B * nfr <= ntot, "asx_op_hd_lstm_frames: %d x %d sequences from %d do not fit in %d", B, nfr, n_off, ntot);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dh, drows;
  BufGuard g{{&dh, &drows}};
  const size_t nh = (size_t)B * T * H, nr = (size_t)steps * ntot * H;
  CHK(to_dev(dh, h_host, nh));
  CHK(to_dev(drows, rows_host, nr));
  if (dir == 0) {
    const int64_t tot = (int64_t)steps * B * nfr * H;
    CHK(timed(e, ASX_PROF_MISC, 0.0, 8.0 * (double)tot, nullptr, [&]() {
      hipLaunchKernelGGL(hd_lstm_frame_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, nullptr, dh.f(), B, T, H, nfr, steps, 100, ntot,
                         n_off, drows.f(), tot);
    }));
    CHK(to_host(rows_host, drows, nr));
  } else {
    const int64_t tot = (int64_t)nh;
    CHK(timed(e, ASX_PROF_MISC, 0.0, 12.0 * (double)tot, nullptr, [&]() {
      hipLaunchKernelGGL(hd_lstm_unframe_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, nullptr, drows.f(), B, T, H, nfr, 100, ntot,
                         n_off, dh.f(), tot);
    }));
    CHK(to_host(h_host, dh, nh));
  }
  if (steps_out) *steps_out = steps;
  if (nfr_out) *nfr_out = nfr;
  return ASX_OK;
}

int asx_op_vr_lstm(asx_engine *e, const float *xp_host, const float *whh_host, int32_t W, int32_t B, int32_t hs, float *out_host) {
  REQUIRE(e && xp_host && whh_host && out_host && W > 0 && B > 0, "asx_op_vr_lstm: bad argument");
  REQUIRE(hs == 4 || hs == 8 || hs == 16 || hs == 32 || hs == 64 || hs == 128, "asx_op_vr_lstm: hidden size %d per direction is not built", hs);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dxp, dwhh, dout;
  BufGuard g{{&dxp, &dwhh, &dout}};
  CHK(to_dev(dxp, xp_host, (size_t)W * B * 8 * hs));
  CHK(to_dev(dwhh, whh_host, (size_t)8 * hs * hs));
  CHK(to_dev(dout, out_host, (size_t)W * B * 2 * hs));
  CHK(vr51_lstm(e, hs, dxp.f(), dwhh.f(), W, B, dout.f(), nullptr));
  return to_host(out_host, dout, (size_t)W * B * 2 * hs);
}

int asx_op_vr_lstm_layout(asx_engine *e, int32_t dir, const float *src_host, int32_t B, int32_t H, int32_t W, int32_t ld, int32_t ch0,
                          float *dst_host) {
  REQUIRE(e && src_host && dst_host && (dir == 0 || dir == 1) && B > 0 && H > 0 && W > 0 && ld > 0 && ch0 >= 0, "asx_op_vr_lstm_layout: bad argument");
  // vr_lstm_out_kernel stores channels ch0 .. ch0+3 of a pixel as one 16-byte vector
  if (dir == 0) REQUIRE(ch0 < ld, "asx_op_vr_lstm_layout: channel %d of %d", ch0, ld);
  else REQUIRE(ld % 4 == 0 && ch0 % 4 == 0 && ch0 + 4 <= ld, "asx_op_vr_lstm_layout: channels %d .. %d of %d are no aligned group of four", ch0, ch0 + 3, ld);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dsrc, ddst;
  BufGuard g{{&dsrc, &ddst}};
  const size_t np = (size_t)B * H * W;
  CHK(to_dev(dsrc, src_host, dir == 0 ? np * ld : np));
  CHK(to_dev(ddst, dst_host, dir == 0 ? np : np * ld));
  if (dir == 0) CHK(vr_ew(e, nullptr, (int64_t)np, 8.0 * np, vr_lstm_in_kernel, (const float *)(dsrc.f() + ch0), B, H, W, ld, ddst.f()));
  else CHK(vr_ew(e, nullptr, (int64_t)np, 8.0 * np, vr_lstm_out_kernel, (const float *)dsrc.f(), B, H, W, ddst.f(), ld, ch0));
  return to_host(dst_host, ddst, dir == 0 ? np : np * ld);
}

// one ht_gg launch from host buffers (engine_ht.h); every check below keeps the kernels' reads and writes inside the buffers uploaded here
int asx_op_gconv(asx_engine *e, const asx_gconv_desc *d, const float *x_host, const float *w_host, const float *b_host,
                 const float *res_host, const char *variant, float *y_host, int32_t *resolved) {
  REQUIRE(e && d && x_host && w_host && b_host && y_host && variant, "asx_op_gconv: null argument");
  int only = -1;
  {
    static const char *names[4] = {"auto", "gg", "halo", "gather"};
    for (int i = 0; i < 4; ++i)
      if (!strcmp(variant, names[i])) only = i;
  }
  REQUIRE(only >= 0, "asx_op_gconv: unknown variant '%s'", variant);
  const int OR = d->OR ? d->OR : d->O;
  REQUIRE(d->B > 0 && d->O > 0 && d->I > 0 && d->Cin > 0 && d->Cout > 0 && OR > 0 && d->IR > 0, "asx_op_gconv: sizes must be positive");
  REQUIRE(d->KO >= 1 && d->KO <= 3 && d->KI >= 1 && d->KI <= 16 && d->DO >= 1 && d->DI >= 1 && d->PO >= 0 && d->PI >= 0 && d->SO >= 1 && d->SI >= 1,
          "asx_op_gconv: taps %d x %d (at most 3 x 16), dilations, paddings and strides out of range", d->KO, d->KI);
  REQUIRE((d->Cin & 3) == 0 && (d->ldc & 3) == 0 && (d->x_col0 & 3) == 0 && d->x_col0 >= 0 && d->x_col0 + d->Cin <= d->ldc,
          "asx_op_gconv: Cin %d at column %d does not fit pixels of %d floats in whole groups of four", d->Cin, d->x_col0, d->ldc);
  REQUIRE((d->Cout & 3) == 0 && (d->ldy & 3) == 0 && (d->y_col0 & 3) == 0 && d->y_col0 >= 0 && d->y_col0 + d->Cout <= d->ldy,
          "asx_op_gconv: Cout %d at column %d does not fit rows of %d floats in whole groups of four", d->Cout, d->y_col0, d->ldy);
  REQUIRE(d->mode >= GG_DENSE && d->mode <= GG_CONVT && d->act >= 0 && d->act <= 6 && (d->mode != GG_GLU || d->act == 0),
          "asx_op_gconv: mode %d / act %d", d->mode, d->act);
  const int64_t x_img = (int64_t)d->O * d->I * d->ldc, x_bs = d->x_bs ? d->x_bs : x_img;
  const bool convt = d->mode == GG_CONVT;
  const int64_t y_img = convt ? (int64_t)d->O * d->Iout * d->ldy : (int64_t)OR * d->IR * d->ldy, y_bs = (d->y_bs && !convt) ? d->y_bs : y_img;
  REQUIRE(x_bs >= x_img && y_bs >= y_img && (!convt || d->y_bs == 0), "asx_op_gconv: batch strides smaller than an image");
  if (convt)
    REQUIRE(d->KO == 1 && d->KI == 2 && d->SO == 1 && d->SI == 1 && OR == d->O && d->So >= 1 && d->So <= 8 && d->Iout > 0 && d->crop >= 0 &&
                d->res_mod == 0,
            "asx_op_gconv: ConvTranspose takes KO 1, KI 2, unit strides, So 1 .. 8, Iout > 0, crop >= 0 and no residual table");
  const int64_t M = (int64_t)d->B * OR * d->IR;
  const int64_t nx = (int64_t)d->B * x_bs, ny = (int64_t)d->B * y_bs;
  REQUIRE(nx < (1ll << 28) && ny < (1ll << 28) && M < (1ll << 26), "asx_op_gconv: the case is too large for a single-op test");
  const int64_t res_rows = d->res_mod > 0 ? d->res_mod : (convt ? (int64_t)d->B * d->O * d->Iout : M);
  if (d->res)
    REQUIRE(res_host && (d->ldr & 3) == 0 && d->ldr >= d->Cout && d->res_mod >= 0, "asx_op_gconv: residual rows of %d floats for %d channels",
            d->ldr, d->Cout);
  HIPCHK(hipSetDevice(e->device));
  HtGemm g;
  DevBuf dx, dy, dres;
  BufGuard guard{{&dx, &dy, &dres, &g.w, &g.b, &g.wh}};
  const bool want_halo = (only == 0 && !d->no_halo) || only == 2;
  if (convt) CHK(ht_pack_convtr_ptr(g, w_host, b_host, d->Cin, d->Cout, 2 * d->So, d->So));
  else if (d->mode == GG_GLU) CHK(ht_pack_conv_ptr(g, w_host, b_host, 2 * d->Cout, d->Cin, d->KI, d->KO, true, 0, 0, want_halo));
  else CHK(ht_pack_conv_ptr(g, w_host, b_host, d->Cout, d->Cin, d->KI, d->KO, false, 0, 0, want_halo));
  CHK(to_dev(dx, x_host, (size_t)nx));
  CHK(to_dev(dy, y_host, (size_t)ny));
  if (d->res) CHK(to_dev(dres, res_host, (size_t)res_rows * d->ldr));
  HtGeom q;
  q.O = d->O;
  q.I = d->I;
  q.Cin = d->Cin;
  q.ldc = d->ldc;
  q.KO = d->KO;
  q.KI = d->KI;
  q.DO = d->DO;
  q.DI = d->DI;
  q.PO = d->PO;
  q.PI = d->PI;
  q.SI = d->SI;
  q.IR = d->IR;
  q.SO = d->SO;
  q.OR = OR;
  q.x_bs = x_bs;
  q.y_bs = convt ? 0 : y_bs;
  q.crop = d->crop;
  q.So = d->So;
  e->gg_only = only;
  e->gg_ran[0] = 0;
  int rc = ht_gg(e, g, dx.f() + d->x_col0, q, (int64_t)d->B * OR, dy.f() + d->y_col0, d->ldy, d->mode, d->act, d->res ? dres.f() : nullptr,
                 d->ldr, d->res_mod, d->Iout, d->Cout, nullptr);
  e->gg_only = 0;
  if (rc == ASX_OK && hipGetLastError() != hipSuccess) {
    set_err("asx_op_gconv: launch failed");
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK) rc = to_host(y_host, dy, (size_t)ny);
  else (void)hipDeviceSynchronize();
  w3_drop(e, g.w.p);                                   // the temporary layer's split image goes with its weight buffer
  if (resolved)
    for (int i = 0; i < 3; ++i) resolved[i] = e->gg_ran[i];
  return rc;
}

// one ht_dconv_layer call from host buffers, on a workspace of exactly the buffers it reads (engine_ht.h)
int asx_op_dconv(asx_engine *e, float *y_host, int32_t B, int32_t O, int32_t I, int32_t C, int32_t hid, int32_t along_outer, int32_t d,
                 int32_t part, const float *w1, const float *b1, const float *g1w, const float *g1b, const float *w2, const float *b2,
                 const float *g2w, const float *g2b, const float *ls, float *h_host, int32_t *ticket_left) {
  REQUIRE(e && y_host && w1 && b1 && g1w && g1b && w2 && b2 && g2w && g2b && ls, "asx_op_dconv: null argument");
  REQUIRE(B > 0 && O > 0 && I > 0 && C > 0 && (C & 3) == 0 && hid > 0 && hid <= C && d >= 0 && d <= 8 && part >= 1 && part <= 3,
          "asx_op_dconv: bad shape (c %d must be a multiple of 4, hid %d in 1 .. c, d %d in 0 .. 8, part %d in 1 .. 3)", C, hid, d, part);
  REQUIRE(part == 3 || h_host, "asx_op_dconv: parts 1 and 2 alone need h_host");
  REQUIRE(along_outer || O == 1, "asx_op_dconv: the inner-axis form is the waveform branch's, o must be 1 (got %d)", O);
  const int64_t M = (int64_t)B * O * I;
  REQUIRE(M * C < (1ll << 28), "asx_op_dconv: the case is too large for a single-op test");
  HIPCHK(hipSetDevice(e->device));
  HtEnc E;
  E.cin = E.cout = C;
  E.dc.assign((size_t)d + 1, HtDconv());
  HtDconv &dc = E.dc[d];
  HtNet net;
  DevBuf dy, dh, drow, dacc, dmr, dtick;
  BufGuard guard{{&dy, &dh, &drow, &dacc, &dmr, &dtick, &dc.c1.w, &dc.c1.b, &dc.c2.w, &dc.c2.b, &dc.g1w, &dc.g1b, &dc.g2w, &dc.g2b, &dc.ls}};
  CHK(ht_pack_dconv(dc, C, hid, w1, b1, g1w, g1b, w2, b2, g2w, g2b, ls));
  const int G2 = along_outer ? I : 1;
  const int np = dc.c2.n;
  const size_t t1 = (size_t)(dc.hp + gg_tile_n(dc.hp) - 1) / gg_tile_n(dc.hp), t2 = (size_t)(np + gg_tile_n(np, true) - 1) / gg_tile_n(np, true);
  const size_t ng = (size_t)B * G2;
  CHK(to_dev(dy, y_host, (size_t)M * C));
  if (h_host) CHK(to_dev(dh, h_host, (size_t)M * dc.hp));
  else CHK(dh.ensure((size_t)M * dc.hp * 4));
  CHK(drow.ensure((size_t)M * std::max(t1, t2) * 8));
  CHK(dacc.ensure(2 * ng * 16));
  CHK(dmr.ensure(ng * 8));
  CHK(dtick.ensure((size_t)B * 4));
  HIPCHK(hipMemset(dtick.p, 0, (size_t)B * 4));
  net.b.h = dh.f();
  net.b.rowstat = drow.f();
  net.b.acc_g = reinterpret_cast<double *>(dacc.p);
  net.b.acc_g2 = net.b.acc_g + 2 * ng;
  net.b.mr_g = dmr.f();
  net.b.ticket = reinterpret_cast<unsigned *>(dtick.p);
  HtNet *const saved = e->ht;
  e->ht = &net;
  int rc = ht_dconv_layer(e, E, (size_t)d, part, dy.f(), B, O, I, along_outer != 0, nullptr);
  e->ht = saved;
  if (rc == ASX_OK && hipGetLastError() != hipSuccess) {
    set_err("asx_op_dconv: launch failed");
    rc = ASX_ERR_HIP;
  }
  if (rc == ASX_OK) rc = to_host(y_host, dy, (size_t)M * C);
  else (void)hipDeviceSynchronize();
  if (rc == ASX_OK && h_host) rc = to_host(h_host, dh, (size_t)M * dc.hp);
  if (rc == ASX_OK && ticket_left) {
    std::vector<unsigned> t((size_t)B);
    if (hipMemcpy(t.data(), dtick.p, (size_t)B * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      set_err("asx_op_dconv: reading the arrival counters failed");
      rc = ASX_ERR_HIP;
    }
    int nz = 0;
    for (unsigned v : t) nz += v != 0;
    *ticket_left = nz;
  }
  w3_drop(e, dc.c1.w.p);
  w3_drop(e, dc.c2.w.p);
  return rc;
}

// ---- single STFT / iSTFT launches ------------------------------------------------------
static int table_to_dev(DevBuf &d, const void *h, size_t bytes) {
  CHK(d.ensure(bytes));
  HIPCHK(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
  return ASX_OK;
}

// the checks both directions share; *need = the floats of the spectrum the launch touches
static int op_stft_check(const asx_engine *e, const asx_stft_desc *d, bool inverse, int64_t *need) {
  const int64_t F = e->cfg.dim_f, T = d->t;
  const int S = d->n_inst > 1 ? d->n_inst : 1;
  REQUIRE(d->b > 0 && d->t >= (inverse ? 2 : 1) && d->c > 0 && d->b <= 64 && d->t <= 4096, "asx_op_stft / istft: b %d, t %d, c %lld", d->b, d->t,
          (long long)d->c);
  REQUIRE(d->layout >= 0 && d->layout <= 2 && d->subbands >= 0 && d->n_inst >= 0 && d->bstride >= 0, "asx_op_stft / istft: layout %d, subbands %d",
          d->layout, d->subbands);
  if (d->subbands >= 1) REQUIRE(d->layout == 1 && F % d->subbands == 0, "asx_op_stft / istft: %d subbands need layout 1 and divide dim_f", d->subbands);
  else REQUIRE(d->bstride == 0 && (d->n_inst <= 1 || d->layout == 2), "asx_op_stft / istft: batch strides and stems need subbands >= 1 (or layout 2)");
  if (!inverse) REQUIRE(d->n_inst == 0 && d->combine == 0, "asx_op_stft: n_inst / combine belong to the inverse");
  if (d->combine) REQUIRE(d->combine == 1 && S == 1 && d->layout != 2, "asx_op_istft: combine takes one stem per item and layout 0 / 1");
  if (d->stft_normalized) REQUIRE(d->layout == 2, "asx_op_stft / istft: stft_normalized belongs to layout 2");
  const int64_t item = (int64_t)S * 4 * T * F, items = (int64_t)d->b * (d->combine ? 2 : 1);
  if (d->layout == 2) *need = (int64_t)d->b * T * F * 4;
  else {
    REQUIRE(d->bstride == 0 || d->bstride >= item, "asx_op_stft / istft: bstride %lld below an item of %lld floats", (long long)d->bstride, (long long)item);
    *need = (items - 1) * (d->bstride ? d->bstride : item) + item;
  }
  REQUIRE(d->spec_floats >= *need && d->spec_floats < (1ll << 28), "asx_op_stft / istft: spec_floats %lld, the launch touches %lld", (long long)d->spec_floats,
          (long long)*need);
  return ASX_OK;
}

int asx_op_stft(asx_engine *e, const asx_stft_desc *d, const float *wave_host, float *spec_host, int32_t *resolved) {
  REQUIRE(e && d && wave_host && spec_host, "asx_op_stft: null argument");
  int64_t need = 0;
  CHK(op_stft_check(e, d, false, &need));
  const int n = e->cfg.n_fft, hop = e->cfg.hop_length, B = d->b, T = d->t;
  const int64_t C = d->c;
  REQUIRE(C > n / 2 && (int64_t)(T - 1) * hop + n / 2 - 1 <= 2 * (C - 1), "asx_op_stft: c %lld too short for %d frames (one reflection)", (long long)C, T);
  REQUIRE(d->sign == 1.0f || d->sign == -1.0f, "asx_op_stft: sign must be +1 or -1");
  REQUIRE(d->zero_low >= 0 && d->mode >= 0 && d->mode <= 2 && d->front >= 0, "asx_op_stft: zero_low / mode / front");
  const int n_songs = d->mode == 2 ? d->n_songs : 1;
  int64_t n_wave = (int64_t)B * 2 * C;
  std::vector<int64_t> song_off;
  if (d->mode) {
    REQUIRE(d->starts && d->song_len && n_songs >= 1 && n_songs <= 64 && (d->mode == 1 || d->song_of), "asx_op_stft: song tables missing");
    n_wave = 0;
    for (int i = 0; i < n_songs; ++i) {
      REQUIRE(d->song_len[i] >= 1, "asx_op_stft: song %d is empty", i);
      song_off.push_back(n_wave);
      n_wave += 2 * d->song_len[i];
    }
    for (int i = 0; i < B; ++i) REQUIRE(d->mode == 1 || (d->song_of[i] >= 0 && d->song_of[i] < n_songs), "asx_op_stft: chunk %d names song %d", i, d->song_of[i]);
  }
  REQUIRE(n_wave < (1ll << 28), "asx_op_stft: the case is too large for a single-op test");
  HIPCHK(hipSetDevice(e->device));
  DevBuf dw, dsp, dst, dptr, dlen;
  BufGuard guard{{&dw, &dsp, &dst, &dptr, &dlen}};
  CHK(to_dev(dw, wave_host, (size_t)n_wave));
  CHK(to_dev(dsp, spec_host, (size_t)d->spec_floats));
  PoolChunks pc{};
  if (d->mode) CHK(table_to_dev(dst, d->starts, (size_t)B * 8));
  if (d->mode == 2) {
    std::vector<const float *> ptr(B);
    std::vector<int64_t> len(B);
    for (int i = 0; i < B; ++i) {
      ptr[i] = dw.f() + song_off[d->song_of[i]];
      len[i] = d->song_len[d->song_of[i]];
    }
    CHK(table_to_dev(dptr, ptr.data(), ptr.size() * sizeof(ptr[0])));
    CHK(table_to_dev(dlen, len.data(), len.size() * 8));
    pc.wave = reinterpret_cast<const float *const *>(dptr.p);
    pc.n_song = reinterpret_cast<const int64_t *>(dlen.p);
  }
  StftGeom g;
  if (d->layout == 2) g = rof_stft_geom(e, d->stft_normalized != 0);
  else if (d->subbands >= 1) g = v3_stft_geom(d->subbands, d->bstride, 0);
  else g.tf_layout = d->layout;
  g.trim = d->front;
  g.zero_low = d->zero_low;
  g.sign *= d->sign;
  e->fft_ran[0] = e->fft_ran[1] = 0;
  const float *wave = dw.f();                          // mode 0: explicit chunks [b, 2, c]
  const int64_t *starts = nullptr;
  int64_t n_song = -1;
  const PoolChunks *pool = nullptr;
  switch (d->mode) {
    case 1:                                            // one song: chunks are windows of it
      starts = reinterpret_cast<const int64_t *>(dst.p);
      n_song = d->song_len[0];
      break;
    case 2:                                            // a pool: song and length per chunk from the tables
      wave = nullptr;
      starts = reinterpret_cast<const int64_t *>(dst.p);
      n_song = 0;
      pool = &pc;
      break;
    default:
      break;
  }
  int rc = stft_launch(e, wave, starts, n_song, B, C, T, dsp.f(), g, nullptr, pool);
  if (rc == ASX_OK) rc = to_host(spec_host, dsp, (size_t)d->spec_floats);
  else (void)hipDeviceSynchronize();
  if (resolved) {
    resolved[0] = e->fft_ran[0];
    resolved[1] = e->fft_ran[1];
  }
  return rc;
}

int asx_op_istft(asx_engine *e, const asx_stft_desc *d, const float *spec_host, const float *mask_host, float *wave_host, int32_t *resolved) {
  REQUIRE(e && d && spec_host && wave_host, "asx_op_istft: null argument");
  int64_t need = 0;
  CHK(op_stft_check(e, d, true, &need));
  const int n = e->cfg.n_fft, hop = e->cfg.hop_length, B = d->b, T = d->t, S = d->n_inst > 1 ? d->n_inst : 1;
  const int64_t C = d->c, F = e->cfg.dim_f;
  REQUIRE(C <= (int64_t)hop * (T - 1), "asx_op_istft: c %lld beyond hop (t - 1) = %lld", (long long)C, (long long)hop * (T - 1));
  REQUIRE((d->layout == 2) == (mask_host != nullptr), "asx_op_istft: the mask belongs to layout 2");
  const size_t n_out = (size_t)B * S * 2 * C, n_frames = (size_t)B * S * 2 * T * n;
  REQUIRE(n_frames < (1ull << 28), "asx_op_istft: the case is too large for a single-op test");
  HIPCHK(hipSetDevice(e->device));
  DevBuf dsp, dmask, dout, denv, dfr, dna, dwin;
  BufGuard guard{{&dsp, &dmask, &dout, &denv, &dfr, &dna, &dwin}};
  CHK(to_dev(dsp, spec_host, (size_t)d->spec_floats));
  if (mask_host) CHK(to_dev(dmask, mask_host, (size_t)B * S * T * F * 4));
  CHK(to_dev(dout, wave_host, n_out));
  std::vector<float> env;
  host_env(n, hop, T, env, e->cfg.win_length, &e->custom_window);
  CHK(to_dev(denv, env.data(), env.size()));
  if (d->n_act) CHK(table_to_dev(dna, d->n_act, (size_t)B * S * 8));
  const int64_t *dn = d->n_act ? reinterpret_cast<const int64_t *>(dna.p) : nullptr;
  e->fft_ran[0] = e->fft_ran[1] = 0;
  int rc;
  if (d->layout == 1 && d->subbands == 0) {
    // the MDX chunk loop's inverse: the fused fast path where the engine has it and the chunk fits it
    rc = e->frames.ensure(n_frames * 4);
    if (rc == ASX_OK) rc = istft_ola_launch(e, dsp.f(), B, T, d->combine ? B : 0, dn, C, dout.f(), nullptr, denv.f());
  } else {
    IstftGeom g;
    if (d->layout == 2) {
      rc = d->stft_normalized ? rof_win_synth(e, dwin) : ASX_OK;
      g = rof_istft_geom(dmask.f(), S, d->stft_normalized ? dwin.f() : nullptr);
    } else {
      rc = ASX_OK;
      if (d->subbands >= 1) g = v3_istft_geom(d->subbands, S, d->bstride);
      g.tf_layout = d->layout;
      g.combine = d->combine ? B : 0;
    }
    if (rc == ASX_OK) rc = dfr.ensure(n_frames * 4);
    if (rc == ASX_OK) rc = istft_launch(e, dsp.f(), B, T, g, dfr.f(), nullptr);
    if (rc == ASX_OK) rc = ola_launch(e, dfr.f(), denv.f(), dn, B * S, T, C, dout.f(), nullptr);
  }
  if (rc == ASX_OK) rc = to_host(wave_host, dout, n_out);
  else (void)hipDeviceSynchronize();
  if (resolved) {
    resolved[0] = e->fft_ran[0];
    resolved[1] = e->fft_ran[1];
  }
  return rc;
}

// the largest transform whose two LDS buffers (+ 1 element, ht_istft_lds) fit the 160 KB of a CU: 8 bytes x (nfft + 1) <= 160 KB
static const int HT_OP_MAX_NFFT = 16384;

int asx_op_ht_spec(asx_engine *e, int32_t nfft, const float *seg_host, int32_t B, int64_t L, int64_t el, int64_t Lv, float *spec_host) {
  REQUIRE(e && seg_host && spec_host && B > 0 && B <= 64 && L >= 1 && L < (1 << 24), "asx_op_ht_spec: bad argument");
  FftPlan plan{};
  REQUIRE(nfft >= 16 && nfft <= HT_OP_MAX_NFFT && nfft % 4 == 0 && make_plan(nfft, &plan), "asx_op_ht_spec: nfft %d", nfft);
  const int hop = nfft / 4, T = (int)((L + hop - 1) / hop);
  REQUIRE(el >= 0 && Lv >= el + L && Lv > hop / 2 * 3 && (int64_t)(T - 1) * hop + nfft - 1 - hop / 2 * 3 + el <= 2 * (Lv - 1),
          "asx_op_ht_spec: the extension el %lld / lv %lld does not carry the reflect padding", (long long)el, (long long)Lv);
  HIPCHK(hipSetDevice(e->device));
  DevBuf win, tw, env, dseg, dsp;
  BufGuard guard{{&win, &tw, &env, &dseg, &dsp}};
  CHK(ht_fft_tables(nfft, win, tw, env));
  ht_fft_grant_lds(plan);
  const size_t ns = (size_t)B * T * plan.nh * 4;
  CHK(to_dev(dseg, seg_host, (size_t)B * 2 * L));
  CHK(to_dev(dsp, spec_host, ns));
  int rc = ht_spec_launch(e, plan, win.f(), tw.p, dseg.f(), B, L, el, Lv, T, dsp.f(), nullptr);
  if (rc == ASX_OK) rc = to_host(spec_host, dsp, ns);
  else (void)hipDeviceSynchronize();
  return rc;
}

int asx_op_ht_ispec(asx_engine *e, int32_t nfft, const float *x_host, int32_t B, int32_t T, int32_t S, const double *acc_f, double n_stat,
                    const float *xt_host, const double *acc_t, int64_t L, float *out_host) {
  REQUIRE(e && x_host && acc_f && xt_host && acc_t && out_host && B > 0 && B <= 64 && T >= 1 && T <= 4096 && S >= 1 && S <= 16 && n_stat > 1.0,
          "asx_op_ht_ispec: bad argument");
  FftPlan plan{};
  REQUIRE(nfft >= 16 && nfft <= HT_OP_MAX_NFFT && nfft % 4 == 0 && make_plan(nfft, &plan), "asx_op_ht_ispec: nfft %d", nfft);
  const int hop = nfft / 4;
  REQUIRE(L >= 1 && L <= (int64_t)T * hop, "asx_op_ht_ispec: l %lld beyond t hop = %lld", (long long)L, (long long)T * hop);
  HIPCHK(hipSetDevice(e->device));
  DevBuf win, tw, env, dx, dxt, dfr, daf, dat, dout;
  BufGuard guard{{&win, &tw, &env, &dx, &dxt, &dfr, &daf, &dat, &dout}};
  CHK(ht_fft_tables(nfft, win, tw, env));
  ht_fft_grant_lds(plan);
  const size_t no = (size_t)B * S * 2 * L;
  CHK(to_dev(dx, x_host, (size_t)B * T * plan.nh * 4 * S));
  CHK(to_dev(dxt, xt_host, (size_t)B * L * 2 * S));
  CHK(table_to_dev(daf, acc_f, (size_t)B * 16));
  CHK(table_to_dev(dat, acc_t, (size_t)B * 16));
  CHK(dfr.ensure((size_t)B * S * 2 * T * nfft * 4));
  CHK(to_dev(dout, out_host, no));
  int rc = ht_ispec_launch(e, plan, win.f(), tw.p, env.f(), dx.f(), B, T, S, reinterpret_cast<const double *>(daf.p), n_stat, dfr.f(), dxt.f(),
                           reinterpret_cast<const double *>(dat.p), L, dout.f(), nullptr);
  if (rc == ASX_OK) rc = to_host(out_host, dout, no);
  else (void)hipDeviceSynchronize();
  return rc;
}

// ---- single normalisation / statistics launches ------------------------------------------
static const int64_t OP_NORM_MAX = 1ll << 28;   // floats of the largest tensor a single-op case may hold

// after the launch helpers returned rc: a launch error becomes ASX_ERR_HIP, and a failed case leaves nothing in flight
static int op_norm_done(int rc, const char *what) {
  if (rc == ASX_OK && hipGetLastError() != hipSuccess) {
    set_err("%s: launch failed", what);
    rc = ASX_ERR_HIP;
  }
  if (rc != ASX_OK) (void)hipDeviceSynchronize();
  return rc;
}

int asx_op_rownorm(asx_engine *e, const char *kind, const float *x_host, int64_t M, int32_t d, int64_t lda, const float *gamma_host,
                   const float *beta_host, const float *pos_host, int64_t pos_mod, int32_t in_place, float *y_host, int64_t ldy) {
  REQUIRE(e && kind && x_host && y_host, "asx_op_rownorm: null argument");
  const bool rms = strcmp(kind, "rms") == 0, fac = strcmp(kind, "rms_factor") == 0, ln = strcmp(kind, "layer") == 0;
  REQUIRE(rms || fac || ln, "asx_op_rownorm: unknown kind '%s'", kind);
  REQUIRE(M > 0 && d > 0 && lda >= d && M < OP_NORM_MAX && lda < OP_NORM_MAX && M * lda < OP_NORM_MAX,
          "asx_op_rownorm: m %lld rows of d %d floats in lda %lld", (long long)M, d, (long long)lda);
  if (rms)
    REQUIRE(gamma_host && ldy >= d && ldy < OP_NORM_MAX && M * ldy < OP_NORM_MAX && (!in_place || lda == ldy),
            "asx_op_rownorm(rms): gamma, ldy %lld >= d %d, and lda == ldy in place", (long long)ldy, d);
  if (fac) REQUIRE(!in_place, "asx_op_rownorm(rms_factor): the factors have a buffer of their own");
  if (ln)
    REQUIRE(gamma_host && beta_host && lda == d && ldy == d && !in_place && (!pos_host || (pos_mod >= 1 && pos_mod * d < OP_NORM_MAX)),
            "asx_op_rownorm(layer): gamma, beta, dense rows (lda %lld, ldy %lld, d %d), pos_mod %lld", (long long)lda, (long long)ldy, d,
            (long long)pos_mod);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dx, dy, dg, db, dp;
  BufGuard guard{{&dx, &dy, &dg, &db, &dp}};
  const size_t ny = fac ? (size_t)M : (size_t)(M * ldy);
  CHK(to_dev(dx, x_host, (size_t)(M * lda)));
  if (!fac) CHK(to_dev(dg, gamma_host, (size_t)d));
  if (ln) CHK(to_dev(db, beta_host, (size_t)d));
  if (ln && pos_host) CHK(to_dev(dp, pos_host, (size_t)(pos_mod * d)));
  if (!in_place) CHK(to_dev(dy, y_host, ny));
  DevBuf &out = in_place ? dx : dy;
  int rc;
  if (rms) rc = rof_rmsnorm(e, dx.f(), lda, d, dg.f(), out.f(), ldy, M, nullptr);
  else if (fac) rc = rof_rownorm(e, dx.f(), lda, d, out.f(), M, nullptr);
  else rc = ht_ln(e, dx.f(), d, dg, db, pos_host ? dp.f() : nullptr, pos_host ? pos_mod : 1, out.f(), M, nullptr);
  rc = op_norm_done(rc, "asx_op_rownorm");
  if (rc == ASX_OK) rc = to_host(y_host, out, ny);
  return rc;
}

static int op_acc_to_host(double *h, const DevBuf &d, size_t pairs) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h, d.p, pairs * 16, hipMemcpyDeviceToHost));
  return ASX_OK;
}

int asx_op_group_stats(asx_engine *e, const float *x_host, int32_t G1, int64_t R, int64_t P, int64_t gdiv, int32_t ld, int32_t Cn,
                       int32_t G2, double *acc_host) {
  REQUIRE(e && x_host && acc_host, "asx_op_group_stats: null argument");
  REQUIRE(G1 > 0 && R > 0 && P > 0 && gdiv > 0 && ld > 0 && Cn > 0 && Cn <= ld && G2 > 0, "asx_op_group_stats: sizes must be positive, cn <= ld");
  REQUIRE(R < OP_NORM_MAX && P < OP_NORM_MAX && R * P < OP_NORM_MAX && (int64_t)G1 * R * P < OP_NORM_MAX && (int64_t)G1 * G2 < (1 << 24),
          "asx_op_group_stats: the case is too large for a single-op test");
  REQUIRE((P - 1) / gdiv < G2, "asx_op_group_stats: a plane of %lld floats in groups of %lld does not fit g2 = %d groups", (long long)P,
          (long long)gdiv, G2);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dx, dacc;
  BufGuard guard{{&dx, &dacc}};
  const size_t pairs = (size_t)G1 * G2;
  CHK(to_dev(dx, x_host, (size_t)((int64_t)G1 * R * P)));
  CHK(dacc.ensure(pairs * 16));
  int rc = op_norm_done(ht_stats(e, dx.f(), G1, R, P, gdiv, ld, Cn, G2, reinterpret_cast<double *>(dacc.p), nullptr), "asx_op_group_stats");
  if (rc == ASX_OK) rc = op_acc_to_host(acc_host, dacc, pairs);
  return rc;
}

int asx_op_group_norm(asx_engine *e, const char *family, const asx_group_norm_desc *d, const float *x_host, const float *gamma_host,
                      const float *beta_host, const float *aux_host, const float *mul_host, float *y_host, float *stats_host) {
  REQUIRE(e && family && d && x_host && y_host, "asx_op_group_norm: null argument");
  enum { F_HT, F_HD, F_STD, F_TIME, F_HD_TIME, F_V3, F_MDX, F_N };
  static const char *const names[F_N] = {"ht", "hd", "std", "time", "hd_time", "v3", "mdx"};
  int fam = -1;
  for (int i = 0; i < F_N; ++i)
    if (strcmp(family, names[i]) == 0) fam = i;
  REQUIRE(fam >= 0, "asx_op_group_norm: unknown family '%s'", family);
  const int B = d->b, C = d->c;
  const int64_t R = d->r, P = d->p;
  REQUIRE(B > 0 && B <= 64, "asx_op_group_norm: b %d", B);
  const bool waves = fam == F_TIME || fam == F_HD_TIME, planes = fam == F_V3 || fam == F_MDX;
  if (waves || planes) REQUIRE(P > 0 && P < OP_NORM_MAX, "asx_op_group_norm(%s): p %lld", family, (long long)P);
  if (!waves) REQUIRE(C > 0, "asx_op_group_norm(%s): c %d", family, C);
  if (!waves && !planes) REQUIRE(R > 0 && R < OP_NORM_MAX, "asx_op_group_norm(%s): r %lld", family, (long long)R);
  HIPCHK(hipSetDevice(e->device));
  DevBuf dx, dy, dg, db, da, dm, dacc, dst, dpart;
  BufGuard guard{{&dx, &dy, &dg, &db, &da, &dm, &dacc, &dst, &dpart}};
  DevBuf *out = &dy;
  size_t ny = 0;
  int rc = ASX_OK;
  if (fam == F_HT || fam == F_STD) {
    // in place on x [b, r, c]
    REQUIRE((int64_t)B * R * C < OP_NORM_MAX, "asx_op_group_norm(%s): the case is too large for a single-op test", family);
    if (fam == F_HT) REQUIRE(gamma_host && beta_host, "asx_op_group_norm(ht): gamma and beta");
    else REQUIRE(C % 4 == 0 && R < (1 << 24), "asx_op_group_norm(std): frames of c = 4 F floats, got %d", C);
    ny = (size_t)((int64_t)B * R * C);
    CHK(to_dev(dx, x_host, ny));
    CHK(dacc.ensure((size_t)B * 16));
    out = &dx;
    if (fam == F_HT) {
      CHK(to_dev(dg, gamma_host, (size_t)C));
      CHK(to_dev(db, beta_host, (size_t)C));
      rc = ht_norm_out(e, dx.f(), B, R, C, dg.f(), db.f(), reinterpret_cast<double *>(dacc.p), nullptr);
    } else {
      rc = ht_spec_standardize(e, dx.f(), B, (int)R, C / 4, reinterpret_cast<double *>(dacc.p), nullptr);
    }
  } else if (waves) {
    // x [b, 2, p] -> y [b, p (rounded up to even), 2]
    REQUIRE((int64_t)B * 2 * (P + 1) < OP_NORM_MAX, "asx_op_group_norm(%s): the case is too large for a single-op test", family);
    const int64_t Lp = fam == F_HD_TIME ? (P + 1) & ~(int64_t)1 : P;
    ny = (size_t)((int64_t)B * Lp * 2);
    CHK(to_dev(dx, x_host, (size_t)((int64_t)B * 2 * P)));
    CHK(to_dev(dy, y_host, ny));
    CHK(dacc.ensure((size_t)B * 16));
    rc = fam == F_TIME ? ht_wave_standardize(e, dx.f(), B, P, reinterpret_cast<double *>(dacc.p), dy.f(), nullptr)
                       : hd_wave_standardize(e, dx.f(), B, P, reinterpret_cast<double *>(dacc.p), dy.f(), nullptr);
  } else if (fam == F_HD) {
    const int G = d->g, mode = d->mode;
    const int64_t Rin = d->rin ? d->rin : R, r0 = d->r0;
    REQUIRE(gamma_host && beta_host && G > 0 && mode >= 0 && mode <= 2 && (mode != 1 || C % 2 == 0), "asx_op_group_norm(hd): g %d, mode %d, c %d", G,
            mode, C);
    REQUIRE(r0 >= 0 && Rin < OP_NORM_MAX && r0 + R <= Rin && (int64_t)B * Rin * C < OP_NORM_MAX,
            "asx_op_group_norm(hd): rows %lld .. %lld of %lld", (long long)r0, (long long)(r0 + R), (long long)Rin);
    REQUIRE(!d->in_place || (mode != 1 && Rin == R), "asx_op_group_norm(hd): in place takes mode 0 / 2 and rin == r");
    const int Ce = mode == 1 ? C / 2 : C;
    ny = (size_t)((int64_t)B * R * Ce);
    CHK(to_dev(dx, x_host, (size_t)((int64_t)B * Rin * C)));
    CHK(to_dev(dg, gamma_host, (size_t)C));
    CHK(to_dev(db, beta_host, (size_t)C));
    if (aux_host) CHK(to_dev(da, aux_host, ny));
    if (d->in_place) out = &dx;
    else CHK(to_dev(dy, y_host, ny));
    CHK(dacc.ensure((size_t)B * G * 16));
    rc = hd_group_norm_core(e, dx.f(), B, R, C, G, dg.f(), db.f(), reinterpret_cast<double *>(dacc.p), mode, out->f(), aux_host ? da.f() : nullptr,
                            nullptr, Rin, r0);
  } else if (fam == F_V3) {
    const int norm = d->norm, Ct = d->ctot, c0 = d->c0;
    REQUIRE(v3_norm_valid(norm) && d->act >= V3_ACT_RELU && d->act <= V3_ACT_ELU, "asx_op_group_norm(v3): norm %d, act %d", norm, d->act);
    REQUIRE(c0 >= 0 && Ct >= C && c0 <= Ct - C && (int64_t)Ct * P < OP_NORM_MAX && (int64_t)B * Ct * P < OP_NORM_MAX,
            "asx_op_group_norm(v3): channels %d .. %d of %d", c0, c0 + C, Ct);
    REQUIRE(norm == V3_NORM_NONE || (gamma_host && beta_host), "asx_op_group_norm(v3): gamma and beta");
    const int G = v3_norm_groups(norm);
    REQUIRE(G == 0 || C % G == 0, "asx_op_group_norm(v3): GroupNorm(%d) over %d channels", G, C);
    ny = (size_t)((int64_t)B * C * P);
    CHK(to_dev(dx, x_host, (size_t)((int64_t)B * Ct * P)));
    CHK(to_dev(dy, y_host, ny));
    if (norm != V3_NORM_NONE) {
      CHK(to_dev(dg, gamma_host, (size_t)C));
      CHK(to_dev(db, beta_host, (size_t)C));
    }
    // the workspaces as v3_ensure_workspace sizes them
    if (stats_host) CHK(to_dev(dst, stats_host, (size_t)B * C * 2));
    else CHK(dst.ensure((size_t)B * C * 8));
    if (G > 0) CHK(dpart.ensure((size_t)B * G * V3_GN_MAX_SPLIT * sizeof(double2)));
    rc = v3_norm_act_core(e, norm, d->act, d->alpha, dg.f(), db.f(), dst, dpart, V3View{dx.f() + (int64_t)c0 * P, (int64_t)Ct * P}, C, P, B, dy.f(),
                          nullptr);
  } else {
    REQUIRE(gamma_host && beta_host && (int64_t)C * P < OP_NORM_MAX && (int64_t)B * C * P < OP_NORM_MAX,
            "asx_op_group_norm(mdx): gamma, beta, and a case small enough for a single-op test");
    ny = (size_t)((int64_t)B * C * P);
    CHK(to_dev(dx, x_host, ny));
    CHK(to_dev(dg, gamma_host, (size_t)C));
    CHK(to_dev(db, beta_host, (size_t)C));
    if (aux_host) CHK(to_dev(da, aux_host, ny));
    if (mul_host) CHK(to_dev(dm, mul_host, ny));
    if (d->in_place) out = &dx;
    else CHK(to_dev(dy, y_host, ny));
    CHK(dpart.ensure((size_t)B * C * 16));
    std::swap(e->gn_part, dpart);                      // gn_launch takes its per-plane sums from the engine
    rc = gn_launch(e, dx.f(), B, C, P, dg, db, aux_host ? da.f() : nullptr, mul_host ? dm.f() : nullptr, out->f(), nullptr);
    std::swap(e->gn_part, dpart);
  }
  rc = op_norm_done(rc, "asx_op_group_norm");
  if (rc == ASX_OK) rc = to_host(y_host, *out, ny);
  if (rc == ASX_OK && stats_host && fam == F_V3) rc = to_host(stats_host, dst, (size_t)B * C * 2);
  return rc;
}

// ---- MDXC / TFC-TDF v3 --------------------------------------------------------------
int asx_v3_begin(asx_engine *e, const asx_v3_config *cfg) {
  w3_flush(e);
  REQUIRE(e && cfg, "asx_v3_begin: null argument");
  REQUIRE(cfg->num_channels == 2, "only stereo (num_channels = 2) is supported");
  REQUIRE(cfg->num_subbands >= 1 && e->cfg.dim_f % cfg->num_subbands == 0, "dim_f must be divisible by num_subbands");
  REQUIRE(cfg->num_scales >= 1 && cfg->num_blocks_per_scale >= 1 && cfg->num_channels_model > 0 && cfg->growth >= 0 &&
              cfg->bottleneck_factor >= 1 && cfg->num_targets >= 1,
          "bad TFC-TDF v3 hyper-parameters");
  REQUIRE(v3_norm_valid(cfg->norm), "norm must be None (0), InstanceNorm (1), BatchNorm (2) or 256 + G for GroupNorm(G), got %d",
          cfg->norm);
  REQUIRE(cfg->act == V3_ACT_RELU || cfg->act == V3_ACT_GELU || cfg->act == V3_ACT_ELU,
          "act must be relu (0), gelu (1) or elu (2), got %d", cfg->act);
  const int fs = e->cfg.dim_f / cfg->num_subbands;
  REQUIRE(fs % (1 << cfg->num_scales) == 0 && e->cfg.segment_size % (1 << cfg->num_scales) == 0,
          "dim_f / num_subbands and segment_size must be divisible by 2^num_scales");
  REQUIRE((fs >> cfg->num_scales) % cfg->bottleneck_factor == 0, "bottleneck_factor must divide the deepest dim_f");
  if (!e->v3) e->v3 = new V3Net();
  v3_free(*e->v3);
  e->v3->cfg = *cfg;
  e->v3->begun = true;
  e->v3->ws_batch = 0;
  e->host_tensors.clear();
  e->net_begun = true;   // asx_net_set_tensor() is shared
  return ASX_OK;
}

int asx_v3_commit(asx_engine *e) {
  w3_flush(e);
  REQUIRE(e, "asx_v3_commit: null engine");
  if (!e->v3 || !e->v3->begun) {
    set_err("asx_v3_commit before asx_v3_begin");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  V3Net &n = *e->v3;
  const asx_v3_config &cf = n.cfg;
  const int k = cf.num_subbands, dim_c = k * cf.num_channels * 2;
  int c = cf.num_channels_model, f = e->cfg.dim_f / k;
  n.act_alpha = 1.f;
  if (cf.act == V3_ACT_ELU) {
    const float *al;
    CHK(get_tensor(e, V3_ACT_ALPHA_TENSOR, 1, &al));
    REQUIRE(std::isfinite(*al), "elu alpha must be finite");
    n.act_alpha = *al;
  }
  CHK(v3_load_conv(e, n.first, CK_1X1, "first_conv.weight", dim_c, c, 1));
  n.enc.assign(cf.num_scales, {});
  n.dec.assign(cf.num_scales, {});
  n.ds.assign(cf.num_scales, ConvLayer());
  n.us.assign(cf.num_scales, ConvLayer());
  n.ds_n.assign(cf.num_scales, V3Norm());
  n.us_n.assign(cf.num_scales, V3Norm());
  for (int i = 0; i < cf.num_scales; ++i) {
    const std::string p = "encoder_blocks." + std::to_string(i);
    CHK(v3_load_tfc_tdf(e, n.enc[i], p + ".tfc_tdf", c, c, f));
    CHK(v3_load_norm(e, n.ds_n[i], p + ".downscale.conv.0", c));
    CHK(v3_load_conv(e, n.ds[i], CK_DOWN, p + ".downscale.conv.2.weight", c, c + cf.growth, 4));
    c += cf.growth;
    f /= 2;
  }
  CHK(v3_load_tfc_tdf(e, n.mid, "bottleneck_block", c, c, f));
  for (int i = 0; i < cf.num_scales; ++i) {
    const std::string p = "decoder_blocks." + std::to_string(i);
    CHK(v3_load_norm(e, n.us_n[i], p + ".upscale.conv.0", c));
    CHK(v3_load_conv(e, n.us[i], CK_UP, p + ".upscale.conv.2.weight", c, c - cf.growth, 4));
    c -= cf.growth;
    f *= 2;
    CHK(v3_load_tfc_tdf(e, n.dec[i], p + ".tfc_tdf", 2 * c, c, f));
  }
  CHK(v3_load_conv(e, n.final0, CK_1X1, "final_conv.0.weight", c + dim_c, c, 1));
  CHK(v3_load_conv(e, n.final1, CK_1X1, "final_conv.2.weight", c, cf.num_targets * dim_c, 1));
  e->host_tensors.clear();
  n.ready = true;
  return ASX_OK;
}

double asx_v3_flops(const asx_engine *e, int32_t batch) { return e ? v3_flops(e, batch) : 0.0; }

int asx_v3_forward(asx_engine *e, const float *wave_host, int32_t B, float *out_host) {
  REQUIRE(e && wave_host && out_host && B > 0, "asx_v3_forward: bad argument");
  READY(e->v3, "asx_v3_forward");
  HIPCHK(hipSetDevice(e->device));
  const int64_t C = (int64_t)e->cfg.hop_length * (e->cfg.segment_size - 1);
  const int S = e->v3->cfg.num_targets;
  return host_round_trip(wave_host, (size_t)B * 2 * C, out_host, (size_t)B * S * 2 * C,
                         [&](const float *w, float *out) { return v3_chunks_dev(e, w, nullptr, -1, 0, B, out, nullptr); });
}

int asx_mdxc_plan(const asx_engine *e, int64_t N, int32_t overlap, asx_plan *out) {
  REQUIRE(e && out, "asx_mdxc_plan: null argument");
  MdxcTfcPlan t;                                         // csrc/mdxc_pool_plan.h: the one statement of the arithmetic
  const std::string why = mdxc_tfc_plan(e->cfg.hop_length, e->cfg.segment_size, N, overlap, t);
  REQUIRE(why.empty(), "%s", why.c_str());
  asx_plan p{};
  p.n_samples = N;
  p.chunk_size = t.chunk_size;
  p.step = t.step;                                       // hop_size (mdxc_separator.py:364)
  p.pad = t.pad;
  p.trim = (int32_t)t.front;                             // zeros in front (:371)
  p.gen_size = p.step;
  p.padded_len = t.padded_len;
  p.n_chunks = (int32_t)t.n_chunks;                      // Tensor.unfold (:374)
  p.n_frames = e->cfg.segment_size;
  *out = p;
  return ASX_OK;
}

// ---- BS-Roformer ------------------------------------------------------------------
int asx_rof_begin(asx_engine *e, const asx_rof_config *cfg) {
  w3_flush(e);
  REQUIRE(e && cfg, "asx_rof_begin: null argument");
  REQUIRE(cfg->dim_head == 64, "dim_head must be 64 (got %d)", cfg->dim_head);
  REQUIRE(cfg->dim > 0 && cfg->dim % 4 == 0 && cfg->depth >= 1 && cfg->heads >= 1 && cfg->num_stems >= 1 &&
              cfg->time_depth >= 1 && cfg->freq_depth >= 1 && cfg->mlp_expansion_factor >= 1 &&
              cfg->mask_estimator_depth >= 1 && cfg->n_out >= 1,
          "bad BS-Roformer hyper-parameters");
  REQUIRE(cfg->n_bands >= 2 && cfg->n_bands <= 128, "n_bands must be in [2, 128]");
  int sum = 0;
  for (int j = 0; j < cfg->n_bands; ++j) {
    REQUIRE(cfg->freqs_per_bands[j] >= 1, "freqs_per_bands must be positive");
    sum += cfg->freqs_per_bands[j];
  }
  REQUIRE(e->cfg.dim_f == e->cfg.n_fft / 2 + 1, "dim_f must be n_fft/2 + 1 = %d", e->cfg.n_fft / 2 + 1);
  if (cfg->mel) {
    for (int j = 0; j < cfg->n_bands; ++j) {
      REQUIRE(cfg->band_start[j] >= 0 && cfg->band_start[j] + cfg->freqs_per_bands[j] <= e->cfg.dim_f, "mel band %d out of range", j);
      REQUIRE(j == 0 || (cfg->band_start[j] >= cfg->band_start[j - 1] &&
                         cfg->band_start[j] + cfg->freqs_per_bands[j] >= cfg->band_start[j - 1] + cfg->freqs_per_bands[j - 1]),
              "mel bands must be ordered");
    }
  } else {
    REQUIRE(sum == e->cfg.dim_f, "sum(freqs_per_bands) = %d must equal dim_f = n_fft/2 + 1 = %d", sum, e->cfg.dim_f);
  }
  if (!e->rof) e->rof = new RofNet();
  rof_free(*e->rof);
  RofNet &n = *e->rof;
  n.cfg = *cfg;
  n.band_dim.clear();
  n.band_off.clear();
  n.mask_off.clear();
  int off = 0;
  for (int j = 0; j < cfg->n_bands; ++j) {
    n.band_dim.push_back(4 * cfg->freqs_per_bands[j]);   // 2 (complex) * 2 (stereo) * freqs
    n.band_off.push_back(cfg->mel ? 4 * cfg->band_start[j] : off);
    n.mask_off.push_back(off);
    off += 4 * cfg->freqs_per_bands[j];
  }
  n.W = 4 * e->cfg.dim_f;   // width of the per-frame spectrum vector (f s c)
  n.MW = off;               // width of the concatenated band masks (= W unless the bands overlap)
  n.begun = true;
  e->host_tensors.clear();
  e->net_begun = true;
  return ASX_OK;
}

int asx_rof_commit(asx_engine *e) {
  w3_flush(e);
  REQUIRE(e, "asx_rof_commit: null engine");
  if (!e->rof || !e->rof->begun) {
    set_err("asx_rof_commit before asx_rof_begin");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  RofNet &n = *e->rof;
  const asx_rof_config &c = n.cfg;
  const int T = e->cfg.segment_size, Fb = c.n_bands, D = c.dim;
  n.bs_gamma.assign(Fb, DevBuf());
  n.bs_lin.assign(Fb, RofLin());
  for (int j = 0; j < Fb; ++j) {
    const std::string p = "band_split.to_features." + std::to_string(j);
    CHK(rof_upload(e, n.bs_gamma[j], p + ".0.gamma", n.band_dim[j]));
    CHK(rof_load_lin(e, n.bs_lin[j], p + ".1", D, n.band_dim[j], true));
  }
  n.time_l.assign(c.depth, {});
  n.freq_l.assign(c.depth, {});
  for (int i = 0; i < c.depth; ++i) {
    n.time_l[i].assign(c.time_depth, RofLayer());
    n.freq_l[i].assign(c.freq_depth, RofLayer());
    for (int j = 0; j < c.time_depth; ++j)
      CHK(rof_load_layer(e, n.time_l[i][j], "layers." + std::to_string(i) + ".0.layers." + std::to_string(j), T));
    for (int j = 0; j < c.freq_depth; ++j)
      CHK(rof_load_layer(e, n.freq_l[i][j], "layers." + std::to_string(i) + ".1.layers." + std::to_string(j), Fb));
  }
  if (c.mel) {
    n.tnorm_t.assign(c.depth, DevBuf());
    n.tnorm_f.assign(c.depth, DevBuf());
    for (int i = 0; i < c.depth; ++i) {
      CHK(rof_upload(e, n.tnorm_t[i], "layers." + std::to_string(i) + ".0.norm.gamma", D));
      CHK(rof_upload(e, n.tnorm_f[i], "layers." + std::to_string(i) + ".1.norm.gamma", D));
    }
    // bins -> covering band range (bands are ordered, so the covering set is one run of bands)
    const int F = e->cfg.dim_f;
    std::vector<int> jlo(F, Fb), jhi(F, -1), bst(Fb), mo(Fb);
    for (int j = 0; j < Fb; ++j) {
      bst[j] = c.band_start[j];
      mo[j] = n.mask_off[j];
      for (int f = c.band_start[j]; f < c.band_start[j] + c.freqs_per_bands[j]; ++f) {
        jlo[f] = std::min(jlo[f], j);
        jhi[f] = std::max(jhi[f], j);
      }
    }
    for (int f = 0; f < F; ++f) {
      REQUIRE(jhi[f] >= jlo[f], "all frequencies need to be covered by all bands for now (bin %d is not)", f);
      for (int j = jlo[f]; j <= jhi[f]; ++j)
        REQUIRE(f >= c.band_start[j] && f < c.band_start[j] + c.freqs_per_bands[j], "mel bands covering bin %d are not one run", f);
    }
    auto upi = [&](DevBuf &d, const std::vector<int> &v) -> int {
      CHK(d.ensure(v.size() * 4));
      HIPCHK(hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
      return ASX_OK;
    };
    CHK(upi(n.d_bstart, bst));
    CHK(upi(n.d_moff, mo));
    CHK(upi(n.d_jlo, jlo));
    CHK(upi(n.d_jhi, jhi));
  } else {
    CHK(rof_upload(e, n.final_g, "final_norm.gamma", D));
  }
  const int hid = D * (c.mel ? 4 : c.mlp_expansion_factor);   // mel: MaskEstimator is built with the default factor 4
  const int n_lin = c.mask_estimator_depth + (c.mel ? 1 : 0);  // mel MLP: dims = (in, hidden * depth, out)
  n.mask.assign(c.num_stems, {});
  for (int st = 0; st < c.num_stems; ++st) {
    n.mask[st].assign(Fb, {});
    for (int j = 0; j < Fb; ++j) {
      auto &mlp = n.mask[st][j];
      mlp.assign(n_lin, RofLin());
      int in = D;
      for (int li = 0; li < n_lin; ++li) {
        const int out = (li + 1 == n_lin) ? 2 * n.band_dim[j] : hid;
        CHK(rof_load_lin(e, mlp[li],
                         "mask_estimators." + std::to_string(st) + ".to_freqs." + std::to_string(j) + ".0." +
                             std::to_string(2 * li),
                         out, in, true));
        in = out;
      }
    }
  }
  // Hamming fold window (scipy.signal.windows.hamming(chunk), float64 -> float32, mdxc_separator.py:310)
  const int64_t C = (int64_t)e->cfg.hop_length * (T - 1);
  std::vector<float> w((size_t)C);
  for (int64_t i = 0; i < C; ++i)
    w[i] = (float)(C == 1 ? 1.0 : 0.54 - 0.46 * cos(2.0 * M_PI * (double)i / (double)(C - 1)));
  CHK(n.d_window.ensure((size_t)C * 4));
  HIPCHK(hipMemcpy(n.d_window.p, w.data(), (size_t)C * 4, hipMemcpyHostToDevice));
  e->host_tensors.clear();
  n.ready = true;
  return ASX_OK;
}

double asx_rof_flops(const asx_engine *e, int32_t batch) { return e ? rof_flops(e, batch) : 0.0; }

int asx_rof_forward(asx_engine *e, const float *wave_host, int32_t B, float *out_host) {
  REQUIRE(e && wave_host && out_host && B > 0, "asx_rof_forward: bad argument");
  READY(e->rof, "asx_rof_forward");
  HIPCHK(hipSetDevice(e->device));
  const int64_t C = (int64_t)e->cfg.hop_length * (e->cfg.segment_size - 1);
  const int S = e->rof->cfg.num_stems;
  return host_round_trip(wave_host, (size_t)B * 2 * C, out_host, (size_t)B * S * 2 * C,
                         [&](const float *w, float *out) { return rof_chunks_dev(e, w, nullptr, -1, B, out, nullptr); });
}

int asx_rof_plan(const asx_engine *e, int64_t N, int64_t step, int32_t *n_chunks, int64_t *chunk_size) {
  REQUIRE(e && n_chunks && chunk_size, "asx_rof_plan: null argument");
  const int64_t C = (int64_t)e->cfg.hop_length * (e->cfg.segment_size - 1);
  const std::string why = rof_plan_check(N, C, step);   // csrc/mdxc_pool_plan.h
  REQUIRE(why.empty(), "%s", why.c_str());
  *n_chunks = (int32_t)rof_plan_count(N, step);
  *chunk_size = C;
  return ASX_OK;
}

// ---- MDXCSeparator.demix: the TFC branch (mdxc_separator.py:345-404) and the Roformer branch (:272-343) ------------------------
// Both loops exist once, for a pool of songs: one chunk list over all songs, in song order (MdxcPoolPlan), walked in net passes
// that may straddle songs, then ONE segmented fold.  The single-song calls run a pool of one song.
struct MdxcBranch {             // what the two branches do not share
  bool rof;
  int S, rows;                  // stems per chunk; rows of a song's out (Roformer: n_out, row o reads stem o % S)
  DevBuf &chunk_out, &d_starts;
  int64_t chunk_floats(const MdxcPoolPlan &pp) const { return (int64_t)S * 2 * pp.chunk_size; }
};
static MdxcBranch mdxc_branch(asx_engine *e, bool rof) {
  if (rof) return {true, e->rof->cfg.num_stems, e->rof->cfg.n_out, e->rof->chunk_out, e->rof->d_starts};
  return {false, e->v3->cfg.num_targets, e->v3->cfg.num_targets, e->v3->chunk_out, e->v3->d_starts};
}

static int mdxc_ready(const asx_engine *e, bool rof, const char *fn) {
  if (rof) READY(e->rof, fn);
  else READY(e->v3, fn);
  return ASX_OK;
}

// The pool's tables on the device, from by-value launch arguments in groups of POOL_GROUP songs: per pooled chunk its song's base
// pointer and length (pool_wave / pool_nsong) and its start (d_starts), per song its fold entry (pool_songs) into `chunks`, the
// buffer that holds pooled chunk 0 first.  *blocks: the fold's grid.x.
static int mdxc_pool_tables(asx_engine *e, const char *fn, const MdxcBranch &br, const asx_mdxc_song *songs, const MdxcPoolPlan &pp,
                            const float *chunks, hipStream_t s, int64_t *blocks) {
  const int n = (int)pp.chunk0.size() - 1, nk = pp.total();
  CHK(br.d_starts.ensure((size_t)nk * 8));
  CHK(e->pool_wave.ensure((size_t)nk * 8));
  CHK(e->pool_nsong.ensure((size_t)nk * 8));
  CHK(e->pool_songs.ensure((size_t)n * sizeof(MdxcPoolSong)));
  int64_t blk = 0;
  for (int g0 = 0; g0 < n; g0 += POOL_GROUP) {
    MdxcPoolGroup g{};
    g.n_songs = std::min(POOL_GROUP, n - g0);
    g.song0 = g0;
    for (int i = 0; i < g.n_songs; ++i) {
      const asx_mdxc_song &sg = songs[g0 + i];
      g.mix[i] = sg.mix_dev;
      g.out[i] = sg.out_dev;
      g.n[i] = sg.n_samples;
      g.chunk0[i] = pp.chunk0[g0 + i];
      g.blk0[i] = blk;
      blk += (sg.n_samples + 255) / 256;
    }
    g.chunk0[g.n_songs] = pp.chunk0[g0 + g.n_songs];
    const int nthr = std::max(g.chunk0[g.n_songs] - g.chunk0[0], g.n_songs);
    hipLaunchKernelGGL(mdxc_pool_table_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, s, g, pp.step, pp.chunk_size, br.rof ? 1 : 0,
                       br.chunk_floats(pp), chunks, reinterpret_cast<const float **>(e->pool_wave.p), reinterpret_cast<int64_t *>(e->pool_nsong.p),
                       reinterpret_cast<int64_t *>(br.d_starts.p), reinterpret_cast<MdxcPoolSong *>(e->pool_songs.p));
    HIPCHK(hipGetLastError());
  }
  REQUIRE(blk < ((int64_t)1 << 31), "%s: %lld samples in one pool", fn, (long long)blk * 256);
  *blocks = blk;
  return ASX_OK;
}

// Pooled chunks [j0, j1), j0 < j1, through the net in passes of mdxc_pool_per_pass(j1 - j0, max_batch): chunk j -> dst + (j - j0) * S * 2 * C
static int mdxc_pool_chunks(asx_engine *e, const MdxcBranch &br, const MdxcPoolPlan &pp, int j0, int j1, float *dst, hipStream_t s) {
  const int per = mdxc_pool_per_pass(j1 - j0, e->cfg.max_batch);
  for (int j = j0; j < j1; j += per) {
    const int B = std::min(per, j1 - j);
    const PoolChunks pc{reinterpret_cast<const float *const *>(e->pool_wave.p) + j, reinterpret_cast<const int64_t *>(e->pool_nsong.p) + j};
    const int64_t *starts = reinterpret_cast<const int64_t *>(br.d_starts.p) + j;
    float *out = dst + (size_t)(j - j0) * br.chunk_floats(pp);
    CHK(br.rof ? rof_chunks_dev(e, nullptr, starts, 0, B, out, s, &pc) : v3_chunks_dev(e, nullptr, starts, 0, (int)pp.front, B, out, s, &pc));
  }
  return ASX_OK;
}

// The segmented fold of the chunk buffer the songs' fold entries point into (mdxc_pool_tables) -> every song's out
static int mdxc_pool_fold(asx_engine *e, const MdxcBranch &br, const asx_mdxc_song *songs, const MdxcPoolPlan &pp, int64_t blocks, hipStream_t s) {
  const int n = (int)pp.chunk0.size() - 1;
  const int64_t C = pp.chunk_size;
  double bytes = 4.0 * (double)pp.total() * br.chunk_floats(pp);
  for (int i = 0; i < n; ++i) bytes += 4.0 * br.rows * 2 * (double)songs[i].n_samples;
  const MdxcPoolSong *table = reinterpret_cast<const MdxcPoolSong *>(e->pool_songs.p);
  return timed(e, ASX_PROF_FINALIZE, 0.0, bytes, s, [&]() {
    if (br.rof)
      hipLaunchKernelGGL(roformer_finalize_pool_kernel, dim3((unsigned)blocks, br.rows * 2), dim3(256), 0, s, table, n, br.S, C, pp.step,
                         e->rof->d_window.f());
    else
      hipLaunchKernelGGL(mdxc_finalize_pool_kernel, dim3((unsigned)blocks, br.rows * 2), dim3(256), 0, s, table, n, br.S, C, pp.step, pp.front,
                         (float)pp.overlap);
  });
}

// A planned pool through its whole loop, the chunks in the engine's chunk buffer.  Every buffer is sized before the first launch;
// the call only enqueues work.
static int mdxc_pool_demix(asx_engine *e, const char *fn, bool rof, const asx_mdxc_song *songs, const MdxcPoolPlan &pp, void *stream) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const MdxcBranch br = mdxc_branch(e, rof);
  const int nk = pp.total(), per = mdxc_pool_per_pass(nk, e->cfg.max_batch);
  CHK(rof ? rof_ensure_workspace(e, per) : v3_ensure_workspace(e, per));
  if (!rof && nk % per) CHK(v3_walks_ensure(e, nk % per));   // the last, shorter pass walks its own tables
  CHK(br.chunk_out.ensure((size_t)nk * br.chunk_floats(pp) * 4));
  int64_t blk = 0;
  CHK(mdxc_pool_tables(e, fn, br, songs, pp, br.chunk_out.f(), s, &blk));
  CHK(mdxc_pool_chunks(e, br, pp, 0, nk, br.chunk_out.f(), s));
  return mdxc_pool_fold(e, br, songs, pp, blk, s);
}

// The arguments of a pooled call, all checked on the host before anything is enqueued; `geom`: overlap (TFC) or step (Roformer).
static int mdxc_pool_plan(const char *fn, asx_engine *e, bool rof, const asx_mdxc_song *songs, int32_t n_songs, int64_t geom, MdxcPoolPlan &pp) {
  REQUIRE(e && n_songs >= 0 && (songs || n_songs == 0), "%s: null argument", fn);
  std::vector<int64_t> Ns((size_t)n_songs);
  for (int i = 0; i < n_songs; ++i) {
    REQUIRE(songs[i].mix_dev && songs[i].out_dev, "%s: null pointer in song %d", fn, i);
    REQUIRE(songs[i].n_samples >= 1, "%s: song %d: n_samples must be >= 1", fn, i);
    Ns[i] = songs[i].n_samples;
  }
  CHK(mdxc_ready(e, rof, fn));
  std::string err;
  const bool ok = rof ? mdxc_pool_build_rof(e->cfg.hop_length, e->cfg.segment_size, geom, Ns.data(), n_songs, pp, err)
                      : mdxc_pool_build_tfc(e->cfg.hop_length, e->cfg.segment_size, (int)geom, Ns.data(), n_songs, pp, err);
  REQUIRE(ok, "%s: %s", fn, err.c_str());
  return ASX_OK;
}

int asx_mdxc_demix_batch_dev(asx_engine *e, const asx_mdxc_song *songs, int32_t n_songs, int32_t overlap, void *stream) {
  MdxcPoolPlan pp;
  CHK(mdxc_pool_plan("asx_mdxc_demix_batch_dev", e, false, songs, n_songs, overlap, pp));
  return n_songs ? mdxc_pool_demix(e, "asx_mdxc_demix_batch_dev", false, songs, pp, stream) : ASX_OK;
}

int asx_rof_demix_batch_dev(asx_engine *e, const asx_mdxc_song *songs, int32_t n_songs, int64_t step, void *stream) {
  MdxcPoolPlan pp;
  CHK(mdxc_pool_plan("asx_rof_demix_batch_dev", e, true, songs, n_songs, step, pp));
  return n_songs ? mdxc_pool_demix(e, "asx_rof_demix_batch_dev", true, songs, pp, stream) : ASX_OK;
}

// ---- one song: a pool of one.  `mix` (chunks), `out` (fold) or both (demix) are given; errors name no song ---------------------
static int mdxc_one_plan(const char *fn, asx_engine *e, bool rof, const void *a, const void *b, int64_t N, int64_t geom, MdxcPoolPlan &pp) {
  REQUIRE(e && a && b, "%s: null argument", fn);
  CHK(mdxc_ready(e, rof, fn));
  const std::string why = rof ? mdxc_pool_push_rof(pp, e->cfg.hop_length, e->cfg.segment_size, geom, N)
                              : mdxc_pool_push_tfc(pp, e->cfg.hop_length, e->cfg.segment_size, (int)geom, N);
  REQUIRE(why.empty(), "%s", why.c_str());
  return ASX_OK;
}

// chunks [k0, k1) of the song's loop (mdxc_separator.py:374-392 / :318-336) -> chunk_out [k1-k0, S, 2, chunk]
static int mdxc_one_chunks(const char *fn, asx_engine *e, bool rof, const float *mix, int64_t N, int64_t geom, int32_t k0, int32_t k1,
                           float *chunk_out, void *stream) {
  MdxcPoolPlan pp;
  CHK(mdxc_one_plan(fn, e, rof, mix, chunk_out, N, geom, pp));
  REQUIRE(k0 >= 0 && k0 <= k1 && k1 <= pp.total(), "chunk range [%d, %d) outside [0, %d)", k0, k1, pp.total());
  if (k1 == k0) return ASX_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const MdxcBranch br = mdxc_branch(e, rof);
  const asx_mdxc_song song{mix, nullptr, N};
  int64_t blk = 0;
  CHK(mdxc_pool_tables(e, fn, br, &song, pp, nullptr, s, &blk));
  return mdxc_pool_chunks(e, br, pp, k0, k1, chunk_out, s);
}

// the fold of ALL chunks of the song (mdxc_separator.py:246-255, 394-404 / :310-343): chunk_out [n_chunks, S, 2, chunk] -> out
static int mdxc_one_finalize(const char *fn, asx_engine *e, bool rof, const float *chunk_out, int64_t N, int64_t geom, float *out,
                             void *stream) {
  MdxcPoolPlan pp;
  CHK(mdxc_one_plan(fn, e, rof, chunk_out, out, N, geom, pp));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const MdxcBranch br = mdxc_branch(e, rof);
  const asx_mdxc_song song{nullptr, out, N};
  int64_t blk = 0;
  CHK(mdxc_pool_tables(e, fn, br, &song, pp, chunk_out, s, &blk));
  return mdxc_pool_fold(e, br, &song, pp, blk, s);
}

static int mdxc_one_demix(const char *fn, asx_engine *e, bool rof, const float *mix, int64_t N, int64_t geom, float *out, void *stream) {
  MdxcPoolPlan pp;
  CHK(mdxc_one_plan(fn, e, rof, mix, out, N, geom, pp));
  const asx_mdxc_song song{mix, out, N};
  return mdxc_pool_demix(e, fn, rof, &song, pp, stream);
}

int asx_mdxc_chunks_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t overlap, int32_t k0, int32_t k1, float *chunk_out_dev,
                        void *stream) {
  return mdxc_one_chunks("asx_mdxc_chunks_dev", e, false, mix_dev, N, overlap, k0, k1, chunk_out_dev, stream);
}
int asx_mdxc_finalize_dev(asx_engine *e, const float *chunk_out_dev, int64_t N, int32_t overlap, float *out_dev, void *stream) {
  return mdxc_one_finalize("asx_mdxc_finalize_dev", e, false, chunk_out_dev, N, overlap, out_dev, stream);
}
int asx_mdxc_demix_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t overlap, float *out_dev, void *stream) {
  return mdxc_one_demix("asx_mdxc_demix_dev", e, false, mix_dev, N, overlap, out_dev, stream);
}
int asx_rof_chunks_dev(asx_engine *e, const float *mix_dev, int64_t N, int64_t step, int32_t k0, int32_t k1, float *chunk_out_dev,
                       void *stream) {
  return mdxc_one_chunks("asx_rof_chunks_dev", e, true, mix_dev, N, step, k0, k1, chunk_out_dev, stream);
}
int asx_rof_finalize_dev(asx_engine *e, const float *chunk_out_dev, int64_t N, int64_t step, float *out_dev, void *stream) {
  return mdxc_one_finalize("asx_rof_finalize_dev", e, true, chunk_out_dev, N, step, out_dev, stream);
}
int asx_rof_demix_dev(asx_engine *e, const float *mix_dev, int64_t N, int64_t step, float *out_dev, void *stream) {
  return mdxc_one_demix("asx_rof_demix_dev", e, true, mix_dev, N, step, out_dev, stream);
}

int asx_mdxc_demix(asx_engine *e, const float *mix_host, int64_t N, int32_t overlap, float *out_host) {
  REQUIRE(e && mix_host && out_host, "asx_mdxc_demix: null argument");
  REQUIRE(N >= 1, "n_samples must be >= 1");
  READY(e->v3, "asx_mdxc_demix");
  HIPCHK(hipSetDevice(e->device));
  const int S = e->v3->cfg.num_targets;
  return host_round_trip(mix_host, (size_t)2 * N, out_host, (size_t)S * 2 * N,
                         [&](const float *mix, float *out) { return asx_mdxc_demix_dev(e, mix, N, overlap, out, nullptr); });
}

int asx_rof_demix(asx_engine *e, const float *mix_host, int64_t N, int64_t step, float *out_host) {
  REQUIRE(e && mix_host && out_host, "asx_rof_demix: null argument");
  READY(e->rof, "asx_rof_demix");
  HIPCHK(hipSetDevice(e->device));
  const int n_out = e->rof->cfg.n_out;
  return host_round_trip(mix_host, (size_t)2 * N, out_host, (size_t)n_out * 2 * N,
                         [&](const float *mix, float *out) { return asx_rof_demix_dev(e, mix, N, step, out, nullptr); });
}

// ---- options -----------------------------------------------------------------------
// ---- Demucs v4 ---------------------------------------------------------------------
int asx_ht_begin(asx_engine *e, const asx_ht_config *cfg) {
  w3_flush(e);
  REQUIRE(e && cfg, "asx_ht_begin: null argument");
  REQUIRE(cfg->n_sources >= 1 && cfg->channels >= 4 && cfg->growth >= 1 && cfg->depth >= 1 && cfg->depth <= 8,
          "bad HTDemucs hyper-parameters");
  REQUIRE(cfg->kernel_size == 8 && cfg->stride == 4, "only kernel_size 8 / stride 4 is built (got %d / %d)",
          cfg->kernel_size, cfg->stride);
  REQUIRE(cfg->dconv_depth >= 0 && cfg->dconv_depth <= 4 && cfg->dconv_comp >= 1 && cfg->channels % cfg->dconv_comp == 0,
          "bad DConv hyper-parameters");
  REQUIRE(cfg->nfft >= 64 && cfg->nfft % 8 == 0, "bad nfft %d", cfg->nfft);
  REQUIRE(cfg->t_layers >= 0 && (cfg->t_layers == 0 || (cfg->t_heads >= 1 && cfg->t_hidden >= 4 && cfg->t_hidden % 4 == 0)),
          "bad transformer hyper-parameters");
  REQUIRE(cfg->samplerate > 0 && cfg->segment_samples > 0, "bad samplerate / segment");
  hd_drop_clones(e);
  if (e->hd) hd_free(*e->hd);   // a Demucs v3 net shares e->ht: it is gone with these weights
  if (!e->ht) e->ht = new HtNet();
  ht_free(*e->ht);
  e->ht->cfg = *cfg;
  e->ht->begun = true;
  e->host_tensors.clear();
  e->net_begun = true;
  return ASX_OK;
}

int asx_ht_commit(asx_engine *e) {
  w3_flush(e);
  REQUIRE(e, "asx_ht_commit: null engine");
  if (!e->ht || !e->ht->begun) {
    set_err("asx_ht_commit before asx_ht_begin");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  const int rc = ht_commit(e);
  e->host_tensors.clear();
  return rc;
}

double asx_ht_flops(const asx_engine *e) { return (e && e->ht && e->ht->ready) ? ht_flops(e) : 0.0; }

int asx_ht_forward(asx_engine *e, const float *mix_host, int32_t B, int64_t length, float *out_host) {
  REQUIRE(e && mix_host && out_host && B > 0, "asx_ht_forward: bad argument");
  READY(e->ht, "asx_ht_forward");
  HIPCHK(hipSetDevice(e->device));
  const int64_t TL = e->ht->L[0];
  const int S = e->ht->cfg.n_sources;
  REQUIRE(length >= 1 && length <= TL, "length %lld outside [1, %lld]", (long long)length, (long long)TL);
  DevBuf din, dout;
  BufGuard g{{&din, &dout}};
  CHK(din.ensure((size_t)B * 2 * TL * 4));
  CHK(dout.ensure((size_t)B * S * 2 * TL * 4));
  HIPCHK(hipMemset(din.p, 0, (size_t)B * 2 * TL * 4));
  HIPCHK(hipMemcpy2D(din.p, (size_t)TL * 4, mix_host, (size_t)length * 4, (size_t)length * 4, (size_t)B * 2,
                     hipMemcpyHostToDevice));
  CHK(ht_forward_dev(e, din.f(), B, dout.f(), nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy2D(out_host, (size_t)length * 4, dout.p, (size_t)TL * 4, (size_t)length * 4, (size_t)B * S * 2,
                     hipMemcpyDeviceToHost));
  return ASX_OK;
}

// ---- Demucs v3 (HDemucs) -------------------------------------------------------------
int asx_hd_begin(asx_engine *e, const asx_hd_config *cfg) {
  w3_flush(e);
  REQUIRE(e && cfg, "asx_hd_begin: null argument");
  REQUIRE(cfg->n_sources >= 1 && cfg->channels >= 4 && cfg->growth >= 1 && cfg->depth >= 3 && cfg->depth <= 8, "bad HDemucs hyper-parameters");
  REQUIRE(cfg->kernel_size == 8 && cfg->stride == 4 && cfg->time_stride == 2,
          "only kernel_size 8 / stride 4 / time_stride 2 is built (got %d / %d / %d)", cfg->kernel_size, cfg->stride, cfg->time_stride);
  REQUIRE(cfg->dconv_depth >= 1 && cfg->dconv_depth <= 4 && cfg->dconv_comp >= 1 && cfg->channels % cfg->dconv_comp == 0, "bad DConv hyper-parameters");
  REQUIRE(cfg->norm_starts == cfg->depth - 2 && cfg->dconv_lstm == cfg->depth - 2 && cfg->dconv_attn == cfg->depth - 2,
          "only the default structure (GroupNorm, BLSTM and LocalState on the two innermost levels: norm_starts = dconv_lstm = dconv_attn = depth - 2) "
          "is built");
  REQUIRE(cfg->norm_groups >= 1, "bad norm_groups");
  REQUIRE(cfg->nfft >= 64 && cfg->nfft % 8 == 0, "bad nfft %d", cfg->nfft);
  REQUIRE(cfg->samplerate > 0 && cfg->segment_samples >= 1, "bad samplerate / segment");
  hd_drop_clones(e);
  if (!e->ht) e->ht = new HtNet();
  ht_free(*e->ht);
  if (!e->hd) e->hd = new HdNet();
  hd_free(*e->hd);
  e->hd->cfg = *cfg;
  e->hd->begun = true;
  asx_ht_config &h = e->ht->cfg;
  h = asx_ht_config{};
  h.n_sources = cfg->n_sources;
  h.channels = cfg->channels;
  h.growth = cfg->growth;
  h.nfft = cfg->nfft;
  h.depth = cfg->depth - 2;
  h.kernel_size = cfg->kernel_size;
  h.stride = cfg->stride;
  h.dconv_depth = cfg->dconv_depth;
  h.dconv_comp = cfg->dconv_comp;
  h.samplerate = cfg->samplerate;
  h.segment_samples = cfg->segment_samples;
  h.freq_emb_scale = cfg->freq_emb_scale;
  h.max_batch = cfg->max_batch;
  e->host_tensors.clear();
  e->net_begun = true;
  return ASX_OK;
}

int asx_hd_commit(asx_engine *e) {
  w3_flush(e);
  REQUIRE(e, "asx_hd_commit: null engine");
  if (!e->hd || !e->hd->begun) {
    set_err("asx_hd_commit before asx_hd_begin");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  const int rc = hd_commit(e);
  e->host_tensors.clear();
  return rc;
}

double asx_hd_flops(const asx_engine *e, int64_t length) { return (e && e->hd && e->hd->ready && length > 0) ? hd_flops(e, length) : 0.0; }

int asx_hd_forward(asx_engine *e, const float *mix_host, int32_t B, int64_t length, float *out_host) {
  REQUIRE(e && mix_host && out_host && B > 0 && length > 0, "asx_hd_forward: bad argument");
  READY(e->hd, "asx_hd_forward");
  HIPCHK(hipSetDevice(e->device));
  const int S = e->hd->cfg.n_sources;
  return host_round_trip(mix_host, (size_t)B * 2 * length, out_host, (size_t)B * S * 2 * length, [&](const float *mix, float *out) -> int {
    CHK(hd_forward_dev(e, mix, B, length, out, nullptr));
    HIPCHK(hipDeviceSynchronize());
    return ASX_OK;
  });
}

// ---- Demucs v4 and v3: the apply_model loop ------------------------------------------------------------------------
// One implementation per verb behind asx_ht_* (v3 = false) and asx_hd_* (v3 = true); `fn` is the entry point that was called.
static int demucs_ready(const asx_engine *e, bool v3, const char *fn) {
  if (v3) READY(e->hd, fn);
  else READY(e->ht, fn);
  return ASX_OK;
}

static int demucs_plan(const asx_engine *e, bool v3, const char *fn, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                       int32_t *n_segments, int64_t *segment_samples) {
  REQUIRE(e && n_segments && segment_samples && N >= 2 && shifts >= 0 && (shifts == 0 || offsets), "%s: bad argument", fn);
  CHK(demucs_ready(e, v3, fn));
  ApplyPlan p;
  CHK(apply_plan(apply_net(e, v3), N, shifts, offsets, overlap, p));
  *n_segments = (int32_t)p.starts.size();
  *segment_samples = p.segment;
  return ASX_OK;
}

static int demucs_segments_dev(asx_engine *e, bool v3, const char *fn, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets,
                               double overlap, uint32_t flags, int32_t k0, int32_t k1, float *chunk_out_dev, void *stream) {
  REQUIRE(e && mix_dev && chunk_out_dev && N >= 2 && shifts >= 0 && (shifts == 0 || offsets), "%s: bad argument", fn);
  CHK(demucs_ready(e, v3, fn));
  HIPCHK(hipSetDevice(e->device));
  const ApplyNet a = apply_net(e, v3);
  ApplyPlan p;
  CHK(apply_plan(a, N, shifts, offsets, overlap, p));
  REQUIRE(k0 >= 0 && k0 <= k1 && k1 <= (int)p.starts.size(), "segment range [%d, %d) outside [0, %d)", k0, k1, (int)p.starts.size());
  return a.segments(e, mix_dev, N, p, flags, k0, k1, chunk_out_dev, reinterpret_cast<hipStream_t>(stream));
}

static int demucs_fold_dev(asx_engine *e, bool v3, const char *fn, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets,
                           double overlap, uint32_t flags, const float *chunk_out_dev, float *out_dev, void *stream) {
  REQUIRE(e && mix_dev && chunk_out_dev && out_dev && N >= 2 && shifts >= 0 && (shifts == 0 || offsets), "%s: bad argument", fn);
  CHK(demucs_ready(e, v3, fn));
  HIPCHK(hipSetDevice(e->device));
  const ApplyNet a = apply_net(e, v3);
  ApplyPlan p;
  CHK(apply_plan(a, N, shifts, offsets, overlap, p));
  return apply_fold_dev(e, a, mix_dev, N, p, flags, chunk_out_dev, out_dev, reinterpret_cast<hipStream_t>(stream));
}

static int demucs_demix_dev(asx_engine *e, bool v3, const char *fn, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets,
                            double overlap, uint32_t flags, float *out_dev, void *stream) {
  REQUIRE(e && mix_dev && out_dev && N >= 2, "%s: bad argument", fn);
  REQUIRE(shifts >= 0 && (shifts == 0 || offsets), "shifts > 0 needs the offsets array");
  REQUIRE(overlap >= 0.0 && overlap < 1.0, "overlap must be in [0, 1)");
  CHK(demucs_ready(e, v3, fn));
  HIPCHK(hipSetDevice(e->device));
  return apply_demix_dev(e, apply_net(e, v3), mix_dev, N, shifts, offsets, overlap, flags, out_dev, reinterpret_cast<hipStream_t>(stream));
}

static int demucs_demix_batch_dev(asx_engine *e, bool v3, const char *fn, const asx_apply_song *songs, int32_t n_songs, int32_t shifts,
                                  double overlap, uint32_t flags, void *stream) {
  REQUIRE(e && n_songs >= 0 && (songs || n_songs == 0), "%s: null argument", fn);
  REQUIRE(shifts >= 0, "%s: shifts must be >= 0", fn);
  REQUIRE(overlap >= 0.0 && overlap < 1.0, "overlap must be in [0, 1)");
  CHK(demucs_ready(e, v3, fn));
  if (n_songs == 0) return ASX_OK;
  HIPCHK(hipSetDevice(e->device));
  return apply_demix_pool_dev(e, apply_net(e, v3), songs, n_songs, shifts, overlap, flags, reinterpret_cast<hipStream_t>(stream));
}

static int demucs_demix(asx_engine *e, bool v3, const char *fn, const float *mix_host, int64_t N, int32_t shifts, const int64_t *offsets,
                        double overlap, uint32_t flags, float *out_host) {
  REQUIRE(e && mix_host && out_host && N >= 2, "%s: bad argument", fn);
  CHK(demucs_ready(e, v3, fn));
  HIPCHK(hipSetDevice(e->device));
  const int S = apply_net(e, v3).S;
  return host_round_trip(mix_host, (size_t)2 * N, out_host, (size_t)S * 2 * N, [&](const float *mix, float *out) {
    return demucs_demix_dev(e, v3, fn, mix, N, shifts, offsets, overlap, flags, out, nullptr);
  });
}

int asx_ht_plan(const asx_engine *e, int64_t N, int32_t shifts, const int64_t *offsets, double overlap, int32_t *n_segments,
                int64_t *segment_samples) {
  return demucs_plan(e, false, "asx_ht_plan", N, shifts, offsets, overlap, n_segments, segment_samples);
}
int asx_hd_plan(const asx_engine *e, int64_t N, int32_t shifts, const int64_t *offsets, double overlap, int32_t *n_segments,
                int64_t *segment_samples) {
  return demucs_plan(e, true, "asx_hd_plan", N, shifts, offsets, overlap, n_segments, segment_samples);
}
int asx_ht_segments_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                        uint32_t flags, int32_t k0, int32_t k1, float *chunk_out_dev, void *stream) {
  return demucs_segments_dev(e, false, "asx_ht_segments_dev", mix_dev, N, shifts, offsets, overlap, flags, k0, k1, chunk_out_dev, stream);
}
int asx_hd_segments_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                        uint32_t flags, int32_t k0, int32_t k1, float *chunk_out_dev, void *stream) {
  return demucs_segments_dev(e, true, "asx_hd_segments_dev", mix_dev, N, shifts, offsets, overlap, flags, k0, k1, chunk_out_dev, stream);
}
int asx_ht_fold_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets, double overlap, uint32_t flags,
                    const float *chunk_out_dev, float *out_dev, void *stream) {
  return demucs_fold_dev(e, false, "asx_ht_fold_dev", mix_dev, N, shifts, offsets, overlap, flags, chunk_out_dev, out_dev, stream);
}
int asx_hd_fold_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets, double overlap, uint32_t flags,
                    const float *chunk_out_dev, float *out_dev, void *stream) {
  return demucs_fold_dev(e, true, "asx_hd_fold_dev", mix_dev, N, shifts, offsets, overlap, flags, chunk_out_dev, out_dev, stream);
}
int asx_ht_demix_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                     uint32_t flags, float *out_dev, void *stream) {
  return demucs_demix_dev(e, false, "asx_ht_demix_dev", mix_dev, N, shifts, offsets, overlap, flags, out_dev, stream);
}
int asx_hd_demix_dev(asx_engine *e, const float *mix_dev, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                     uint32_t flags, float *out_dev, void *stream) {
  return demucs_demix_dev(e, true, "asx_hd_demix_dev", mix_dev, N, shifts, offsets, overlap, flags, out_dev, stream);
}
int asx_ht_demix_batch_dev(asx_engine *e, const asx_apply_song *songs, int32_t n_songs, int32_t shifts, double overlap, uint32_t flags,
                           void *stream) {
  return demucs_demix_batch_dev(e, false, "asx_ht_demix_batch_dev", songs, n_songs, shifts, overlap, flags, stream);
}
int asx_hd_demix_batch_dev(asx_engine *e, const asx_apply_song *songs, int32_t n_songs, int32_t shifts, double overlap, uint32_t flags,
                           void *stream) {
  return demucs_demix_batch_dev(e, true, "asx_hd_demix_batch_dev", songs, n_songs, shifts, overlap, flags, stream);
}
int asx_ht_demix(asx_engine *e, const float *mix_host, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                 uint32_t flags, float *out_host) {
  return demucs_demix(e, false, "asx_ht_demix", mix_host, N, shifts, offsets, overlap, flags, out_host);
}
int asx_hd_demix(asx_engine *e, const float *mix_host, int64_t N, int32_t shifts, const int64_t *offsets, double overlap,
                 uint32_t flags, float *out_host) {
  return demucs_demix(e, true, "asx_hd_demix", mix_host, N, shifts, offsets, overlap, flags, out_host);
}

// ---- VR ------------------------------------------------------------------------------
int asx_vr_begin(asx_engine *e, const asx_vr_config *cfg) {
  w3_flush(e);
  REQUIRE(e && cfg, "asx_vr_begin: null argument");
  REQUIRE(cfg->n_bands >= 1 && cfg->n_bands <= 8 && cfg->bins >= 32, "bad band layout");
  REQUIRE(cfg->channel_mode >= 0 && cfg->channel_mode <= 3, "bad channel_mode");
  for (int i = 0; i < (cfg->v51 ? 2 : 5); ++i) REQUIRE(cfg->cap[i] >= 4 && cfg->cap[i] % 4 == 0, "net widths must be multiples of 4");
  REQUIRE(cfg->window_size >= 16 && cfg->offset >= 0, "bad window_size / offset");
  for (int d = 0; d < cfg->n_bands; ++d)
    REQUIRE(cfg->band[d].sr > 0 && cfg->band[d].hl > 0 && cfg->band[d].n_fft >= 8 && cfg->band[d].n_fft % 2 == 0, "band %d: bad sr / hl / n_fft",
            d + 1);
  if (!e->vr) e->vr = new VrNet();
  vr_free(*e->vr);
  e->vr->cfg = *cfg;
  e->vr->begun = true;
  e->host_tensors.clear();
  e->net_begun = true;
  return ASX_OK;
}

int asx_vr_commit(asx_engine *e) {
  w3_flush(e);
  REQUIRE(e, "asx_vr_commit: null engine");
  if (!e->vr || !e->vr->begun) {
    set_err("asx_vr_commit before asx_vr_begin");
    return ASX_ERR_STATE;
  }
  HIPCHK(hipSetDevice(e->device));
  const int rc = vr_commit(e);
  e->host_tensors.clear();
  return rc;
}

double asx_vr_flops(const asx_engine *e) { return (e && e->vr && e->vr->ready) ? vr_flops_patch(e) : 0.0; }

int asx_vr_plan(const asx_engine *e, int64_t n_samples, int32_t *n_frames, int64_t *n_out) {
  REQUIRE(e && n_frames && n_out && n_samples > 0, "asx_vr_plan: bad argument");
  READY(e->vr, "asx_vr_plan");
  int T;
  CHK(vr_plan(*e->vr, n_samples, &T, n_out));
  *n_frames = T;
  return ASX_OK;
}

int asx_vr_forward(asx_engine *e, const float *x_host, int32_t B, float *out_host) {
  REQUIRE(e && x_host && out_host && B > 0, "asx_vr_forward: bad argument");
  READY(e->vr, "asx_vr_forward");
  HIPCHK(hipSetDevice(e->device));
  VrNet &n = *e->vr;
  const int W = n.cfg.window_size;
  const size_t numel = (size_t)B * 2 * n.nb1 * W;
  return host_round_trip(x_host, numel, out_host, numel, [&](const float *x, float *y) -> int {
    CHK(n.cfg.v51 ? vr51_ensure_workspace(e, B) : vr_ensure_workspace(e, B));
    const int64_t P = (int64_t)B * n.max_bin * W;
    hipLaunchKernelGGL(vr_from_nchw_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, nullptr, x, n.nb1, n.max_bin, W, n.ctot, n.b.hc, P);
    HIPCHK(hipGetLastError());
    CHK(n.cfg.v51 ? vr51_net_dev(e, B, nullptr) : vr_net_dev(e, B, nullptr));
    hipLaunchKernelGGL(vr_to_nchw_kernel, dim3((unsigned)((numel + 255) / 256)), dim3(256), 0, nullptr, n.b.mk, n.nb1, n.max_bin, W, y,
                       (int64_t)numel);
    HIPCHK(hipGetLastError());
    return ASX_OK;
  });
}

int asx_vr_analysis(asx_engine *e, const float *wave_host, int64_t n_samples, float *spec_host) {
  REQUIRE(e && wave_host && spec_host && n_samples > 0, "asx_vr_analysis: bad argument");
  READY(e->vr, "asx_vr_analysis");
  HIPCHK(hipSetDevice(e->device));
  VrNet &n = *e->vr;
  int T;
  int64_t n_out;
  CHK(vr_plan(n, n_samples, &T, &n_out));
  DevBuf dw;
  BufGuard g{{&dw}};
  CHK(to_dev(dw, wave_host, (size_t)2 * n_samples));
  CHK(n.X.ensure((size_t)2 * T * n.nb1 * 8));
  CHK(vr_analysis_dev(e, dw.f(), n_samples, VrSongView{reinterpret_cast<float2 *>(n.X.p), nullptr, nullptr, nullptr, T, 0}, nullptr));
  CHK(to_host(spec_host, n.X, (size_t)2 * T * n.nb1 * 2));
  return ASX_OK;
}

int asx_vr_separate_dev(asx_engine *e, const float *wave_dev, int64_t n_samples, const asx_vr_params *params, float *primary_dev,
                        float *secondary_dev, void *stream) {
  REQUIRE(e && wave_dev && params && n_samples > 0, "asx_vr_separate_dev: bad argument");
  READY(e->vr, "asx_vr_separate_dev");
  HIPCHK(hipSetDevice(e->device));
  return vr_separate_dev(e, wave_dev, n_samples, params, primary_dev, secondary_dev, reinterpret_cast<hipStream_t>(stream));
}

int asx_vr_separate_batch_dev(asx_engine *e, const asx_vr_song *songs, int32_t n_songs, const asx_vr_params *params, void *stream) {
  REQUIRE(e && params && n_songs >= 0 && (songs || n_songs == 0), "asx_vr_separate_batch_dev: bad argument");
  READY(e->vr, "asx_vr_separate_batch_dev");
  HIPCHK(hipSetDevice(e->device));
  return vr_separate_pool_dev(e, songs, n_songs, params, reinterpret_cast<hipStream_t>(stream));
}

int asx_vr_separate(asx_engine *e, const float *wave_host, int64_t n_samples, const asx_vr_params *params, float *primary_host,
                    float *secondary_host) {
  REQUIRE(e && wave_host && params && n_samples > 0, "asx_vr_separate: bad argument");
  READY(e->vr, "asx_vr_separate");
  HIPCHK(hipSetDevice(e->device));
  int T;
  int64_t n_out;
  CHK(vr_plan(*e->vr, n_samples, &T, &n_out));
  DevBuf dw, dp, ds;
  BufGuard g{{&dw, &dp, &ds}};
  CHK(to_dev(dw, wave_host, (size_t)2 * n_samples));
  if (primary_host) CHK(dp.ensure((size_t)2 * n_out * 4));
  if (secondary_host) CHK(ds.ensure((size_t)2 * n_out * 4));
  CHK(vr_separate_dev(e, dw.f(), n_samples, params, primary_host ? dp.f() : nullptr, secondary_host ? ds.f() : nullptr, nullptr));
  if (primary_host) CHK(to_host(primary_host, dp, (size_t)2 * n_out));
  if (secondary_host) CHK(to_host(secondary_host, ds, (size_t)2 * n_out));
  return ASX_OK;
}

// launch counters of the bf16 x 6 kernels since the process started (tests assert that the path under test is the one that ran)
int asx_counter(const asx_engine *e, const char *name, int64_t *out) {
  REQUIRE(e && name && out, "asx_counter: null argument");
  const std::string nm(name);
  if (nm == "tdf3_launches") *out = (int64_t)g_tdf3_launches.load();
  else if (nm == "tdf3h_launches") *out = (int64_t)g_tdf3h_launches.load();
  else if (nm == "tdf3s_launches") *out = (int64_t)g_tdf3s_launches.load();
  else if (nm == "attn6s_launches") *out = (int64_t)g_attn6s_launches.load();
  else if (nm == "attn6_launches") *out = (int64_t)g_attn6_launches.load();
  else if (nm == "attn6h_launches") *out = (int64_t)g_attn6h_launches.load();
  else if (nm == "tdf3_gather_launches") *out = (int64_t)g_tdf3_gather_launches.load();
  else if (nm == "wino6_launches") *out = (int64_t)g_wino6_launches.load();
  else if (nm == "wino6h_launches") *out = (int64_t)g_wino6h_launches.load();
  else if (nm == "conv3h_launches") *out = (int64_t)g_conv3h_launches.load();
  else if (nm == "conv3h_fin_launches") *out = (int64_t)g_conv3h_fin_launches.load();
  else if (nm == "conv3h_tiled_launches") *out = (int64_t)g_conv3h_tiled_launches.load();
  else if (nm == "conv3h_merged_dispatches") *out = (int64_t)g_conv3h_merged_dispatches.load();
  else if (nm == "tdf_fused_output_launches") *out = (int64_t)g_tdf_fused_output_launches.load();
  else if (nm == "tdf3_pair_image_launches") *out = (int64_t)g_tdf3ps_launches.load();
  else if (nm == "down6_launches") *out = (int64_t)g_down6_launches.load();
  else if (nm == "up6_launches") *out = (int64_t)g_up6_launches.load();
  else if (nm == "hd_rounds") *out = (int64_t)g_hd_rounds.load();
  else if (nm == "vr_net_passes") *out = (int64_t)g_vr_net_passes.load();
  else if (nm == "v3_net_passes") *out = (int64_t)g_v3_net_passes.load();
  else if (nm == "rof_net_passes") *out = (int64_t)g_rof_net_passes.load();
  else if (nm == "phasefix_launches") *out = (int64_t)g_phasefix_launches.load();
  else if (nm == "flac_block_cycles") *out = (int64_t)e->flac_block_cycles;
  else if (nm == "flac_crc16_cycles") *out = (int64_t)e->flac_crc16_cycles;
  else {
    set_err("asx_counter: unknown counter '%s'", name);
    return ASX_ERR_INVALID;
  }
  return ASX_OK;
}

// debug hook: copy `numel` floats of a named engine workspace buffer to the host (tests / bring-up only)
int asx_debug_trace(uint64_t *host, int64_t n_u64) {
  REQUIRE(host && n_u64 > 0 && n_u64 <= 4096 * 8, "asx_debug_trace: bad argument");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpyFromSymbol(host, HIP_SYMBOL(asx_dbg_trace), (size_t)n_u64 * 8));
  return ASX_OK;
}

int asx_debug_fetch(asx_engine *e, const char *name, float *host, int64_t numel) {
  REQUIRE(e && name && host && numel > 0, "asx_debug_fetch: bad argument");
  HIPCHK(hipSetDevice(e->device));
  const float *src = nullptr;
  const std::string nm(name);
  if (e->vr && e->vr->ws_batch > 0) {
    auto &b = e->vr->b;
    if (nm == "vr.hc") src = b.hc;
    else if (nm == "vr.y2") src = b.y2;
    else if (nm == "vr.y3") src = b.y3;
    else if (nm == "vr.h3") src = b.h3;
    else if (nm == "vr.mk") src = b.mk;
    else if (nm == "vr.cat") src = b.cat;
    else if (nm == "vr.bn") src = b.bn;
    else if (nm == "vr.pool") src = b.pool;
    else if (nm == "vr.pool2") src = b.pool2;
    else if (nm == "vr.tmp") src = b.tmp;
    else if (nm.size() == 5 && nm.compare(0, 3, "vr.") == 0 && nm[4] >= '0' && nm[4] < '0' + (int)b.D.size()) {
      const int i = nm[4] - '0';
      src = nm[3] == 'D' ? b.D[i] : (nm[3] == 'E' ? b.E[i] : (nm[3] == 'O' ? b.O[i] : nullptr));
    }
  }
  if (e->hd && e->hd->ws_batch > 0 && e->ht && nm.compare(0, 3, "hd.") == 0) {
    auto &w = e->hd->b;
    auto &b = e->ht->b;
    const int D = e->hd->D;
    const int i = nm.size() == 7 ? nm[6] - '0' : -1;
    if (nm == "hd.inj") src = w.inj;
    else if (nm == "hd.ya") src = w.ya;
    else if (nm == "hd.yz") src = w.yz;
    else if (nm == "hd.skA") src = w.skA;
    else if (nm == "hd.skZ") src = w.skZ;
    else if (nm == "hd.dAin") src = w.dAin;
    else if (nm == "hd.pre") src = w.pre;
    else if (nm.compare(0, 6, "hd.skf") == 0 && i >= 0 && i < D) src = b.skf[i];
    else if (nm.compare(0, 6, "hd.skt") == 0 && i >= 0 && i < D) src = b.skt[i];
    else if (nm.compare(0, 6, "hd.df_") == 0 && i >= 0 && i <= D) src = b.df[i];
    else if (nm.compare(0, 6, "hd.dt_") == 0 && i >= 0 && i <= D) src = b.dt[i];
  }
  if (!src) {
    set_err("asx_debug_fetch: unknown buffer '%s'", name);
    return ASX_ERR_INVALID;
  }
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, src, (size_t)numel * 4, hipMemcpyDeviceToHost));
  return ASX_OK;
}

// ---- spectral edges ------------------------------------------------------------------
int asx_ensemble(asx_engine *e, const float *waves_host, int32_t K, int64_t N, int32_t algorithm, const double *weights,
                 float *out_host, int64_t *n_out) {
  REQUIRE(e && waves_host && out_host && n_out && N >= 1, "asx_ensemble: bad argument");
  HIPCHK(hipSetDevice(e->device));
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  CHK(c.din.ensure((size_t)K * 2 * N * 4));
  CHK(c.dout.ensure((size_t)2 * N * 4));
  HIPCHK(hipMemcpy(c.din.p, waves_host, (size_t)K * 2 * N * 4, hipMemcpyHostToDevice));
  CHK(ens_ensemble_dev(e, c.din.f(), K, N, algorithm, weights, c.dout.f(), n_out, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_host, c.dout.p, (size_t)2 * (*n_out) * 4, hipMemcpyDeviceToHost));
  return ASX_OK;
}

int asx_ensemble_dev(asx_engine *e, const float *waves_dev, int32_t K, int64_t N, int32_t algorithm, const double *weights,
                     float *out_dev, int64_t *n_out, void *stream) {
  REQUIRE(e && waves_dev && out_dev && n_out && N >= 1, "asx_ensemble_dev: bad argument");
  HIPCHK(hipSetDevice(e->device));
  return ens_ensemble_dev(e, waves_dev, K, N, algorithm, weights, out_dev, n_out, reinterpret_cast<hipStream_t>(stream));
}

// One member stem -> slot k of the [K, 2, n_max] stack asx_ensemble_dev reads, through the member's file round trip
// (write_audio's normalise + int16, librosa.load's / 32768, the Ensembler's zero padding; or the soundfile writer's file of the
// mode's sample format and its decode): ens_slot_kernel.
int asx_ensemble_slot_dev(asx_engine *e, const float *stem_dev, int64_t n, int32_t layout, float max_peak, float min_peak,
                          int32_t has_min, int32_t mode, float *stack_dev, int32_t k, int64_t n_max, float *peak_after, void *stream) {
  REQUIRE(e && stack_dev && (stem_dev || n == 0), "asx_ensemble_slot_dev: bad argument");
  REQUIRE(n >= 0 && n <= n_max && n_max >= 1 && n_max <= ((int64_t)1 << 38) && k >= 0,
          "asx_ensemble_slot_dev: need 0 <= n <= n_max, 1 <= n_max <= 2^38 and k >= 0 (n %lld, n_max %lld, k %d)",
          (long long)n, (long long)n_max, (int)k);
  REQUIRE(layout == ASX_STEM_PLANAR || layout == ASX_STEM_ROWS, "asx_ensemble_slot_dev: layout %d (0 planar [2, n], 1 rows [n, 2])", (int)layout);
  static_assert(ASX_SLOT_PCM16 == ENS_SLOT_PCM16 && ASX_SLOT_FLOAT32 == ENS_SLOT_FLOAT32 && ASX_SLOT_FILE_PCM16 == ENS_SLOT_FILE_PCM16 &&
                    ASX_SLOT_FILE_PCM24 == ENS_SLOT_FILE_PCM24 && ASX_SLOT_FILE_PCM32 == ENS_SLOT_FILE_PCM32 && ASX_SLOT_FILE_FLOAT == ENS_SLOT_FILE_FLOAT &&
                    ASX_SLOT_FILE_PCM16 == PCMENC_S16 && ASX_SLOT_FILE_PCM24 == PCMENC_S24 && ASX_SLOT_FILE_PCM32 == PCMENC_S32 &&
                    ASX_SLOT_FILE_FLOAT == PCMENC_F32, "asx.h, the slot kernel and the PCM encoder disagree");
  REQUIRE(ens_slot_mode_known(mode), "asx_ensemble_slot_dev: mode %d (" ENS_SLOT_MODE_TEXT ")", (int)mode);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(e->d_peak.ensure(256));
  unsigned int *pk = reinterpret_cast<unsigned int *>(e->d_peak.p) + 3;   // its own word (0: separate / pcm16, 1: decode, 2: normalize_dev)
  HIPCHK(hipMemsetAsync(pk, 0, 4, s));
  const int64_t n2 = 2 * n;
  if (n2 > 0) {
    const unsigned nb = (unsigned)std::min<int64_t>((n2 + 255) / 256, 2048);
    CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * n2, s, [&]() { hipLaunchKernelGGL(absmax_kernel, dim3(nb), dim3(256), 0, s, stem_dev, n2, pk); }));
  }
  float *slot = stack_dev + (size_t)k * 2 * (size_t)n_max;
  CHK(timed(e, ASX_PROF_MISC, 0.0, 4.0 * (n2 + 2.0 * n_max), s, [&]() {
    hipLaunchKernelGGL(ens_slot_kernel, dim3((unsigned)((n_max + 255) / 256)), dim3(256), 0, s, stem_dev, n, (int)(layout == ASX_STEM_ROWS), pk,
                       max_peak, min_peak, (int)has_min, (int)mode, slot, n_max);
  }));
  if (peak_after) {
    float maxv = 0.f;
    HIPCHK(hipMemcpyAsync(&maxv, pk, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *peak_after = ens_peak_after(maxv, mode, max_peak, min_peak, has_min);
  }
  return ASX_OK;
}

int asx_ensemble_batch_dev(asx_engine *e, asx_ens_job *jobs, int32_t n_jobs, int32_t algorithm, const double *weights, int32_t n_weights,
                           int32_t mode, float max_peak, float min_peak, int32_t has_min, double silent_below, void *stream) {
  REQUIRE(e, "asx_ensemble_batch_dev: null engine");
  static_assert(ASX_ENS_MAX_K == ENS_MAX_K && ASX_ENS_MAX_K == ENS_PLAN_MAX_K && ASX_ENS_MAX_JOBS == ENS_PLAN_MAX_JOBS, "asx.h and the plan disagree");
  HIPCHK(hipSetDevice(e->device));
  return ens_ensemble_batch_dev(e, "asx_ensemble_batch_dev", jobs, n_jobs, nullptr, algorithm, weights, n_weights, mode, max_peak, min_peak, has_min,
                                silent_below, reinterpret_cast<hipStream_t>(stream));
}

// the same with the slot mode of every contributor: modes [n_jobs][ASX_ENS_MAX_K]
int asx_ensemble_batch_modes_dev(asx_engine *e, asx_ens_job *jobs, int32_t n_jobs, const int32_t *modes, int32_t algorithm, const double *weights,
                                 int32_t n_weights, float max_peak, float min_peak, int32_t has_min, double silent_below, void *stream) {
  REQUIRE(e, "asx_ensemble_batch_modes_dev: null engine");
  REQUIRE(modes || n_jobs <= 0, "asx_ensemble_batch_modes_dev: null modes");
  HIPCHK(hipSetDevice(e->device));
  static const int32_t none[1] = {0};
  return ens_ensemble_batch_dev(e, "asx_ensemble_batch_modes_dev", jobs, n_jobs, modes ? modes : none, algorithm, weights, n_weights, ASX_SLOT_PCM16,
                                max_peak, min_peak, has_min, silent_below, reinterpret_cast<hipStream_t>(stream));
}

int asx_invert_stem(asx_engine *e, const float *mix_host, const float *stem_host, int64_t N, float *out_host, int64_t *n_out) {
  REQUIRE(e && mix_host && stem_host && out_host && n_out && N >= 1, "asx_invert_stem: bad argument");
  HIPCHK(hipSetDevice(e->device));
  CHK(ens_ctx(e));
  EnsCtx &c = *e->ens;
  CHK(c.din.ensure((size_t)2 * N * 4));
  CHK(c.din2.ensure((size_t)2 * N * 4));
  CHK(c.dout.ensure((size_t)2 * N * 4));
  HIPCHK(hipMemcpy(c.din.p, mix_host, (size_t)2 * N * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c.din2.p, stem_host, (size_t)2 * N * 4, hipMemcpyHostToDevice));
  CHK(ens_invert_dev(e, c.din.f(), c.din2.f(), N, c.dout.f(), n_out, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_host, c.dout.p, (size_t)2 * (*n_out) * 4, hipMemcpyDeviceToHost));
  return ASX_OK;
}

int asx_invert_stem_dev(asx_engine *e, const float *mix_dev, const float *stem_dev, int64_t N, int32_t stem_layout, float stem_scale,
                        float *out_dev, int64_t out_capacity, int64_t *n_out, void *stream) {
  REQUIRE(e && n_out, "asx_invert_stem_dev: null engine or n_out");
  HIPCHK(hipSetDevice(e->device));
  return ens_invert_stem_dev(e, mix_dev, stem_dev, N, (int)stem_layout, stem_scale, out_dev, out_capacity, n_out, reinterpret_cast<hipStream_t>(stream));
}

int asx_invert_stem_batch_dev(asx_engine *e, asx_invert_song *songs, int32_t n_songs, float stem_scale, void *stream) {
  REQUIRE(e, "asx_invert_stem_batch_dev: null engine");
  HIPCHK(hipSetDevice(e->device));
  return ens_invert_stem_batch_dev(e, songs, n_songs, stem_scale, reinterpret_cast<hipStream_t>(stream));
}

// ---- BagOfModels combine on the device (every member keeps its own engine / weights; no float stem visits the host) -------
int asx_ht_standardize_dev(asx_engine *e, const float *mix_dev, int64_t N, float *out_dev, void *stream) {
  REQUIRE(e && mix_dev && out_dev && N >= 2, "asx_ht_standardize_dev: bad argument");
  REQUIRE(e->ht != nullptr, "asx_ht_standardize_dev: no Demucs model committed on this engine");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  CHK(ht_ref_stats(e, mix_dev, N, s));
  return timed(e, ASX_PROF_MISC, 0.0, 16.0 * N, s, [&]() {
    hipLaunchKernelGGL(ht_standardize_kernel, dim3((unsigned)((2 * N + 255) / 256)), dim3(256), 0, s, mix_dev, 2 * N, N,
                       reinterpret_cast<const double *>(e->ht->ref_acc.p), out_dev);
  });
}

int asx_ht_bag_accumulate_dev(asx_engine *e, float *est_dev, const float *member_dev, const float *weights, int32_t S, int64_t N,
                              int32_t first, void *stream) {
  REQUIRE(e && est_dev && member_dev && weights && S >= 1 && S <= 16 && N >= 1, "asx_ht_bag_accumulate_dev: bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  BagWeights w{};
  for (int i = 0; i < S; ++i) w.v[i] = weights[i];
  const int64_t per = 2 * N;
  return timed(e, ASX_PROF_MISC, 0.0, 12.0 * S * per, s, [&]() {
    hipLaunchKernelGGL(ht_bag_accumulate_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)S), dim3(256), 0, s, est_dev, member_dev, per, w,
                       (int)first);
  });
}

int asx_ht_bag_finish_dev(asx_engine *e, const float *est_dev, const float *totals, int32_t S, const float *mix_dev, int64_t N,
                          uint32_t flags, float *out_dev, void *stream) {
  REQUIRE(e && est_dev && totals && out_dev && S >= 1 && S <= 16 && N >= 2, "asx_ht_bag_finish_dev: bad argument");
  REQUIRE(est_dev != out_dev, "asx_ht_bag_finish_dev: est and out must be different buffers (the stem swap is not in place)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIPCHK(hipSetDevice(e->device));
  const int standardize = (flags & ASX_HT_STANDARDIZE) ? 1 : 0;
  if (standardize) {
    REQUIRE(e->ht != nullptr && mix_dev != nullptr, "asx_ht_bag_finish_dev: de-standardising needs the mix and a committed Demucs model");
    CHK(ht_ref_stats(e, mix_dev, N, s));
  }
  BagWeights t{};
  for (int i = 0; i < S; ++i) t.v[i] = totals[i];
  const int64_t per = 2 * N;
  return timed(e, ASX_PROF_MISC, 0.0, 8.0 * S * per, s, [&]() {
    hipLaunchKernelGGL(ht_bag_finish_kernel, dim3((unsigned)((per + 255) / 256), (unsigned)S), dim3(256), 0, s, est_dev, per, N, t,
                       standardize ? reinterpret_cast<const double *>(e->ht->ref_acc.p) : nullptr, standardize,
                       (flags & ASX_HT_SWAP01) ? 1 : 0, out_dev);
  });
}

// ---- weighted sums of stems (kernels_mix.h, engine_mix.h) ---------------------------------------------------------------------------
int asx_mixdown_batch_dev(asx_engine *e, const asx_mix_job *jobs, int32_t n_jobs, void *stream) {
  return mix_batch_dev(e, jobs, n_jobs, reinterpret_cast<hipStream_t>(stream));
}

int asx_mixdown(asx_engine *e, const float *const *x_host, const int32_t *layouts, const int64_t *n_samples, const float *weights, int32_t k,
                float *out_host, int32_t out_layout, int64_t n_out) {
  REQUIRE(x_host && layouts && n_samples && weights && out_host, "asx_mixdown: null argument");
  REQUIRE(k >= 1 && k <= ASX_MIX_MAX_K, "asx_mixdown: %d sources (1 .. %d)", (int)k, ASX_MIX_MAX_K);
  REQUIRE(n_out >= 1 && n_out <= ((int64_t)1 << 40), "asx_mixdown: n_out = %lld (1 .. 2^40)", (long long)n_out);
  for (int i = 0; i < k; ++i) {
    REQUIRE(n_samples[i] >= 0 && n_samples[i] <= ((int64_t)1 << 40), "asx_mixdown: source %d has n = %lld (0 .. 2^40)", i, (long long)n_samples[i]);
    REQUIRE(x_host[i] || n_samples[i] == 0, "asx_mixdown: source %d is null with n = %lld", i, (long long)n_samples[i]);
  }
  REQUIRE(e, "asx_mixdown: null engine");
  HIPCHK(hipSetDevice(e->device));
  DevBuf dx[ASX_MIX_MAX_K], dout;
  BufGuard g{{&dx[0], &dx[1], &dx[2], &dx[3], &dx[4], &dx[5], &dx[6], &dx[7], &dout}};
  asx_mix_job job;
  memset(&job, 0, sizeof(job));
  for (int i = 0; i < k; ++i) {
    if (n_samples[i] > 0) CHK(to_dev(dx[i], x_host[i], (size_t)2 * n_samples[i]));
    job.src[i] = asx_mix_src{dx[i].f(), layouts[i], n_samples[i], weights[i]};
  }
  CHK(dout.ensure((size_t)2 * n_out * 4));
  job.k = k;
  job.out = dout.f();
  job.out_layout = out_layout;
  job.n_out = n_out;
  CHK(mix_batch_dev(e, &job, 1, nullptr));
  return to_host(out_host, dout, (size_t)2 * n_out);
}

// ---- phase fix: a target stem's magnitudes on phases blended towards a source stem's (kernels_phasefix.h, engine_phasefix.h) ---------
int asx_phase_fix_batch_dev(asx_engine *e, const asx_phase_job *jobs, int32_t n_jobs, const float *bin_weights, int32_t hop, void *stream) {
  return phase_fix_batch_dev(e, "asx_phase_fix_batch_dev", jobs, n_jobs, bin_weights, (int)hop, false, reinterpret_cast<hipStream_t>(stream));
}

int asx_phase_fix_dev(asx_engine *e, const asx_phase_job *job, const float *bin_weights, int32_t hop, void *stream) {
  REQUIRE(job, "asx_phase_fix_dev: null job");
  return phase_fix_batch_dev(e, "asx_phase_fix_dev", job, 1, bin_weights, (int)hop, true, reinterpret_cast<hipStream_t>(stream));
}

int asx_phase_fix(asx_engine *e, const float *target_host, int32_t target_layout, int64_t n_samples, const float *source_host, int32_t source_layout,
                  int64_t source_n_samples, const float *bin_weights, int32_t hop, float *out_host, int32_t out_layout) {
  REQUIRE(target_host && out_host, "asx_phase_fix: null target or output");
  REQUIRE(n_samples >= 1 && n_samples <= ((int64_t)1 << 38), "asx_phase_fix: n_samples %lld (1 .. 2^38)", (long long)n_samples);
  REQUIRE(source_n_samples >= 0 && source_n_samples <= ((int64_t)1 << 38), "asx_phase_fix: source_n_samples %lld (0 .. 2^38)", (long long)source_n_samples);
  REQUIRE(source_host || source_n_samples == 0, "asx_phase_fix: the source is null with n = %lld", (long long)source_n_samples);
  REQUIRE(e, "asx_phase_fix: null engine");
  HIPCHK(hipSetDevice(e->device));
  DevBuf dt, ds, dout;
  BufGuard g{{&dt, &ds, &dout}};
  CHK(to_dev(dt, target_host, (size_t)2 * n_samples));
  if (source_n_samples > 0) CHK(to_dev(ds, source_host, (size_t)2 * source_n_samples));
  CHK(dout.ensure((size_t)2 * n_samples * 4));
  asx_phase_job job;
  memset(&job, 0, sizeof(job));
  job.target_dev = dt.f();
  job.target_layout = target_layout;
  job.n_samples = n_samples;
  job.source_dev = ds.f();
  job.source_layout = source_layout;
  job.source_n_samples = source_n_samples;
  job.out_dev = dout.f();
  job.out_layout = out_layout;
  CHK(phase_fix_batch_dev(e, "asx_phase_fix", &job, 1, bin_weights, (int)hop, true, nullptr));
  return to_host(out_host, dout, (size_t)2 * n_samples);
}

int asx_set_option(asx_engine *e, const char *key, int32_t value) {
  REQUIRE(e && key, "asx_set_option: null argument");
  const EngineOption *o = find_option("asx_set_option", key);
  if (!o) return ASX_ERR_INVALID;
#ifndef ASX_EXPERIMENTAL_KERNELS
  REQUIRE(!o->refusal || value <= 0 || value == o->shipped, o->refusal, (int)value);
#endif
  e->*o->field = o->norm(value);
  return ASX_OK;
}

int asx_get_option(const asx_engine *e, const char *key, int32_t *value) {
  REQUIRE(e && key && value, "asx_get_option: null argument");
  const EngineOption *o = find_option("asx_get_option", key);
  if (!o) return ASX_ERR_INVALID;
  *value = e->*o->field;
  return ASX_OK;
}

// ---- profiling -------------------------------------------------------------------
int asx_profile_enable(asx_engine *e, int32_t on) {
  REQUIRE(e, "asx_profile_enable: null engine");
  for (auto &r : e->recs) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  e->recs.clear();
  e->prof = on != 0;
  return ASX_OK;
}

int asx_profile_read(asx_engine *e, asx_profile *out) {
  REQUIRE(e && out, "asx_profile_read: null argument");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  memset(out, 0, sizeof(*out));
  const bool dump = knobs().prof_dump;
  for (auto &r : e->recs) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
    if (dump) fprintf(stderr, "asx_prof cls=%d ms=%.4f gflop=%.3f mbytes=%.2f\n", r.cls, ms, r.flops * 1e-9, r.bytes * 1e-6);
    out->launches[r.cls] += 1;
    out->ms[r.cls] += ms;
    out->flops[r.cls] += r.flops;
    out->bytes[r.cls] += r.bytes;
  }
  return ASX_OK;
}

int asx_profile_launches(asx_engine *e, asx_launch_rec *out, int32_t cap, int32_t *n) {
  REQUIRE(e && n && (out || cap == 0), "asx_profile_launches: null argument");
  HIPCHK(hipSetDevice(e->device));
  HIPCHK(hipDeviceSynchronize());
  *n = (int32_t)e->recs.size();
  for (int32_t i = 0; i < *n && i < cap; ++i) {
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e->recs[i].a, e->recs[i].b));
    out[i].cls = e->recs[i].cls | (e->recs[i].nprod << 8);
    out[i].ms = ms;
    out[i].flops = e->recs[i].flops;
    out[i].bytes = e->recs[i].bytes;
  }
  return ASX_OK;
}

}  // extern "C"
