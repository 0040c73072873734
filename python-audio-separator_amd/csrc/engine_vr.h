// VR architecture on the engine: VRSeparator.loading_mix / inference_vr / spec_to_wav
// (architectures/vr_separator.py:255-375), the spec_utils band logic they call and CascadedASPPNet
// (uvr_lib_v5/vr_network/nets.py:95-175, layers.py).  Included by asx.hip (one TU).
//
// One call keeps the state of the songs it separates in the buffers X, M, HE (slabs) and peak, fmin, wgt (slots) of VrNet: the
// single-song call uses them for its one song; asx_vr_separate_batch_dev lays the songs of a pool end to end in them
// (vr_pool_plan.h), so the slabs hold the WHOLE pool at once -- 2 * (bins + 1) * 12 bytes per frame of every song -- and stay
// that large afterwards.  Walking a very large pool in waves is left to the caller.
#pragma once
#include "sinc_pool_plan.h"
#include "vr_pool_plan.h"

struct VrConv {
  HtGemm g;
  int cin_p = 0, cout = 0, k = 1, act = 1;
};
struct VrSep {
  DevBuf dw;     // [9][C]
  VrConv pw;
  int dil = 1;
};
struct VrBase {
  int nin_p = 0, ch = 0, n_enc = 4, nb = 5;
  std::vector<VrConv> enc1, enc2, dec;   // index 0 = level 1
  VrConv aspp1, aspp2, bott;
  std::vector<VrSep> sep;
  std::vector<int> C;                    // channels per level
};
struct VrFilt {
  int up = 1, down = 1, hlen = 0, n_pre_remove = 0;
  DevBuf h32, h64;
  // ASX_VR_RES_SINC_FASTEST (libsamplerate's converter, kernels_vr.h vr_sinc_kernel): no per-ratio filter, one shared table
  int kind = ASX_VR_RES_POLYPHASE;
  double ratio = 1.0;       // float(target_sr) / orig_sr, as librosa forms it
};
struct VrBand {
  asx_vr_band b{};
  FftPlan plan{};
  DevBuf window, tw, gain_syn;
  VrFilt ana, syn;    // ana: band d+1 -> d (float32); syn: band d -> d+1 (float64 accumulate)
};

// VR 5.1 (nets_new.py, layers_new.py)
struct Vr51Lstm {
  VrConv conv;          // 2n -> 1 (padded to 4)
  HtGemm ih, dense;     // [8*hs, nbins] (both directions, b_ih + b_hh), [nbins, 2*hs] with BatchNorm1d folded
  DevBuf whh;           // [2, 4*hs, hs]
  int hs = 0, nbins = 0;
};
struct Vr51Base {
  int nin_p = 0, n = 0;
  VrConv enc1, e1[4], e2[4], aspp1, aspp2, aspp3[3], bott, dec[4];   // dec[0] = dec1 ... dec[3] = dec4
  Vr51Lstm lstm;
};

struct VrNet {
  asx_vr_config cfg{};
  Vr51Base b1l, b1h, b2l, b2h, b3;
  VrConv c1l, c2l;
  struct {
    float *D[4], *T[4], *e5, *o4, *o3, *ol, *hcv, *xs, *xp, *hsq, *ys, *yt;
  } w51{};
  bool begun = false, ready = false;
  VrBase s1l, s1h, s2, s3;
  VrConv br2, br3, outc;
  std::vector<VrBand> band;   // index 0 = band 1
  DevBuf gain_ana;            // [bins + 1]
  int max_bin = 0, nb1 = 0, ctot = 0;
  // workspace
  int ws_batch = 0;
  DevBuf ws;
  struct {
    float *hc, *y2, *y3, *h3, *mk, *pool, *pool2, *tmp, *cat, *bn;
    std::vector<float *> D, E, O;
  } b;
  DevBuf X, M, M2, peak, fmin, wgt, frames, wss, HE, sinc_tab;
  // The pool's merge weights on their way to `wgt`.  The upload is asynchronous and this vector is pageable, so it must not change
  // while a copy may be in flight: it is written only in vr_separate_pool_dev, right after that call has synchronised its stream
  // (the fmin read-back), which also drains the previous pool's upload -- on the SAME stream.  An engine serves one stream at a
  // time (its workspaces are shared anyway); calls on two streams at once are not supported.
  std::vector<float> wgt_host;
  VrPlanCfg plan_cfg;            // what vr_pool_plan.h needs of the committed net (vr_commit)
  std::vector<DevBuf> wav_ana, wav_syn, wav_up;
};

static void vr_free(VrNet &n) {
  auto fc = [](VrConv &c) {
    c.g.w.release();
    c.g.b.release();
    c.g.wh.release();
  };
  for (VrBase *bs : {&n.s1l, &n.s1h, &n.s2, &n.s3}) {
    for (auto *v : {&bs->enc1, &bs->enc2, &bs->dec})
      for (auto &c : *v) fc(c);
    fc(bs->aspp1);
    fc(bs->aspp2);
    fc(bs->bott);
    for (auto &s : bs->sep) {
      s.dw.release();
      fc(s.pw);
    }
    bs->enc1.clear();
    bs->enc2.clear();
    bs->dec.clear();
    bs->sep.clear();
  }
  fc(n.br2);
  fc(n.br3);
  fc(n.outc);
  for (Vr51Base *bs : {&n.b1l, &n.b1h, &n.b2l, &n.b2h, &n.b3}) {
    fc(bs->enc1);
    for (int i = 0; i < 4; ++i) {
      fc(bs->e1[i]);
      fc(bs->e2[i]);
      fc(bs->dec[i]);
    }
    for (int i = 0; i < 3; ++i) fc(bs->aspp3[i]);
    fc(bs->aspp1);
    fc(bs->aspp2);
    fc(bs->bott);
    fc(bs->lstm.conv);
    for (HtGemm *g : {&bs->lstm.ih, &bs->lstm.dense}) {
      g->w.release();
      g->b.release();
    }
    bs->lstm.whh.release();
  }
  fc(n.c1l);
  fc(n.c2l);
  for (auto &b : n.band) {
    for (DevBuf *p : {&b.window, &b.tw, &b.gain_syn, &b.ana.h32, &b.ana.h64, &b.syn.h32, &b.syn.h64}) p->release();
  }
  n.band.clear();
  for (DevBuf *p : {&n.gain_ana, &n.ws, &n.X, &n.M, &n.M2, &n.peak, &n.fmin, &n.wgt, &n.frames, &n.wss, &n.HE}) p->release();
  for (auto *v : {&n.wav_ana, &n.wav_syn, &n.wav_up})
    for (auto &d : *v) d.release();
  n.ready = false;
  n.ws_batch = 0;
}
static void vr_destroy(VrNet *n) {
  vr_free(*n);
  delete n;
}

// Conv2d (no bias) + BatchNorm2d (eval) folded; weight [cout, cin, k, k] with kh on the frequency (outer) axis ->
// W[n][(kh*k + kw) * cin_p + map[ci]];  map: reference input channel -> padded engine channel
static int vr_pack_conv(asx_engine *e, VrConv &c, const std::string &wname, const std::string &bn, int cout, int cin, int k,
                        const std::vector<int> &map, int cin_p, int act, int cout_p = 0) {
  const float *w;
  CHK(get_tensor(e, wname, (int64_t)cout * cin * k * k, &w));
  const float *gam = nullptr, *bet = nullptr, *mu = nullptr, *var = nullptr;
  if (!bn.empty()) {
    CHK(get_tensor(e, bn + ".weight", cout, &gam));
    CHK(get_tensor(e, bn + ".bias", cout, &bet));
    CHK(get_tensor(e, bn + ".running_mean", cout, &mu));
    CHK(get_tensor(e, bn + ".running_var", cout, &var));
  }
  if (!cout_p) cout_p = cout;
  const int K = k * k * cin_p;
  std::vector<float> pw((size_t)cout_p * K, 0.f), pb((size_t)cout_p, 0.f);
  for (int n = 0; n < cout; ++n) {
    double sc = 1.0, sh = 0.0;
    if (gam) {
      sc = (double)gam[n] / sqrt((double)var[n] + 1e-5);
      sh = (double)bet[n] - (double)mu[n] * sc;
    }
    pb[n] = (float)sh;
    for (int ci = 0; ci < cin; ++ci)
      for (int kh = 0; kh < k; ++kh)
        for (int kw = 0; kw < k; ++kw)
          pw[(size_t)n * K + ((size_t)kh * k + kw) * cin_p + map[ci]] = (float)((double)w[(((size_t)n * cin + ci) * k + kh) * k + kw] * sc);
  }
  c.cin_p = cin_p;
  c.cout = cout_p;
  c.k = k;
  c.act = act;
  c.g.n = cout_p;
  c.g.k = K;
  CHK(ht_up(c.g.w, pw));
  CHK(ht_up(c.g.b, pb));
  if (k == 3) CHK(ht_halo_pack(c.g, pw, 9, cin_p));   // stride-1 launches of this layer take the halo-tile kernel
  return ASX_OK;
}

static std::vector<int> vr_ident(int n) {
  std::vector<int> m(n);
  for (int i = 0; i < n; ++i) m[i] = i;
  return m;
}
// [x(2) | rest] -> [x(2) pad(2) | rest]
static std::vector<int> vr_xmap(int n) {
  std::vector<int> m(n);
  for (int i = 0; i < n; ++i) m[i] = i < 2 ? i : i + 2;
  return m;
}

static int vr_load_base(asx_engine *e, VrBase &bs, const std::string &p, int nin, int ch, int arch) {
  bs.n_enc = arch == 129605 ? 5 : 4;
  bs.nb = arch == 129605 ? 6 : ((arch == 537238 || arch == 537227 || arch == 33966) ? 7 : 5);
  bs.ch = ch;
  bs.nin_p = (nin + 3) & ~3;
  REQUIRE(ch % 4 == 0, "VR net width %d must be a multiple of 4", ch);
  bs.C.assign(bs.n_enc, 0);
  bs.enc1.assign(bs.n_enc, VrConv());
  bs.enc2.assign(bs.n_enc, VrConv());
  bs.dec.assign(bs.n_enc, VrConv());
  int cin = nin;
  for (int i = 0; i < bs.n_enc; ++i) {
    const int c = ch << i;
    bs.C[i] = c;
    const std::string en = p + ".enc" + std::to_string(i + 1);
    const int cin_p = i == 0 ? bs.nin_p : cin;
    CHK(vr_pack_conv(e, bs.enc1[i], en + ".conv1.conv.0.weight", en + ".conv1.conv.1", c, cin, 3, (i == 0 && nin == 2) ? vr_xmap(cin) : vr_ident(cin),
                     cin_p, 4));
    CHK(vr_pack_conv(e, bs.enc2[i], en + ".conv2.conv.0.weight", en + ".conv2.conv.1", c, c, 3, vr_ident(c), c, 4));
    const std::string dn = p + ".dec" + std::to_string(i + 1) + ".conv";
    CHK(vr_pack_conv(e, bs.dec[i], dn + ".conv.0.weight", dn + ".conv.1", c, 3 * c, 3, vr_ident(3 * c), 3 * c, 1));
    cin = c;
  }
  const int ca = bs.C.back();
  const std::string a = p + ".aspp";
  CHK(vr_pack_conv(e, bs.aspp1, a + ".conv1.1.conv.0.weight", a + ".conv1.1.conv.1", ca, ca, 1, vr_ident(ca), ca, 1));
  CHK(vr_pack_conv(e, bs.aspp2, a + ".conv2.conv.0.weight", a + ".conv2.conv.1", ca, ca, 1, vr_ident(ca), ca, 1));
  const int dil[5] = {4, 8, 16, 16, 16};
  bs.sep.assign(bs.nb - 2, VrSep());
  for (int j = 0; j < bs.nb - 2; ++j) {
    const std::string s = a + ".conv" + std::to_string(j + 3);
    const float *dw;
    CHK(get_tensor(e, s + ".conv.0.weight", (int64_t)ca * 9, &dw));
    std::vector<float> t((size_t)9 * ca);
    for (int c = 0; c < ca; ++c)
      for (int q = 0; q < 9; ++q) t[(size_t)q * ca + c] = dw[(size_t)c * 9 + q];
    CHK(ht_up(bs.sep[j].dw, t));
    bs.sep[j].dil = dil[j];
    CHK(vr_pack_conv(e, bs.sep[j].pw, s + ".conv.1.weight", s + ".conv.2", ca, ca, 1, vr_ident(ca), ca, 1));
  }
  CHK(vr_pack_conv(e, bs.bott, a + ".bottleneck.0.conv.0.weight", a + ".bottleneck.0.conv.1", 2 * ca, bs.nb * ca, 1,
                   vr_ident(bs.nb * ca), bs.nb * ca, 1));
  return ASX_OK;
}

static double vr_i0(double x) {
  double s = 1.0, t = 1.0;
  const double q = x * x / 4.0;
  for (int k = 1; k < 200; ++k) {
    t *= q / ((double)k * k);
    s += t;
    if (t < 1e-18 * s) break;
  }
  return s;
}

// scipy.signal.resample_poly's filter: firwin(2*half_len + 1, 1/max(up, down), window=("kaiser", 5.0)) * up, left-padded
// with n_pre_pad zeros.  f32: the float32 variant (`.astype(x.dtype)` then `h *= up` in float32) used for float32 input.
static int vr_design_filter(VrFilt &f, int orig_sr, int target_sr) {
  int a = target_sr, b = orig_sr;
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  f.up = target_sr / a;
  f.down = orig_sr / a;
  if (f.up == 1 && f.down == 1) return ASX_OK;
  const int max_rate = std::max(f.up, f.down);
  const double fc = 1.0 / max_rate;
  const int half_len = 10 * max_rate;
  const int nt = 2 * half_len + 1;
  std::vector<double> h(nt);
  const double alpha = 0.5 * (nt - 1);
  double sum = 0.0;
  for (int i = 0; i < nt; ++i) {
    const double m = i - alpha;
    const double x = fc * m;
    const double sinc = x == 0.0 ? 1.0 : sin(M_PI * x) / (M_PI * x);
    const double r = (i - alpha) / alpha;
    const double win = vr_i0(5.0 * sqrt(std::max(0.0, 1.0 - r * r))) / vr_i0(5.0);
    h[i] = fc * sinc * win;
    sum += h[i];
  }
  for (auto &v : h) v /= sum;
  const int n_pre_pad = f.down - half_len % f.down;
  f.n_pre_remove = (half_len + n_pre_pad) / f.down;
  f.hlen = n_pre_pad + nt;
  std::vector<float> h32((size_t)f.hlen, 0.f);
  std::vector<double> h64((size_t)f.hlen, 0.0);
  for (int i = 0; i < nt; ++i) {
    h32[n_pre_pad + i] = (float)h[i] * (float)f.up;
    h64[n_pre_pad + i] = h[i] * (double)f.up;
  }
  CHK(ht_up(f.h32, h32));
  CHK(f.h64.ensure(h64.size() * 8));
  HIPCHK(hipMemcpy(f.h64.p, h64.data(), h64.size() * 8, hipMemcpyHostToDevice));
  return ASX_OK;
}

// Stand-in for libsamplerate's fastest_coeffs.h (2464 floats, increment 128): a Kaiser-windowed sinc sized to the converter's
// documented figures -- 97 dB SNR, 80 % bandwidth -- cutoff midway between the pass-band edge and Nyquist, window reaching
// zero at 2464 / 128 = 19.25 input samples.  float64 design, rounded to float32 like the library's coeff_t (the CPU-side checker
// of the test suite builds the same table).  [0, TL): coefficients; [TL, 2 TL): float differences c[i + 1] - c[i].
static constexpr int VR_SINC_TL = 2464, VR_SINC_INC = 128;
static int vr_sinc_table(DevBuf &buf) {
  std::vector<float> t(2 * (size_t)VR_SINC_TL, 0.f);
  const double half = (double)VR_SINC_TL / VR_SINC_INC, fc = 0.5 * (0.80 + 1.0), beta = 0.1102 * (97.0 - 8.7);
  const double i0b = vr_i0(beta);
  for (int i = 0; i < VR_SINC_TL; ++i) {
    const double x = (double)i / VR_SINC_INC, r = x / half;
    const double a = fc * x;
    const double sinc = a == 0.0 ? 1.0 : sin(M_PI * a) / (M_PI * a);
    t[i] = (float)(fc * sinc * vr_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b);
  }
  for (int i = 0; i + 1 < VR_SINC_TL; ++i) t[VR_SINC_TL + i] = t[i + 1] - t[i];
  return ht_up(buf, t);
}

static int vr51_commit_net(asx_engine *e);
static VrPlanCfg vr_plan_cfg(const VrNet &n);

static int vr_commit(asx_engine *e) {
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  n.nb1 = c.bins + 1;
  n.max_bin = c.bins;          // CascadedASPPNet(n_fft = bins * 2): max_bin = n_fft // 2
  if (c.v51) {
    CHK(vr51_commit_net(e));
  } else {
    const int ch1 = c.cap[0], c2b = c.cap[1], ch2 = c.cap[2], c3b = c.cap[3], ch3 = c.cap[4];
    const int lev = c.arch == 129605 ? 5 : 4;
    REQUIRE(c.bins % (2 << lev) == 0, "bins %d: each half band must halve %d times", c.bins, lev);
    REQUIRE(c.window_size % (1 << lev) == 0 && c.window_size > 2 * c.offset, "window_size %d must be a multiple of %d and exceed 2*offset",
            c.window_size, 1 << lev);
    n.ctot = 4 + ch1 + ch2;
    CHK(vr_load_base(e, n.s1l, "stg1_low_band_net", 2, ch1, c.arch));
    CHK(vr_load_base(e, n.s1h, "stg1_high_band_net", 2, ch1, c.arch));
    CHK(vr_pack_conv(e, n.br2, "stg2_bridge.conv.0.weight", "stg2_bridge.conv.1", c2b, 2 + ch1, 1, vr_xmap(2 + ch1), 4 + ch1, 1));
    CHK(vr_load_base(e, n.s2, "stg2_full_band_net", c2b, ch2, c.arch));
    CHK(vr_pack_conv(e, n.br3, "stg3_bridge.conv.0.weight", "stg3_bridge.conv.1", c3b, 2 + ch1 + ch2, 1, vr_xmap(2 + ch1 + ch2),
                     4 + ch1 + ch2, 1));
    CHK(vr_load_base(e, n.s3, "stg3_full_band_net", c3b, ch3, c.arch));
    CHK(vr_pack_conv(e, n.outc, "out.weight", "", 2, ch3, 1, vr_ident(ch3), ch3, 5, 4));
    REQUIRE(c2b % 4 == 0 && c3b % 4 == 0, "bridge widths must be multiples of 4");
  }
  // bands
  const int NB = c.n_bands;
  n.band.assign(NB, VrBand());
  int off = 0;
  for (int d = 0; d < NB; ++d) {
    VrBand &B = n.band[d];
    B.b = c.band[d];
    REQUIRE(make_plan(B.b.n_fft, &B.plan), "band %d: n_fft/2 = %d must factor into {2,3,5}", d + 1, B.b.n_fft / 2);
    REQUIRE(B.b.crop_start >= 0 && B.b.crop_stop <= B.b.n_fft / 2 + 1 && B.b.crop_start < B.b.crop_stop, "band %d: bad crop", d + 1);
    std::vector<float> w;
    host_window(B.b.n_fft, w);
    CHK(ht_up(B.window, w));
    std::vector<float> tw((size_t)B.b.n_fft * 2);
    for (int j = 0; j < B.b.n_fft; ++j) {
      const double ang = -2.0 * M_PI * (double)j / (double)B.b.n_fft;
      tw[2 * j] = (float)cos(ang);
      tw[2 * j + 1] = (float)sin(ang);
    }
    CHK(ht_up(B.tw, tw));
    // synthesis gains: fft_hp_filter / fft_lp_filter of cmb_spectrogram_to_wave (spec_utils.py:355-388, 411-429)
    const int nbin = B.b.n_fft / 2 + 1;
    std::vector<double> g(nbin, 1.0);
    auto hp = [&](int bs, int be) {   // fft_hp_filter(spec, bs, be)
      double gg = 1.0;
      for (int b = bs; b > be; --b) {
        gg -= 1.0 / (bs - be);
        if (b >= 0 && b < nbin) g[b] *= gg;
      }
      for (int b = 0; b <= be && b < nbin; ++b) g[b] = 0.0;
    };
    auto lp = [&](int bs, int be) {   // fft_lp_filter(spec, bs, be)
      double gg = 1.0;
      for (int b = bs; b < be; ++b) {
        gg -= 1.0 / (be - bs);
        if (b >= 0 && b < nbin) g[b] *= gg;
      }
      for (int b = std::max(be, 0); b < nbin; ++b) g[b] = 0.0;
    };
    // VR 5.1: get_hp_filter_mask / get_lp_filter_mask (spec_utils.py:399-408) instead
    auto hp51 = [&](int bs, int be) {
      for (int b = 0; b < nbin; ++b) {
        double m;
        if (b <= be) m = 0.0;
        else if (b <= bs + 1) m = (bs - be) > 0 ? (double)(b - be - 1) / (double)(bs - be) : 1.0;   // linspace(0, 1, 1 + bs - be)
        else m = 1.0;
        g[b] *= m;
      }
    };
    auto lp51 = [&](int bs, int be) {
      for (int b = 0; b < nbin; ++b) {
        double m;
        if (b < bs - 1) m = 1.0;
        else if (b < be) m = (be - bs) > 0 ? 1.0 - (double)(b - (bs - 1)) / (double)(be - bs) : 0.0;   // linspace(1, 0, be - bs + 1)
        else m = 0.0;
        g[b] *= m;
      }
    };
    if (c.v51) {
      if (d == NB - 1) {
        if (B.b.hpf_start > 0) hp51(B.b.hpf_start, B.b.hpf_stop - 1);
      } else if (d == 0) {
        lp51(B.b.lpf_start, B.b.lpf_stop);
      } else {
        hp51(B.b.hpf_start, B.b.hpf_stop - 1);
        lp51(B.b.lpf_start, B.b.lpf_stop);
      }
    } else if (d == NB - 1) {
      if (B.b.hpf_start > 0) hp(B.b.hpf_start, B.b.hpf_stop - 1);
    } else if (d == 0) {
      lp(B.b.lpf_start, B.b.lpf_stop);
    } else {
      hp(B.b.hpf_start, B.b.hpf_stop - 1);
      lp(B.b.lpf_start, B.b.lpf_stop);
    }
    std::vector<float> gf(g.begin(), g.end());
    CHK(ht_up(B.gain_syn, gf));
    if (d + 1 < NB) {
      CHK(vr_design_filter(B.ana, c.band[d + 1].sr, B.b.sr));
      CHK(vr_design_filter(B.syn, B.b.sr, c.band[d + 1].sr));
      B.ana.kind = B.b.res_type == ASX_VR_RES_SINC_FASTEST ? ASX_VR_RES_SINC_FASTEST : ASX_VR_RES_POLYPHASE;
      B.syn.kind = c.synth_res_type == ASX_VR_RES_SINC_FASTEST ? ASX_VR_RES_SINC_FASTEST : ASX_VR_RES_POLYPHASE;
      B.ana.ratio = (double)B.b.sr / (double)c.band[d + 1].sr;
      B.syn.ratio = (double)c.band[d + 1].sr / (double)B.b.sr;
      if ((B.ana.kind | B.syn.kind) == ASX_VR_RES_SINC_FASTEST && n.sinc_tab.p == nullptr) CHK(vr_sinc_table(n.sinc_tab));
    }
    off += B.b.crop_stop - B.b.crop_start;
  }
  REQUIRE(off <= c.bins, "Too much bins");
  // analysis gains over the combined rows (combine_spectrograms, spec_utils.py:266-279), float32 like complex64 *= float
  {
    std::vector<float> g((size_t)n.nb1, 1.0f);
    if (c.pre_filter_start > 0 && c.v51) {   // spec_c *= get_lp_filter_mask(bins + 1, start, stop) (spec_utils.py:267-268)
      const int bs = c.pre_filter_start, be = c.pre_filter_stop;
      for (int b = 0; b < n.nb1; ++b) {
        if (b < bs - 1) g[b] = 1.f;
        else if (b < be) g[b] = (float)((be - bs) > 0 ? 1.0 - (double)(b - (bs - 1)) / (double)(be - bs) : 0.0);
        else g[b] = 0.f;
      }
    } else if (c.pre_filter_start > 0) {
      if (NB == 1) {
        double gg = 1.0;
        for (int b = c.pre_filter_start; b < c.pre_filter_stop; ++b) {
          gg -= 1.0 / (c.pre_filter_stop - c.pre_filter_start);
          if (b < n.nb1) g[b] = (float)gg;
        }
        for (int b = c.pre_filter_stop; b < n.nb1; ++b) g[b] = 0.f;
      } else {
        double gp = 1.0;
        for (int b = c.pre_filter_start + 1; b < c.pre_filter_stop; ++b) {
          const double gg = pow(10.0, -(b - c.pre_filter_start) * (3.5 - gp) / 20.0);
          gp = gg;
          if (b < n.nb1) g[b] = (float)gg;
        }
      }
    }
    CHK(ht_up(n.gain_ana, g));
  }
  int max_lds_f = 0, max_lds_i = 0;
  for (auto &B : n.band) {
    max_lds_f = std::max(max_lds_f, (int)stft_lds(B.plan));
    max_lds_i = std::max(max_lds_i, (int)istft_lds(B.plan));
  }
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&vr_stft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds_f);
  (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&vr_istft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_lds_i);
  n.plan_cfg = vr_plan_cfg(n);
  n.ready = true;
  return ASX_OK;
}

// ---- net ----------------------------------------------------------------------------------------------------------
static int vr_conv(asx_engine *e, const VrConv &c, const float *x, int ldc, int64_t x_bs, int B, int H, int W, int stride, float *y,
                   int ldy, int64_t y_bs, hipStream_t s, int dil_o = 1, int dil_i = 1) {
  HtGeom g;
  g.O = H;
  g.I = W;
  g.Cin = c.cin_p;
  g.ldc = ldc;
  g.KO = c.k;
  g.KI = c.k;
  g.DO = dil_o;
  g.DI = dil_i;
  g.PO = (c.k / 2) * dil_o;
  g.PI = (c.k / 2) * dil_i;
  g.SO = stride;
  g.SI = stride;
  g.OR = H / stride;
  g.IR = W / stride;
  g.x_bs = x_bs;
  g.y_bs = y_bs;
  return ht_gg(e, c.g, x, g, (int64_t)B * g.OR, y, ldy, GG_DENSE, c.act, nullptr, 0, 0, 0, 0, s);
}

template <class K, class... A>
static int vr_ew(asx_engine *e, hipStream_t s, int64_t total, double bytes, K kern, A... args) {
  return timed(e, ASX_PROF_MISC, 0.0, bytes, s, [&]() {
    hipLaunchKernelGGL(kern, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, args..., total);
  });
}

// BaseASPPNet.__call__ (nets.py:46-62): x view [B, H, W, nin_p] -> y view [B, H, W, ch]
static int vr_base(asx_engine *e, const VrBase &bs, const float *x, int x_ld, int64_t x_bs, int B, int H, int W, float *y, int y_ld,
                   int64_t y_bs, hipStream_t s) {
  VrNet &n = *e->vr;
  auto &b = n.b;
  const int L = bs.n_enc;
  const float *in = x;
  int in_ld = x_ld;
  int64_t in_bs = x_bs;
  int h = H, w = W;
  for (int i = 0; i < L; ++i) {
    const int c = bs.C[i];
    float *D = b.D[i];
    CHK(vr_conv(e, bs.enc1[i], in, in_ld, in_bs, B, h, w, 1, D + 2 * c, 3 * c, 0, s));       // skip -> its slot of the decoder concat
    CHK(vr_conv(e, bs.enc2[i], D + 2 * c, 3 * c, (int64_t)h * w * 3 * c, B, h, w, 2, b.E[i], c, 0, s));
    in = b.E[i];
    in_ld = c;
    in_bs = 0;
    h /= 2;
    w /= 2;
  }
  const int ca = bs.C[L - 1];
  const float *E = b.E[L - 1];
  const int catc = bs.nb * ca;
  // ASPP (layers.py:254-288)
  CHK(vr_ew(e, s, (int64_t)B * w * ca, 4.0 * B * h * w * ca, vr_rowmean_kernel, E, h, w, ca, b.pool));
  CHK(vr_conv(e, bs.aspp1, b.pool, ca, 0, B, 1, w, 1, b.pool2, ca, 0, s));
  CHK(vr_ew(e, s, (int64_t)B * h * w * ca, 4.0 * B * h * w * ca, vr_bcast_rows_kernel, (const float *)b.pool2, h, w, ca, b.cat, catc));
  CHK(vr_conv(e, bs.aspp2, E, ca, 0, B, h, w, 1, b.cat + ca, catc, 0, s));
  for (size_t j = 0; j < bs.sep.size(); ++j) {
    CHK(vr_ew(e, s, (int64_t)B * h * w * ca, 8.0 * B * h * w * ca, vr_dwconv_kernel, E, h, w, ca, bs.sep[j].dil, (const float *)bs.sep[j].dw.f(),
              b.tmp));
    CHK(vr_conv(e, bs.sep[j].pw, b.tmp, ca, 0, B, h, w, 1, b.cat + (2 + j) * ca, catc, 0, s));
  }
  CHK(vr_conv(e, bs.bott, b.cat, catc, 0, B, h, w, 1, b.bn, 2 * ca, 0, s));
  const float *prev = b.bn;
  for (int i = L - 1; i >= 0; --i) {
    const int c = bs.C[i];
    float *D = b.D[i];
    CHK(vr_ew(e, s, (int64_t)B * 2 * h * 2 * w * (2 * c / 4), 4.0 * B * 5.0 * h * w * 2 * c, vr_upsample2x_kernel, prev, h, w, 2 * c, 2 * c, D, 3 * c));
    h *= 2;
    w *= 2;
    if (i > 0) {
      CHK(vr_conv(e, bs.dec[i], D, 3 * c, 0, B, h, w, 1, b.O[i], c, 0, s));
      prev = b.O[i];
    } else {
      CHK(vr_conv(e, bs.dec[i], D, 3 * c, 0, B, h, w, 1, y, y_ld, y_bs, s));
    }
  }
  return ASX_OK;
}

static int vr_ensure_workspace(asx_engine *e, int B) {
  VrNet &n = *e->vr;
  if (B <= n.ws_batch) return ASX_OK;
  const asx_vr_config &c = n.cfg;
  const size_t P = (size_t)B * n.max_bin * c.window_size;   // positions at full resolution
  size_t off = 0;
  std::vector<std::pair<float **, size_t>> plan;
  auto want = [&](float *&p, size_t floats) {
    plan.push_back({&p, off});
    off += (floats * 4 + 255) & ~(size_t)255;
  };
  auto &b = n.b;
  const int chmax = std::max(std::max(c.cap[0], c.cap[2]), c.cap[4]);
  const int L = c.arch == 129605 ? 5 : 4;
  want(b.hc, P * n.ctot);
  want(b.y2, P * c.cap[1]);
  want(b.y3, P * c.cap[3]);
  want(b.h3, P * c.cap[4]);
  want(b.mk, P * 4);
  b.D.assign(L, nullptr);
  b.E.assign(L, nullptr);
  b.O.assign(L, nullptr);
  for (int i = 0; i < L; ++i) {
    const size_t pi = P >> (2 * i);
    want(b.D[i], pi * 3 * ((size_t)chmax << i));
    want(b.E[i], (pi / 4) * ((size_t)chmax << i));
    want(b.O[i], pi * ((size_t)chmax << i));
  }
  const size_t pa = P >> (2 * L);
  const size_t ca = (size_t)chmax << (L - 1);
  want(b.pool, (size_t)B * c.window_size * ca);
  want(b.pool2, (size_t)B * c.window_size * ca);
  want(b.tmp, pa * ca);
  want(b.cat, pa * ca * 7);
  want(b.bn, pa * 2 * ca);
  CHK(n.ws.ensure(off));
  for (auto &pr : plan) *pr.first = reinterpret_cast<float *>(reinterpret_cast<char *>(n.ws.p) + pr.second);
  n.ws_batch = B;
  return ASX_OK;
}

static std::atomic<long long> g_vr_net_passes{0};   // calls of vr_net_dev / vr51_net_dev since the process started (asx_counter "vr_net_passes")

// CascadedASPPNet.forward (nets.py:132-161) on B patches already in hc[..., 0:4]; result (sigmoid mask) in b.mk [B, max_bin, W, 4]
static int vr_net_dev(asx_engine *e, int B, hipStream_t s) {
  g_vr_net_passes.fetch_add(1);
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  auto &b = n.b;
  const int F = n.max_bin, W = c.window_size, ct = n.ctot, ch1 = c.cap[0];
  const int bw = F / 2;
  const int64_t hc_bs = (int64_t)F * W * ct;
  CHK(vr_base(e, n.s1l, b.hc, ct, hc_bs, B, bw, W, b.hc + 4, ct, hc_bs, s));
  CHK(vr_base(e, n.s1h, b.hc + (int64_t)bw * W * ct, ct, hc_bs, B, bw, W, b.hc + (int64_t)bw * W * ct + 4, ct, hc_bs, s));
  CHK(vr_conv(e, n.br2, b.hc, ct, 0, B, F, W, 1, b.y2, c.cap[1], 0, s));
  CHK(vr_base(e, n.s2, b.y2, c.cap[1], 0, B, F, W, b.hc + 4 + ch1, ct, hc_bs, s));
  CHK(vr_conv(e, n.br3, b.hc, ct, 0, B, F, W, 1, b.y3, c.cap[3], 0, s));
  CHK(vr_base(e, n.s3, b.y3, c.cap[3], 0, B, F, W, b.h3, c.cap[4], 0, s));
  return vr_conv(e, n.outc, b.h3, c.cap[4], 0, B, F, W, 1, b.mk, 4, 0, s);
}


// ---- VR 5.1 --------------------------------------------------------------------------------------------------------
static int vr51_load_base(asx_engine *e, Vr51Base &bs, const std::string &p, int nin, int n, int nbins, int nout_lstm) {
  bs.n = n;
  bs.nin_p = nin == 2 ? 4 : nin + 2;     // [x(2) pad(2) | rest]
  REQUIRE(n % 4 == 0 && nbins % 4 == 0 && nout_lstm % 2 == 0, "VR 5.1 widths must be multiples of 4 (n=%d, lstm bins=%d)", n, nbins);
  const int cw[5] = {n, 2 * n, 4 * n, 6 * n, 8 * n};
  CHK(vr_pack_conv(e, bs.enc1, p + ".enc1.conv.0.weight", p + ".enc1.conv.1", n, nin, 3, vr_xmap(nin), bs.nin_p, 1));
  for (int i = 0; i < 4; ++i) {
    const std::string en = p + ".enc" + std::to_string(i + 2);
    CHK(vr_pack_conv(e, bs.e1[i], en + ".conv1.conv.0.weight", en + ".conv1.conv.1", cw[i + 1], cw[i], 3, vr_ident(cw[i]), cw[i], 4));
    CHK(vr_pack_conv(e, bs.e2[i], en + ".conv2.conv.0.weight", en + ".conv2.conv.1", cw[i + 1], cw[i + 1], 3, vr_ident(cw[i + 1]), cw[i + 1], 4));
  }
  const int ca = cw[4];
  const std::string a = p + ".aspp";
  CHK(vr_pack_conv(e, bs.aspp1, a + ".conv1.1.conv.0.weight", a + ".conv1.1.conv.1", ca, ca, 1, vr_ident(ca), ca, 1));
  CHK(vr_pack_conv(e, bs.aspp2, a + ".conv2.conv.0.weight", a + ".conv2.conv.1", ca, ca, 1, vr_ident(ca), ca, 1));
  for (int j = 0; j < 3; ++j) {
    const std::string c = a + ".conv" + std::to_string(j + 3);
    CHK(vr_pack_conv(e, bs.aspp3[j], c + ".conv.0.weight", c + ".conv.1", ca, ca, 3, vr_ident(ca), ca, 1));
  }
  CHK(vr_pack_conv(e, bs.bott, a + ".bottleneck.conv.0.weight", a + ".bottleneck.conv.1", ca, 5 * ca, 1, vr_ident(5 * ca), 5 * ca, 1));
  // decoders: input = [upsampled | skip]
  for (int i = 3; i >= 1; --i) {   // dec4, dec3, dec2
    const std::string dn = p + ".dec" + std::to_string(i + 1) + ".conv1";
    const int cin = cw[i + 1] + cw[i];
    CHK(vr_pack_conv(e, bs.dec[i], dn + ".conv.0.weight", dn + ".conv.1", cw[i], cin, 3, vr_ident(cin), cin, 1));
  }
  {   // dec1: [dec2 out (2n) | lstm (1) pad (3) | enc1 (n)]
    const int cin = 3 * n + 1;
    std::vector<int> m(cin);
    for (int c = 0; c < cin; ++c) m[c] = c <= 2 * n ? c : c + 3;
    CHK(vr_pack_conv(e, bs.dec[0], p + ".dec1.conv1.conv.0.weight", p + ".dec1.conv1.conv.1", n, cin, 3, m, 3 * n + 4, 1));
  }
  // LSTMModule
  Vr51Lstm &L = bs.lstm;
  L.hs = nout_lstm / 2;
  L.nbins = nbins;
  REQUIRE(L.hs == 4 || L.hs == 8 || L.hs == 16 || L.hs == 32 || L.hs == 64 || L.hs == 128, "LSTM hidden size %d per direction is not built", L.hs);
  const std::string lp = p + ".lstm_dec2";
  CHK(vr_pack_conv(e, L.conv, lp + ".conv.conv.0.weight", lp + ".conv.conv.1", 1, 2 * n, 1, vr_ident(2 * n), 2 * n, 1, 4));
  {
    const int hs = L.hs, G = 4 * hs;
    std::vector<float> wih((size_t)2 * G * nbins), bih((size_t)2 * G), whh((size_t)2 * G * hs);
    const char *sfx[2] = {"", "_reverse"};
    for (int d = 0; d < 2; ++d) {
      const float *wi, *wh, *bi, *bh;
      CHK(get_tensor(e, lp + ".lstm.weight_ih_l0" + sfx[d], (int64_t)G * nbins, &wi));
      CHK(get_tensor(e, lp + ".lstm.weight_hh_l0" + sfx[d], (int64_t)G * hs, &wh));
      CHK(get_tensor(e, lp + ".lstm.bias_ih_l0" + sfx[d], G, &bi));
      CHK(get_tensor(e, lp + ".lstm.bias_hh_l0" + sfx[d], G, &bh));
      std::copy(wi, wi + (size_t)G * nbins, wih.begin() + (size_t)d * G * nbins);
      std::copy(wh, wh + (size_t)G * hs, whh.begin() + (size_t)d * G * hs);
      for (int g = 0; g < G; ++g) bih[(size_t)d * G + g] = bi[g] + bh[g];
    }
    L.ih.n = 2 * G;
    L.ih.k = nbins;
    CHK(ht_up(L.ih.w, wih));
    CHK(ht_up(L.ih.b, bih));
    CHK(ht_up(L.whh, whh));
    const float *dw, *db, *gam, *bet, *mu, *var;
    CHK(get_tensor(e, lp + ".dense.0.weight", (int64_t)nbins * 2 * hs, &dw));
    CHK(get_tensor(e, lp + ".dense.0.bias", nbins, &db));
    CHK(get_tensor(e, lp + ".dense.1.weight", nbins, &gam));
    CHK(get_tensor(e, lp + ".dense.1.bias", nbins, &bet));
    CHK(get_tensor(e, lp + ".dense.1.running_mean", nbins, &mu));
    CHK(get_tensor(e, lp + ".dense.1.running_var", nbins, &var));
    std::vector<float> w2((size_t)nbins * 2 * hs), b2((size_t)nbins);
    for (int r = 0; r < nbins; ++r) {
      const double sc = (double)gam[r] / sqrt((double)var[r] + 1e-5);
      b2[r] = (float)(((double)db[r] - (double)mu[r]) * sc + (double)bet[r]);
      for (int k = 0; k < 2 * hs; ++k) w2[(size_t)r * 2 * hs + k] = (float)((double)dw[(size_t)r * 2 * hs + k] * sc);
    }
    L.dense.n = nbins;
    L.dense.k = 2 * hs;
    CHK(ht_up(L.dense.w, w2));
    CHK(ht_up(L.dense.b, b2));
  }
  return ASX_OK;
}

static int vr51_commit_net(asx_engine *e) {
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  const int no = c.arch == 218409 ? 64 : c.cap[0];   // nets_new.py:103
  const int nl = c.cap[1];
  REQUIRE(no % 16 == 0, "VR 5.1 nout %d must be a multiple of 16", no);
  REQUIRE(c.bins % 32 == 0 && c.window_size % 16 == 0 && c.window_size > 2 * c.offset, "bins %d / window_size %d do not halve 4 times", c.bins,
          c.window_size);
  const int nin_lstm = n.max_bin / 2;
  n.ctot = 4 + no / 4 + no / 2;
  CHK(vr51_load_base(e, n.b1l, "stg1_low_band_net.0", 2, no / 2, nin_lstm / 2, nl));
  CHK(vr_pack_conv(e, n.c1l, "stg1_low_band_net.1.conv.0.weight", "stg1_low_band_net.1.conv.1", no / 4, no / 2, 1, vr_ident(no / 2), no / 2, 1));
  CHK(vr51_load_base(e, n.b1h, "stg1_high_band_net", 2, no / 4, nin_lstm / 2, nl / 2));
  CHK(vr51_load_base(e, n.b2l, "stg2_low_band_net.0", no / 4 + 2, no, nin_lstm / 2, nl));
  CHK(vr_pack_conv(e, n.c2l, "stg2_low_band_net.1.conv.0.weight", "stg2_low_band_net.1.conv.1", no / 2, no, 1, vr_ident(no), no, 1));
  CHK(vr51_load_base(e, n.b2h, "stg2_high_band_net", no / 4 + 2, no / 2, nin_lstm / 2, nl / 2));
  CHK(vr51_load_base(e, n.b3, "stg3_full_band_net", 3 * no / 4 + 2, no, nin_lstm, nl));
  CHK(vr_pack_conv(e, n.outc, "out.weight", "", 2, no, 1, vr_ident(no), no, 5, 4));
  return ASX_OK;
}

template <int HS>
static void vr51_launch_lstm(const float *xp, const float *whh, int W, int B, float *out, hipStream_t s) {
  hipLaunchKernelGGL((vr_lstm_seq_kernel<HS>), dim3((unsigned)B, 2), dim3(4 * HS), 0, s, xp, whh, W, B, out);
}

// the recurrence of the LSTMModule: vr_lstm_seq_kernel<hs> over xp [W, B, 2, 4 * hs], whh [2, 4 * hs, hs] into out [W, B, 2 * hs]
// (vr51_base below and the single-op hook asx_op_vr_lstm)
static int vr51_lstm(asx_engine *e, int hs, const float *xp, const float *whh, int W, int B, float *out, hipStream_t s) {
  REQUIRE(hs == 4 || hs == 8 || hs == 16 || hs == 32 || hs == 64 || hs == 128, "LSTM hidden size %d per direction is not built", hs);
  REQUIRE(W > 0 && B > 0, "LSTM over %d frames of %d sequences", W, B);
  return timed(e, ASX_PROF_MISC, 0.0, 4.0 * W * B * 10.0 * hs, s, [&]() {
    switch (hs) {
      case 4: vr51_launch_lstm<4>(xp, whh, W, B, out, s); break;
      case 8: vr51_launch_lstm<8>(xp, whh, W, B, out, s); break;
      case 16: vr51_launch_lstm<16>(xp, whh, W, B, out, s); break;
      case 32: vr51_launch_lstm<32>(xp, whh, W, B, out, s); break;
      case 64: vr51_launch_lstm<64>(xp, whh, W, B, out, s); break;
      default: vr51_launch_lstm<128>(xp, whh, W, B, out, s); break;
    }
  });
}

// BaseNet.__call__ (nets_new.py:40-56): x view [B, H, W, nin_p] -> y view [B, H, W, n]
static int vr51_base(asx_engine *e, const Vr51Base &bs, const float *x, int x_ld, int64_t x_bs, int B, int H, int W, float *y, int y_ld,
                     int64_t y_bs, hipStream_t s) {
  VrNet &nn = *e->vr;
  auto &w = nn.w51;
  const int n = bs.n;
  const int cw[5] = {n, 2 * n, 4 * n, 6 * n, 8 * n};
  const int up_w[4] = {2 * n + 4, 4 * n, 6 * n, 8 * n};   // width of the upsampled slice of D[i]
  // D[i] (level i) = [upsampled (up_w[i]) | skip (cw[i])]
  int hs_[5], ws_[5];
  for (int i = 0; i < 5; ++i) {
    hs_[i] = H >> i;
    ws_[i] = W >> i;
  }
  CHK(vr_conv(e, bs.enc1, x, x_ld, x_bs, B, H, W, 1, w.D[0] + up_w[0], up_w[0] + cw[0], 0, s));
  for (int i = 0; i < 4; ++i) {
    const int ld_in = up_w[i] + cw[i];
    CHK(vr_conv(e, bs.e1[i], w.D[i] + up_w[i], ld_in, (int64_t)hs_[i] * ws_[i] * ld_in, B, hs_[i], ws_[i], 2, w.T[i], cw[i + 1], 0, s));
    if (i < 3) CHK(vr_conv(e, bs.e2[i], w.T[i], cw[i + 1], 0, B, hs_[i + 1], ws_[i + 1], 1, w.D[i + 1] + up_w[i + 1], up_w[i + 1] + cw[i + 1], 0, s));
    else CHK(vr_conv(e, bs.e2[i], w.T[i], cw[i + 1], 0, B, hs_[4], ws_[4], 1, w.e5, cw[4], 0, s));
  }
  // ASPP (layers_new.py:95-126), dilations ((4, 2), (8, 4), (12, 6))
  const int h = hs_[4], ww = ws_[4], ca = cw[4], catc = 5 * ca;
  auto &b = nn.b;
  CHK(vr_ew(e, s, (int64_t)B * ww * ca, 4.0 * B * h * ww * ca, vr_rowmean_kernel, (const float *)w.e5, h, ww, ca, b.pool));
  CHK(vr_conv(e, bs.aspp1, b.pool, ca, 0, B, 1, ww, 1, b.pool2, ca, 0, s));
  CHK(vr_ew(e, s, (int64_t)B * h * ww * ca, 4.0 * B * h * ww * ca, vr_bcast_rows_kernel, (const float *)b.pool2, h, ww, ca, b.cat, catc));
  CHK(vr_conv(e, bs.aspp2, w.e5, ca, 0, B, h, ww, 1, b.cat + ca, catc, 0, s));
  const int dil[3][2] = {{4, 2}, {8, 4}, {12, 6}};
  for (int j = 0; j < 3; ++j) CHK(vr_conv(e, bs.aspp3[j], w.e5, ca, 0, B, h, ww, 1, b.cat + (2 + j) * ca, catc, 0, s, dil[j][0], dil[j][1]));
  CHK(vr_conv(e, bs.bott, b.cat, catc, 0, B, h, ww, 1, b.bn, ca, 0, s));
  // decoders dec4 .. dec2
  const float *prev = b.bn;
  int prev_c = ca;
  float *outs[4] = {nullptr, w.ol, w.o3, w.o4};
  const int out_ld[4] = {0, 2 * n + 4, 4 * n, 6 * n};
  for (int i = 3; i >= 1; --i) {
    const int ld = up_w[i] + cw[i];
    CHK(vr_ew(e, s, (int64_t)B * hs_[i] * ws_[i] * (prev_c / 4), 4.0 * B * 5.0 * hs_[i + 1] * ws_[i + 1] * prev_c, vr_upsample2x_kernel, prev,
              hs_[i + 1], ws_[i + 1], prev_c, i == 3 ? ca : out_ld[i + 1], w.D[i], ld));
    CHK(vr_conv(e, bs.dec[i], w.D[i], ld, 0, B, hs_[i], ws_[i], 1, outs[i], out_ld[i], 0, s));
    prev = outs[i];
    prev_c = cw[i];
  }
  // LSTMModule on the dec2 output (level 1)
  {
    const Vr51Lstm &L = bs.lstm;
    const int H1 = hs_[1], W1 = ws_[1], old_ = 2 * n + 4;
    if (L.nbins != H1) {
      set_err("VR 5.1 LSTM expects %d frequency rows, the net has %d at that level", L.nbins, H1);
      return ASX_ERR_INVALID;
    }
    CHK(vr_conv(e, L.conv, w.ol, old_, 0, B, H1, W1, 1, w.hcv, 4, 0, s));
    CHK(vr_ew(e, s, (int64_t)W1 * B * H1, 8.0 * W1 * B * H1, vr_lstm_in_kernel, (const float *)w.hcv, B, H1, W1, 4, w.xs));
    CHK(ht_linear(e, L.ih, w.xs, H1, (int64_t)W1 * B, w.xp, 8 * L.hs, 0, nullptr, 0, s));
    CHK(vr51_lstm(e, L.hs, w.xp, L.whh.f(), W1, B, w.hsq, s));
    CHK(ht_linear(e, L.dense, w.hsq, 2 * L.hs, (int64_t)W1 * B, w.ys, H1, 1, nullptr, 0, s));
    CHK(vr_ew(e, s, (int64_t)B * H1 * W1, 8.0 * B * H1 * W1, vr_lstm_out_kernel, (const float *)w.ys, B, H1, W1, w.ol, old_, 2 * n));
  }
  // dec1
  {
    const int ld = up_w[0] + cw[0];
    CHK(vr_ew(e, s, (int64_t)B * H * W * (up_w[0] / 4), 4.0 * B * 5.0 * hs_[1] * ws_[1] * up_w[0], vr_upsample2x_kernel, (const float *)w.ol, hs_[1], ws_[1],
              up_w[0], up_w[0], w.D[0], ld));
    CHK(vr_conv(e, bs.dec[0], w.D[0], ld, 0, B, H, W, 1, y, y_ld, y_bs, s));
  }
  return ASX_OK;
}

static int vr51_ensure_workspace(asx_engine *e, int B) {
  VrNet &n = *e->vr;
  if (B <= n.ws_batch) return ASX_OK;
  const asx_vr_config &c = n.cfg;
  const int no = c.arch == 218409 ? 64 : c.cap[0];
  const size_t P = (size_t)B * n.max_bin * c.window_size;
  size_t off = 0;
  std::vector<std::pair<float **, size_t>> plan;
  auto want = [&](float *&p, size_t floats) {
    plan.push_back({&p, off});
    off += (floats * 4 + 255) & ~(size_t)255;
  };
  auto &b = n.b;
  auto &w = n.w51;
  const size_t nm = no;   // widest BaseNet
  want(b.hc, P * n.ctot);
  want(b.h3, P * nm);
  want(b.mk, P * 4);
  want(w.yt, P * nm);
  const size_t upw[4] = {2 * nm + 4, 4 * nm, 6 * nm, 8 * nm}, cw[5] = {nm, 2 * nm, 4 * nm, 6 * nm, 8 * nm};
  for (int i = 0; i < 4; ++i) {
    want(w.D[i], (P >> (2 * i)) * (upw[i] + cw[i]));
    want(w.T[i], (P >> (2 * (i + 1))) * cw[i + 1]);
  }
  want(w.e5, (P >> 8) * cw[4]);
  want(w.o4, (P >> 6) * cw[3]);
  want(w.o3, (P >> 4) * cw[2]);
  want(w.ol, (P >> 2) * (2 * nm + 4));
  want(w.hcv, (P >> 2) * 4);
  const size_t seq = (size_t)B * (c.window_size / 2);
  const size_t hsmax = std::max(c.cap[1] / 2, 4);
  want(w.xs, (P >> 2));
  want(w.xp, seq * 8 * hsmax);
  want(w.hsq, seq * 2 * hsmax);
  want(w.ys, (P >> 2));
  want(b.pool, (size_t)B * c.window_size * cw[4]);
  want(b.pool2, (size_t)B * c.window_size * cw[4]);
  want(b.cat, (P >> 8) * 5 * cw[4]);
  want(b.bn, (P >> 8) * cw[4]);
  CHK(n.ws.ensure(off));
  for (auto &pr : plan) *pr.first = reinterpret_cast<float *>(reinterpret_cast<char *>(n.ws.p) + pr.second);
  n.ws_batch = B;
  return ASX_OK;
}

// CascadedNet.forward (nets_new.py:115-150) on B windows already in hc[..., 0:4]
static int vr51_net_dev(asx_engine *e, int B, hipStream_t s) {
  g_vr_net_passes.fetch_add(1);
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  auto &b = n.b;
  const int no = c.arch == 218409 ? 64 : c.cap[0];
  const int F = n.max_bin, W = c.window_size, ct = n.ctot, bw = F / 2;
  const int64_t hc_bs = (int64_t)F * W * ct, hi = (int64_t)bw * W * ct;
  const int a1 = 4, a2 = 4 + no / 4;
  CHK(vr51_base(e, n.b1l, b.hc, ct, hc_bs, B, bw, W, n.w51.yt, no / 2, 0, s));
  CHK(vr_conv(e, n.c1l, n.w51.yt, no / 2, 0, B, bw, W, 1, b.hc + a1, ct, hc_bs, s));
  CHK(vr51_base(e, n.b1h, b.hc + hi, ct, hc_bs, B, bw, W, b.hc + hi + a1, ct, hc_bs, s));
  CHK(vr51_base(e, n.b2l, b.hc, ct, hc_bs, B, bw, W, n.w51.yt, no, 0, s));
  CHK(vr_conv(e, n.c2l, n.w51.yt, no, 0, B, bw, W, 1, b.hc + a2, ct, hc_bs, s));
  CHK(vr51_base(e, n.b2h, b.hc + hi, ct, hc_bs, B, bw, W, b.hc + hi + a2, ct, hc_bs, s));
  CHK(vr51_base(e, n.b3, b.hc, ct, hc_bs, B, F, W, b.h3, no, 0, s));
  return vr_conv(e, n.outc, b.h3, no, 0, B, F, W, 1, b.mk, 4, 0, s);
}

static double vr_flops_patch(const asx_engine *e) {
  const VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  if (c.v51) {
    auto cf = [](const VrConv &v, double pos) { return 2.0 * pos * v.g.n * (double)v.g.k; };
    auto base51 = [&](const Vr51Base &bs, double P) {
      double f = cf(bs.enc1, P) + cf(bs.dec[0], P);
      for (int i = 0; i < 4; ++i) {
        const double pi = P / (double)(1 << (2 * (i + 1)));
        f += cf(bs.e1[i], pi) + cf(bs.e2[i], pi);
        if (i < 3) f += cf(bs.dec[i + 1], pi);
      }
      const double pa = P / 256.0;
      f += cf(bs.aspp2, pa) + cf(bs.bott, pa);
      for (int j = 0; j < 3; ++j) f += cf(bs.aspp3[j], pa);
      return f;
    };
    const double P = (double)n.max_bin * c.window_size;
    return base51(n.b1l, P / 2) + base51(n.b1h, P / 2) + base51(n.b2l, P / 2) + base51(n.b2h, P / 2) + base51(n.b3, P) +
           cf(n.c1l, P / 2) + cf(n.c2l, P / 2);
  }
  auto base = [&](const VrBase &bs, double P) {
    double f = 0.0;
    double p = P;
    for (int i = 0; i < bs.n_enc; ++i) {
      f += 2.0 * p * bs.enc1[i].g.n * bs.enc1[i].g.k + 2.0 * (p / 4) * bs.enc2[i].g.n * bs.enc2[i].g.k + 2.0 * p * bs.dec[i].g.n * bs.dec[i].g.k;
      p /= 4;
    }
    f += 2.0 * p * (bs.aspp2.g.n * (double)bs.aspp2.g.k * (1 + bs.sep.size()) + bs.bott.g.n * (double)bs.bott.g.k);
    return f;
  };
  const double P = (double)n.max_bin * c.window_size;
  return base(n.s1l, P / 2) + base(n.s1h, P / 2) + base(n.s2, P) + base(n.s3, P) +
         2.0 * P * (n.br2.g.n * (double)n.br2.g.k + n.br3.g.n * (double)n.br3.g.k + 2.0 * n.outc.g.k);
}

// ---- signal chain ---------------------------------------------------------------------------------------------------
static int vr_resample(asx_engine *e, const VrFilt &f, const float *x, int64_t n_in, float *y, int64_t n_out, int acc64, hipStream_t s) {
  if (f.kind == ASX_VR_RES_SINC_FASTEST) {
    const float *tab = e->vr->sinc_tab.f();
    const double float_inc = VR_SINC_INC * (f.ratio < 1.0 ? f.ratio : 1.0);
    const long long inc_fp = llrint(float_inc * 4096.0);
    // librosa >= 0.10 resamples every channel as its own one-channel src_simple call (np.apply_along_axis): python-samplerate generates
    // int(num_frames * ratio) frames, and the one-channel call's end-of-input test drops the last of them when num_frames * ratio is an
    // integer (the frame would need input up to the very end); fix_length pads the zero (round 5, ADVICE r4 -- rounds 3-4 modelled
    // librosa 0.9's single interleaved stereo call)
    const double t_gen = (double)n_in * f.ratio;
    int64_t n_gen = (int64_t)t_gen;
    if ((double)n_gen == t_gen && n_gen > 0) --n_gen;
    n_gen = std::min<int64_t>(n_out, n_gen);
    return timed(e, ASX_PROF_MISC, 0.0, 8.0 * (n_in + n_out), s, [&]() {
      hipLaunchKernelGGL(vr_sinc_kernel, dim3((unsigned)((n_out + 255) / 256), 2), dim3(256), 2 * VR_SINC_TL * sizeof(float), s, x, n_in, tab,
                         tab + VR_SINC_TL, VR_SINC_TL, VR_SINC_TL - 2, f.up, f.down, 0.0, float_inc, inc_fp, float_inc / VR_SINC_INC, n_gen, y, n_out);
    });
  }
  return timed(e, ASX_PROF_MISC, 0.0, 8.0 * (n_in + n_out), s, [&]() {
    hipLaunchKernelGGL(vr_resample_kernel, dim3((unsigned)((n_out + 255) / 256), 2), dim3(256), 0, s, x, n_in, f.h32.f(),
                       reinterpret_cast<const double *>(f.h64.p), f.hlen, f.up, f.down, f.n_pre_remove, y, n_out, acc64);
  });
}

// librosa.resample(y, orig_sr, target_sr, res_type="sinc_fastest") on planar data [channels, n_in] -> [channels, n_out] for ANY
// ratio = float(target_sr) / orig_sr (spec_utils.change_pitch_semitones, :783-790: ratio = 2^(semitones / 12)).  n_out is librosa's
// fix_length target ceil(n_in * ratio); mono_calls: every channel is its own one-channel src_simple call, whose termination test
// drops the last frame when n_in * ratio is an integer (the reference resamples channel by channel there).
static int resample_sinc_dev(asx_engine *e, DevBuf &tabbuf, const float *x, int channels, int64_t n_in, double ratio, int mono_calls,
                             float *y, int64_t n_out, hipStream_t s) {
  if (tabbuf.p == nullptr) CHK(vr_sinc_table(tabbuf));
  const float *tab = tabbuf.f();
  const double float_inc = VR_SINC_INC * (ratio < 1.0 ? ratio : 1.0);
  const long long inc_fp = llrint(float_inc * 4096.0);
  // python-samplerate: int(num_frames * ratio); a one-channel call drops the frame that would reach the end of the input (sinc_pool_plan.h)
  const int64_t n_gen = std::min(sinc_plan_generated(n_in, ratio, mono_calls || channels == 1), n_out);
  return timed(e, ASX_PROF_MISC, 0.0, 4.0 * channels * (n_in + n_out), s, [&]() {
    hipLaunchKernelGGL(vr_sinc_kernel, dim3((unsigned)((n_out + 255) / 256), channels), dim3(256), 2 * VR_SINC_TL * sizeof(float), s, x, n_in,
                       tab, tab + VR_SINC_TL, VR_SINC_TL, VR_SINC_TL - 2, 0, 1, 1.0 / ratio, float_inc, inc_fp, float_inc / VR_SINC_INC, n_gen,
                       y, n_out);
  });
}

// resample_sinc_dev for a list of jobs at one ratio: the checks and the plan on the host (sinc_pool_plan.h), the job table written on
// the device from launch arguments, then ONE launch of vr_sinc_batch_kernel over the workgroups of all jobs.  Nothing is enqueued
// unless every job is valid; the call only enqueues work.
static int resample_sinc_batch_dev(asx_engine *e, const asx_sinc_job *jobs, int n_jobs, double ratio, int mono_calls, hipStream_t s) {
  const char *fn = "asx_resample_sinc_batch_dev";
  std::vector<SincPlanJobIn> in((size_t)std::max(n_jobs, 0));
  if (jobs)
    for (int j = 0; j < n_jobs; ++j) in[j] = SincPlanJobIn{jobs[j].x_dev, jobs[j].y_dev, jobs[j].n_in, jobs[j].n_out, (int)jobs[j].channels};
  const std::string why = sinc_pool_check(jobs ? in.data() : nullptr, n_jobs, ratio);
  REQUIRE(why.empty(), "%s: %s", fn, why.c_str());
  if (n_jobs == 0) return ASX_OK;
  SincPoolPlan pp;
  sinc_pool_build(in.data(), n_jobs, ratio, mono_calls != 0, pp);
  if (e->sinc_tab.p == nullptr) CHK(vr_sinc_table(e->sinc_tab));
  // sized once for the most jobs a call may carry (3.7 MB): a table that grew would be freed, and freeing waits for the device
  CHK(e->sinc_jobs.ensure((size_t)SINC_PLAN_MAX_JOBS * sizeof(SincPoolJob)));
  SincPoolJob *table = reinterpret_cast<SincPoolJob *>(e->sinc_jobs.p);
  double bytes = 0.0;
  for (int g0 = 0; g0 < n_jobs; g0 += SINC_POOL_GROUP) {
    SincPoolGroup g{};
    g.n_jobs = std::min(SINC_POOL_GROUP, n_jobs - g0);
    g.job0 = g0;
    for (int i = 0; i < g.n_jobs; ++i) {
      const asx_sinc_job &jb = jobs[g0 + i];
      g.job[i] = SincPoolJob{jb.x_dev, jb.y_dev, jb.n_in, jb.n_out, pp.job[g0 + i].n_gen, pp.job[g0 + i].blk0, jb.channels, 0};
      bytes += 4.0 * jb.channels * (double)(jb.n_in + jb.n_out);
    }
    hipLaunchKernelGGL(sinc_pool_table_kernel, dim3(1), dim3(64), 0, s, g, table);
    HIPCHK(hipGetLastError());
  }
  const float *tab = e->sinc_tab.f();
  const double float_inc = VR_SINC_INC * (ratio < 1.0 ? ratio : 1.0);   // the arguments of resample_sinc_dev's launch
  const long long inc_fp = llrint(float_inc * 4096.0);
  return timed(e, ASX_PROF_MISC, 0.0, bytes, s, [&]() {
    hipLaunchKernelGGL(vr_sinc_batch_kernel, dim3((unsigned)pp.blocks, (unsigned)pp.max_channels), dim3(256), 2 * VR_SINC_TL * sizeof(float), s,
                       (const SincPoolJob *)table, n_jobs, tab, tab + VR_SINC_TL, VR_SINC_TL, VR_SINC_TL - 2, 1.0 / ratio, float_inc, inc_fp,
                       float_inc / VR_SINC_INC);
  });
}

static int64_t vr_resampled_len(const VrFilt &f, int64_t n_in) {   // ceil(n * ratio) == resample_poly's n_out == librosa's fix_length
  return vr_plan_resampled_len(f.up, f.down, n_in);
}

// what the host-only plan (vr_pool_plan.h) needs of the committed net; built once, by vr_commit
static VrPlanCfg vr_plan_cfg(const VrNet &n) {
  const asx_vr_config &c = n.cfg;
  VrPlanCfg pc;
  pc.band.resize(c.n_bands);
  for (int d = 0; d < c.n_bands; ++d) {
    pc.band[d].hl = n.band[d].b.hl;
    if (d < c.n_bands - 1) {
      pc.band[d].up = n.band[d].ana.up;
      pc.band[d].down = n.band[d].ana.down;
    }
  }
  pc.window_size = c.window_size;
  pc.offset = c.offset;
  pc.max_batch = c.max_batch;
  pc.top_n_fft = c.band[c.n_bands - 1].n_fft;
  pc.top_crop_stop = c.band[c.n_bands - 1].crop_stop;
  pc.pre_filter_start = c.pre_filter_start;
  pc.pre_filter_stop = c.pre_filter_stop;
  return pc;
}

// frames of the combined spectrogram and output length for an input of n samples at the top band's rate
static int vr_plan(const VrNet &n, int64_t n_samples, int *T, int64_t *n_out) {
  vr_plan_frames(n.plan_cfg, n_samples, T, n_out);
  return ASX_OK;
}

// one song's share of the call's state: spectrogram [2, T, bins+1] complex, mask [2, T, bins+1], the rows high_end_process
// keeps [2, T, he_n] complex (he_n = 0: off for the current call), the peak slot
struct VrSongView {
  float2 *X;
  float *M;
  float2 *HE;
  unsigned int *peak;
  int T, he_n;
};

// loading_mix (vr_separator.py:255-291): wave [2, n] float32 at band[N].sr -> X [2, T, bins+1] complex64
static int vr_analysis_dev(asx_engine *e, const float *wave, int64_t n_samples, const VrSongView &v, hipStream_t s) {
  VrNet &n = *e->vr;
  const int NB = n.cfg.n_bands, T = v.T;
  n.wav_ana.resize(NB);
  HIPCHK(hipMemsetAsync(v.X, 0, (size_t)2 * T * n.nb1 * 8, s));
  const float *cur = wave;
  int64_t len = n_samples;
  std::vector<int> row_off(NB, 0);
  for (int d = 1; d < NB; ++d) row_off[d] = row_off[d - 1] + n.band[d - 1].b.crop_stop - n.band[d - 1].b.crop_start;
  for (int d = NB - 1; d >= 0; --d) {
    VrBand &B = n.band[d];
    if (d < NB - 1 && !(B.ana.up == 1 && B.ana.down == 1)) {
      const int64_t lo = vr_resampled_len(B.ana, len);
      CHK(n.wav_ana[d].ensure((size_t)2 * lo * 4));
      CHK(vr_resample(e, B.ana, cur, len, n.wav_ana[d].f(), lo, 0, s));
      cur = n.wav_ana[d].f();
      len = lo;
    }
    CHK(timed(e, ASX_PROF_STFT, 0.0, 8.0 * len + 16.0 * T * (B.b.crop_stop - B.b.crop_start), s, [&]() {
      hipLaunchKernelGGL(vr_stft_kernel, dim3(T, 2), dim3(256), stft_lds(B.plan), s, cur, len, B.b.hl, n.cfg.v51 ? B.b.convert : n.cfg.channel_mode,
                         B.b.crop_start, B.b.crop_stop, row_off[d], n.nb1, n.gain_ana.f(), v.X,
                         B.window.f(), reinterpret_cast<const float2 *>(B.tw.p), B.plan,
                         (d == NB - 1 && v.he_n > 0) ? v.HE : nullptr, v.he_n);
    }));
  }
  return ASX_OK;
}

// one pass of inference_vr._execute over all patches (vr_separator.py:294-327)
static int vr_mask_pass(asx_engine *e, int T, int pad_l, int shift, int patches, int tta, float *M, hipStream_t s) {
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  const int W = c.window_size, roi = W - 2 * c.offset;
  // patches per net pass: an engine knob (results do not depend on it).  4-minute song, 84 patches: 8 / 21 / 28 / 42 / 84 per pass
  // -> 476 / 507 / 489 / 509 / 513x real time (the deep levels of the cascade fill the chip only with many patches); batches are
  // evened out so that no short tail batch runs alone.  ~1 GB of workspace per patch at the 4band_44100 layout (vr.py asks for 48).
  const int maxB = even_batches(patches, c.max_batch > 0 ? c.max_batch : 4);
  CHK(c.v51 ? vr51_ensure_workspace(e, maxB) : vr_ensure_workspace(e, maxB));
  for (int k0 = 0; k0 < patches; k0 += maxB) {
    const int B = std::min(maxB, patches - k0);
    CHK(vr_ew(e, s, (int64_t)B * n.max_bin * W, 16.0 * B * n.max_bin * W, vr_patch_kernel, reinterpret_cast<const float2 *>(n.X.p), T, n.nb1,
              n.max_bin, W, k0, roi, pad_l, reinterpret_cast<const unsigned int *>(n.peak.p), n.b.hc, n.ctot));
    CHK(c.v51 ? vr51_net_dev(e, B, s) : vr_net_dev(e, B, s));
    CHK(vr_ew(e, s, (int64_t)B * roi * n.nb1, 16.0 * B * roi * n.nb1, vr_mask_kernel, (const float *)n.b.mk, B, n.max_bin, W, c.offset, k0, roi,
              shift, T, n.nb1, tta, M));
  }
  return ASX_OK;
}

// weight of merge_artifacts (spec_utils.py:187-211) from the per-frame minimum of the mask; false = the reference's
// try block would have raised (mask left unchanged)
static bool vr_artifact_weight(const std::vector<float> &fmin, float thres, std::vector<float> &weight) {
  const int T = (int)fmin.size(), min_range = 64, fade = 32;
  std::vector<int> idx;
  for (int t = 0; t < T; ++t)
    if (fmin[t] > thres) idx.push_back(t);
  if (idx.empty()) return false;   // idx[0] raises IndexError
  std::vector<int> st{idx[0]}, en;
  for (size_t i = 1; i < idx.size(); ++i)
    if (idx[i] - idx[i - 1] != 1) {
      en.push_back(idx[i - 1]);
      st.push_back(idx[i]);
    }
  en.push_back(idx.back());
  weight.assign(T, 0.f);
  bool have_old = false;
  int old_e = 0;
  auto lin = [&](int i, bool up) { return (float)(up ? (double)i / (fade - 1) : 1.0 - (double)i / (fade - 1)); };
  auto put = [&](int a, int b, auto f) -> bool {   // numpy slice assignment weight[a:b] = vec(len fade or scalar)
    // negative indices wrap like numpy; a broadcast mismatch raises in the reference
    int aa = a < 0 ? a + T : a, bb = b < 0 ? b + T : b;
    aa = std::min(std::max(aa, 0), T);
    bb = std::min(std::max(bb, 0), T);
    return f(aa, bb);
  };
  for (size_t r = 0; r < st.size(); ++r) {
    if (!(en[r] - st[r] > min_range)) continue;
    int s0 = st[r], e0 = en[r];
    if (have_old && s0 - old_e < fade) s0 = old_e - fade * 2;
    if (s0 != 0) {
      if (!put(s0, s0 + fade, [&](int a, int b) {
            if (b - a != fade) return b - a <= 0 ? true : false;
            for (int i = 0; i < fade; ++i) weight[a + i] = lin(i, true);
            return true;
          }))
        return false;
    } else {
      s0 -= fade;
    }
    if (e0 != T) {
      if (!put(e0 - fade, e0, [&](int a, int b) {
            if (b - a != fade) return b - a <= 0 ? true : false;
            for (int i = 0; i < fade; ++i) weight[a + i] = lin(i, false);
            return true;
          }))
        return false;
    } else {
      e0 += fade;
    }
    put(s0 + fade, e0 - fade, [&](int a, int b) {
      for (int i = a; i < b; ++i) weight[i] = 1.f;
      return true;
    });
    old_e = e0;
    have_old = true;
  }
  return true;
}

// cmb_spectrogram_to_wave (spec_utils.py:341-396) of y_spec (which = 0) or v_spec (which = 1) -> out [2, n_out]
static int vr_synthesis_dev(asx_engine *e, int which, const VrSongView &v, float *out, int64_t n_out, hipStream_t s) {
  VrNet &n = *e->vr;
  const int NB = n.cfg.n_bands, T = v.T;
  n.wav_syn.resize(NB);
  n.wav_up.resize(NB);
  int row_off = 0;
  const float *lower = nullptr;
  int64_t lower_len = 0;
  for (int d = 0; d < NB; ++d) {
    VrBand &B = n.band[d];
    const int nf = B.b.n_fft, hop = B.b.hl;
    const int64_t len = (int64_t)hop * (T - 1);
    if (lower != nullptr && lower_len != len) {
      set_err("band %d: the resampled lower bands have %lld samples, this band %lld (hl / sr ratios must agree)", d + 1,
              (long long)lower_len, (long long)len);
      return ASX_ERR_INVALID;
    }
    CHK(n.frames.ensure((size_t)2 * T * nf * 4));
    // squared-window sum over the T frames (librosa.filters.window_sumsquare), on the device: the host loop it replaces cost
    // T * n_fft double adds per band and stem (~100 ms per 4-minute song) and a stream synchronisation
    {
      const int64_t nw = (int64_t)nf + (int64_t)hop * (T - 1);
      CHK(n.wss.ensure((size_t)nw * 4));
      hipLaunchKernelGGL(vr_wss_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, B.window.f(), nf, hop, T, nw, n.wss.f());
      HIPCHK(hipGetLastError());
    }
    CHK(timed(e, ASX_PROF_ISTFT, 0.0, 4.0 * 2 * T * (3.0 * (B.b.crop_stop - B.b.crop_start) + nf), s, [&]() {
      hipLaunchKernelGGL(vr_istft_kernel, dim3(T, 2), dim3(256), istft_lds(B.plan), s, (const float2 *)v.X, (const float *)v.M, which,
                         n.nb1, B.b.crop_start, B.b.crop_stop, row_off, B.gain_syn.f(), n.frames.f(), B.window.f(),
                         reinterpret_cast<const float2 *>(B.tw.p), B.plan,
                         (d == NB - 1 && v.he_n > 0) ? (const float2 *)v.HE : nullptr, v.he_n,
                         n.cfg.pre_filter_start - 10 - v.he_n);
    }));
    row_off += B.b.crop_stop - B.b.crop_start;
    float *dst = d == NB - 1 ? out : nullptr;
    if (!dst) {
      CHK(n.wav_syn[d].ensure((size_t)2 * len * 4));
      dst = n.wav_syn[d].f();
    }
    CHK(timed(e, ASX_PROF_OLA, 0.0, 4.0 * 2 * (T * (double)nf + 2.0 * len), s, [&]() {
      hipLaunchKernelGGL(vr_ola_kernel, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, n.frames.f(), n.wss.f(), nf, hop, T, len,
                         n.cfg.v51 ? B.b.convert : n.cfg.channel_mode, lower, dst);
    }));
    if (d < NB - 1) {
      if (B.syn.up == 1 && B.syn.down == 1) {
        lower = dst;
        lower_len = len;
      } else {
        lower_len = vr_resampled_len(B.syn, len);
        CHK(n.wav_up[d].ensure((size_t)2 * lower_len * 4));
        CHK(vr_resample(e, B.syn, dst, len, n.wav_up[d].f(), lower_len, 1, s));
        lower = n.wav_up[d].f();
      }
    }
  }
  (void)n_out;
  return ASX_OK;
}

// adjust_aggr (spec_utils.py:472-492) of one song's mask
static int vr_aggr_dev(asx_engine *e, const asx_vr_params *pr, float *M, int T, hipStream_t s) {
  VrNet &n = *e->vr;
  double aggr = (double)pr->aggr_value * 2.0;
  if (aggr == 0.0) return ASX_OK;
  if (pr->is_non_accom) aggr = 1.0 - aggr;
  double a0 = aggr, a1 = aggr;
  if (pr->has_corr) {
    a0 += pr->corr_left;
    a1 += pr->corr_right;
  }
  const int64_t nx = (int64_t)2 * T * n.nb1;
  return vr_ew(e, s, nx, 8.0 * nx, vr_aggr_kernel, M, T, n.nb1, (int)pr->split_bin, (float)(1.0 + a0 / 3.0), (float)(1.0 + a0),
               (float)(1.0 + a1 / 3.0), (float)(1.0 + a1));
}

// VRSeparator.separate on arrays (vr_separator.py:168-236): wave [2, n] -> primary [2, n_out], secondary [2, n_out]
static int vr_separate_dev(asx_engine *e, const float *wave, int64_t n_samples, const asx_vr_params *pr, float *primary, float *secondary,
                           hipStream_t s) {
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  int T;
  int64_t n_out;
  CHK(vr_plan(n, n_samples, &T, &n_out));
  REQUIRE(T >= 2, "input too short: %d frames", T);
  int he_n = 0;
  if (pr->high_end_process) {
    // input_high_end_h (vr_separator.py:287): bins above the top band's crop + the pre-filter ramp
    const asx_vr_band &tb = c.band[c.n_bands - 1];
    const int h = (tb.n_fft / 2 - tb.crop_stop) + (c.pre_filter_stop - c.pre_filter_start);
    REQUIRE(h > 0 && h <= tb.n_fft / 2 && c.pre_filter_start - 10 - h >= 0, "high_end_process: %d mirrored rows do not fit below pre_filter_start - 10",
            h);
    const int t_top = (int)(1 + n_samples / tb.hl);
    REQUIRE(t_top == T, "high_end_process needs the top band's frame count (%d) to equal the combined spectrogram's (%d)", t_top, T);
    he_n = h;
    CHK(n.HE.ensure((size_t)2 * T * h * 8));
  }
  const int64_t nx = (int64_t)2 * T * n.nb1;
  CHK(n.X.ensure((size_t)nx * 8));
  CHK(n.M.ensure((size_t)nx * 4));
  CHK(n.peak.ensure(4));
  // this call's one song owns the state buffers from their start
  const VrSongView v{reinterpret_cast<float2 *>(n.X.p), n.M.f(), reinterpret_cast<float2 *>(n.HE.p), reinterpret_cast<unsigned int *>(n.peak.p), T, he_n};
  CHK(vr_analysis_dev(e, wave, n_samples, v, s));
  HIPCHK(hipMemsetAsync(n.peak.p, 0, 4, s));
  hipLaunchKernelGGL(vr_absmax_kernel, dim3(512), dim3(256), 0, s, reinterpret_cast<const float2 *>(n.X.p), nx,
                     reinterpret_cast<unsigned int *>(n.peak.p));
  HIPCHK(hipGetLastError());
  // make_padding (spec_utils.py:86-96)
  const int W = c.window_size;
  int roi = W - 2 * c.offset;
  if (roi == 0) roi = W;
  const int patches = T / roi + 1;
  CHK(vr_mask_pass(e, T, c.offset, 0, patches, 0, n.M.f(), s));
  if (pr->enable_tta) CHK(vr_mask_pass(e, T, c.offset + roi / 2, roi / 2, patches + 1, 1, n.M.f(), s));
  CHK(vr_aggr_dev(e, pr, n.M.f(), T, s));
  if (pr->enable_post_process) {
    CHK(n.fmin.ensure((size_t)T * 4));
    CHK(n.wgt.ensure((size_t)T * 4));
    hipLaunchKernelGGL(vr_frame_min_kernel, dim3((T + 3) / 4), dim3(256), 0, s, n.M.f(), T, n.nb1, n.fmin.f());
    HIPCHK(hipGetLastError());
    std::vector<float> fmin(T), weight;
    HIPCHK(hipMemcpyAsync(fmin.data(), n.fmin.p, (size_t)T * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (vr_artifact_weight(fmin, pr->post_thres, weight)) {
      HIPCHK(hipMemcpyAsync(n.wgt.p, weight.data(), (size_t)T * 4, hipMemcpyHostToDevice, s));
      HIPCHK(hipStreamSynchronize(s));
      CHK(vr_ew(e, s, nx, 8.0 * nx, vr_merge_kernel, n.M.f(), T, n.nb1, (const float *)n.wgt.f()));
    }
  }
  if (primary) CHK(vr_synthesis_dev(e, 0, v, primary, n_out, s));
  if (secondary) CHK(vr_synthesis_dev(e, 1, v, secondary, n_out, s));
  return ASX_OK;
}

// ---- the same for a pool of songs: the patches of all of them share the net passes --------------------------------------
// One pass kind (plain, or TTA with one more patch per song) over the flat patch list of the pool, in passes of
// even_batches(total, max_batch) patches whichever song a patch belongs to.  The gather and the scatter take one launch per
// VR_POOL_SEGMENTS songs a pass touches; the net runs once per pass on the same workspace of max_batch patches.
static int vr_mask_pass_pool(asx_engine *e, const VrPlanCfg &pc, const VrPoolPlan &pp, const std::vector<VrSongView> &views, int tta,
                             hipStream_t s) {
  VrNet &n = *e->vr;
  const asx_vr_config &c = n.cfg;
  const std::vector<VrPoolPatch> &list = tta ? pp.tta : pp.plain;
  const int total = (int)list.size();
  if (total == 0) return ASX_OK;
  const int W = c.window_size, roi = pp.roi;
  const int pad_l = tta ? c.offset + roi / 2 : c.offset, shift = tta ? roi / 2 : 0;
  const int per = vr_pool_per_pass(pc, total);
  CHK(c.v51 ? vr51_ensure_workspace(e, per) : vr_ensure_workspace(e, per));
  std::vector<VrPoolRun> runs;
  // the segments of runs [r0, r1) with slots counted from the first of them; returns the slots they take
  auto segments = [&](int r0, int r1, int B, VrPoolSegs &sg) {
    sg.n = r1 - r0;
    for (int r = r0; r < r1; ++r) {
      const VrSongView &v = views[runs[r].song];
      sg.v[r - r0] = VrPoolSeg{v.X, v.M, v.peak, v.T, runs[r].k0, runs[r].slot0 - runs[r0].slot0};
    }
    return (r1 < (int)runs.size() ? runs[r1].slot0 : B) - runs[r0].slot0;
  };
  for (int j0 = 0; j0 < total; j0 += per) {
    const int B = std::min(per, total - j0);
    vr_pool_runs(list, j0, B, runs);
    const int nr = (int)runs.size();
    for (int r0 = 0; r0 < nr; r0 += VR_POOL_SEGMENTS) {
      VrPoolSegs sg{};
      const int64_t nb = segments(r0, std::min(nr, r0 + VR_POOL_SEGMENTS), B, sg);
      CHK(vr_ew(e, s, nb * n.max_bin * W, 16.0 * nb * n.max_bin * W, vr_patch_pool_kernel, sg, n.nb1, n.max_bin, W, roi, pad_l,
                n.b.hc + (int64_t)runs[r0].slot0 * n.max_bin * W * n.ctot, n.ctot));
    }
    CHK(c.v51 ? vr51_net_dev(e, B, s) : vr_net_dev(e, B, s));
    for (int r0 = 0; r0 < nr; r0 += VR_POOL_SEGMENTS) {
      VrPoolSegs sg{};
      const int64_t nb = segments(r0, std::min(nr, r0 + VR_POOL_SEGMENTS), B, sg);
      CHK(vr_ew(e, s, nb * roi * n.nb1, 16.0 * nb * roi * n.nb1, vr_mask_pool_kernel,
                (const float *)(n.b.mk + (int64_t)runs[r0].slot0 * n.max_bin * W * 4), sg, n.max_bin, W, c.offset, roi, shift, n.nb1, tta));
    }
  }
  return ASX_OK;
}

// songs[i].wave_dev [2, n_i] -> songs[i].primary_dev / secondary_dev [2, n_out_i], each what vr_separate_dev writes for that
// song alone.  Every song is checked and planned before anything is enqueued (vr_pool_plan.h).  Analysis, the peak, the mask
// post-processing and the synthesis run per song on the single-song kernels, each on its song's view of the pooled state; the
// mask passes are shared.  enable_post_process costs one device-to-host copy and one synchronisation for the whole pool.
static int vr_separate_pool_dev(asx_engine *e, const asx_vr_song *songs, int n_songs, const asx_vr_params *pr, hipStream_t s) {
  VrNet &n = *e->vr;
  const VrPlanCfg &pc = n.plan_cfg;
  std::vector<VrPoolSongIn> in((size_t)n_songs);
  for (int i = 0; i < n_songs; ++i) in[i] = VrPoolSongIn{songs[i].wave_dev != nullptr, songs[i].n_samples};
  VrPoolPlan pp;
  std::string err;
  REQUIRE(vr_pool_build(pc, in.data(), n_songs, pr->high_end_process != 0, pp, err), "%s", err.c_str());
  if (n_songs == 0) return ASX_OK;
  const int64_t nb1 = n.nb1, F = pp.frames;
  CHK(n.X.ensure((size_t)2 * F * nb1 * 8));
  CHK(n.M.ensure((size_t)2 * F * nb1 * 4));
  CHK(n.peak.ensure((size_t)n_songs * 4));
  if (pp.he_rows > 0) CHK(n.HE.ensure((size_t)2 * F * pp.he_rows * 8));
  std::vector<VrSongView> views((size_t)n_songs);
  for (int i = 0; i < n_songs; ++i) {
    const VrPoolSong &ps = pp.song[i];
    views[i] = VrSongView{reinterpret_cast<float2 *>(n.X.p) + 2 * ps.frame0 * nb1, n.M.f() + 2 * ps.frame0 * nb1,
                          reinterpret_cast<float2 *>(n.HE.p) + 2 * ps.frame0 * pp.he_rows, reinterpret_cast<unsigned int *>(n.peak.p) + i, ps.T,
                          pp.he_rows};
  }
  HIPCHK(hipMemsetAsync(n.peak.p, 0, (size_t)n_songs * 4, s));
  for (int i = 0; i < n_songs; ++i) {
    CHK(vr_analysis_dev(e, songs[i].wave_dev, songs[i].n_samples, views[i], s));
    hipLaunchKernelGGL(vr_absmax_kernel, dim3(512), dim3(256), 0, s, (const float2 *)views[i].X, (int64_t)2 * views[i].T * nb1, views[i].peak);
    HIPCHK(hipGetLastError());
  }
  CHK(vr_mask_pass_pool(e, pc, pp, views, 0, s));
  if (pr->enable_tta) CHK(vr_mask_pass_pool(e, pc, pp, views, 1, s));
  for (int i = 0; i < n_songs; ++i) CHK(vr_aggr_dev(e, pr, views[i].M, views[i].T, s));
  if (pr->enable_post_process) {
    CHK(n.fmin.ensure((size_t)F * 4));
    CHK(n.wgt.ensure((size_t)F * 4));
    for (int i = 0; i < n_songs; ++i) {
      hipLaunchKernelGGL(vr_frame_min_kernel, dim3((views[i].T + 3) / 4), dim3(256), 0, s, (const float *)views[i].M, views[i].T, n.nb1,
                         n.fmin.f() + pp.song[i].frame0);
      HIPCHK(hipGetLastError());
    }
    std::vector<float> fmin_all((size_t)F), fmin, weight;
    HIPCHK(hipMemcpyAsync(fmin_all.data(), n.fmin.p, (size_t)F * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    n.wgt_host.assign((size_t)F, 0.f);
    std::vector<char> merge((size_t)n_songs, 0);
    bool any = false;
    for (int i = 0; i < n_songs; ++i) {
      const VrPoolSong &ps = pp.song[i];
      fmin.assign(fmin_all.begin() + ps.frame0, fmin_all.begin() + ps.frame0 + ps.T);
      if (vr_artifact_weight(fmin, pr->post_thres, weight)) {
        std::copy(weight.begin(), weight.end(), n.wgt_host.begin() + ps.frame0);
        merge[i] = 1;
        any = true;
      }
    }
    if (any) {
      HIPCHK(hipMemcpyAsync(n.wgt.p, n.wgt_host.data(), (size_t)F * 4, hipMemcpyHostToDevice, s));
      for (int i = 0; i < n_songs; ++i)
        if (merge[i]) {
          const int64_t nx = (int64_t)2 * views[i].T * nb1;
          CHK(vr_ew(e, s, nx, 8.0 * nx, vr_merge_kernel, views[i].M, views[i].T, n.nb1, (const float *)(n.wgt.f() + pp.song[i].frame0)));
        }
    }
  }
  for (int i = 0; i < n_songs; ++i) {
    if (songs[i].primary_dev) CHK(vr_synthesis_dev(e, 0, views[i], songs[i].primary_dev, pp.song[i].n_out, s));
    if (songs[i].secondary_dev) CHK(vr_synthesis_dev(e, 1, views[i], songs[i].secondary_dev, pp.song[i].n_out, s));
  }
  return ASX_OK;
}
