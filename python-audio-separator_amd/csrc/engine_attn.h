// Launch code of the attention kernels, shared by the engines (engine_rof.h, engine_ht.h, engine_hd.h) and the single-op hooks
// asx_op_attention / asx_op_mha (asx.hip): kernel selection by variant, query-tile count and the 1-D XCD-aware grids.  The engines
// keep only the rule that picks a variant (environment switches and engine options); what a variant launches is decided here, so
// the hooks run the production launch code.  Included by asx.hip (one TU).
#pragma once

enum AttnVariant {
  AV_AUTO = 0,
  AV_ATTN2,        // attention2_kernel<1>                 (Roformer, fp32 MFMA)
  AV_ATTN2_QW2,    // attention2_kernel<2>                 (128 queries per workgroup)
  AV_ATTN2_DB,     // attention2_kernel<1, true>           (double-buffered K / V)
  AV_ATTN6,        // attention6_kernel<1>                 (bf16 x 6)
  AV_ATTN6_QW2,    // attention6_kernel<2>
  AV_ATTN6H,       // attention6_kernel<1, true>           (fp16 x 3)
  AV_ATTN6H_QW2,   // attention6_kernel<2, true>
  AV_MHA,          // mha_kernel<dh / 16[, decay]>         (HTDemucs / LocalState, fp32 MFMA)
  AV_MHA_DB,       // mha_kernel<3, decay, true>           (double-buffered, dh 48)
  AV_MHA6,         // mha6_kernel<dh / 16, 1>              (bf16 x 6, dh 48 / 64)
  AV_MHA6_WIDE,    // mha6_kernel<dh / 16, 2>
  AV_MHA6H,        // mha6_kernel<dh / 16, 1, true>        (fp16 x 3)
  AV_MHA6H_WIDE,   // mha6_kernel<dh / 16, 2, true>
  AV_HD_LOCAL,     // hd_local_attn_kernel<dh>             (LocalState, narrow heads: dh 4, 8, 12, 24)
  AV_ATTN6S,       // attention6_kernel<1, true, true>     (fp16 x 1: single product, reduced precision, opt-in)
  AV_ATTN6S_QW2,   // attention6_kernel<2, true, true>
  AV_COUNT
};

static const char *const k_attn_variant_names[AV_COUNT] = {"auto", "attn2", "attn2_qw2", "attn2_db", "attn6", "attn6_qw2", "attn6h",
                                                           "attn6h_qw2", "mha", "mha_db", "mha6", "mha6_wide", "mha6h", "mha6h_wide",
                                                           "hd_local", "attn6s", "attn6s_qw2"};

static int attn_variant_parse(const char *name, int *v) {
  for (int i = 0; i < AV_COUNT; ++i)
    if (name && !strcmp(name, k_attn_variant_names[i])) {
      *v = i;
      return ASX_OK;
    }
  set_err("unknown attention variant '%s'", name ? name : "(null)");
  return ASX_ERR_INVALID;
}

// ---- Roformer (AttnArgs: qkv [M, 3 * heads * 64], one sequence per (outer, inner) index) -------------------------------------
// The sequences of the token matrix [B, T, Fb] (rows b * T * Fb + t * Fb + f): along time (one per (b, f), length T) or along
// frequency (one per (b, t), length Fb).  Sets a.len / row_stride / inner_cnt / outer_stride / inner_stride; returns the sequence count.
static int64_t rof_attn_geometry(AttnArgs &a, int B, int T, int Fb, bool time_axis) {
  if (time_axis) {
    a.len = T;
    a.row_stride = Fb;
    a.inner_cnt = Fb;
    a.outer_stride = (int64_t)T * Fb;
    a.inner_stride = 1;
    return (int64_t)B * Fb;
  }
  a.len = Fb;
  a.row_stride = 1;
  a.inner_cnt = 1;
  a.outer_stride = Fb;
  a.inner_stride = 0;
  return (int64_t)B * T;
}

// Fills a.nqt and launches `v` (one of AV_ATTN2 .. AV_ATTN6H_QW2) over nseq sequences.
static int rof_attn_launch(asx_engine *e, int v, AttnArgs a, int64_t nseq, hipStream_t s) {
  const int qw = (v == AV_ATTN2_QW2 || v == AV_ATTN6_QW2 || v == AV_ATTN6H_QW2 || v == AV_ATTN6S_QW2) ? 2 : 1;
  a.nqt = (a.len + 64 * qw - 1) / (64 * qw);
  const dim3 grid((unsigned)((int64_t)a.nqt * a.heads * nseq));   // 1-D, XCD-aware (kernels_rof.h)
  switch (v) {
    case AV_ATTN2: hipLaunchKernelGGL(attention2_kernel<1>, grid, dim3(256), 0, s, a); break;
    case AV_ATTN2_QW2: hipLaunchKernelGGL(attention2_kernel<2>, grid, dim3(256), 0, s, a); break;
    case AV_ATTN2_DB: hipLaunchKernelGGL((attention2_kernel<1, true>), grid, dim3(256), 0, s, a); break;
    case AV_ATTN6: hipLaunchKernelGGL(attention6_kernel<1>, grid, dim3(256), 0, s, a); break;
    case AV_ATTN6_QW2: hipLaunchKernelGGL(attention6_kernel<2>, grid, dim3(256), 0, s, a); break;
    case AV_ATTN6H: hipLaunchKernelGGL((attention6_kernel<1, true>), grid, dim3(256), 0, s, a); break;
    case AV_ATTN6H_QW2: hipLaunchKernelGGL((attention6_kernel<2, true>), grid, dim3(256), 0, s, a); break;
    case AV_ATTN6S: hipLaunchKernelGGL((attention6_kernel<1, true, true>), grid, dim3(256), 0, s, a); break;
    case AV_ATTN6S_QW2: hipLaunchKernelGGL((attention6_kernel<2, true, true>), grid, dim3(256), 0, s, a); break;
    default: set_err("attention variant '%s' is not a Roformer attention", k_attn_variant_names[v]); return ASX_ERR_INVALID;
  }
  if (v >= AV_ATTN6) {
    const bool s1 = v == AV_ATTN6S || v == AV_ATTN6S_QW2;
    const bool h3 = s1 || v == AV_ATTN6H || v == AV_ATTN6H_QW2;
    g_attn6_launches.fetch_add(1);
    if (h3) g_attn6h_launches.fetch_add(1);
    if (s1) g_attn6s_launches.fetch_add(1);
    e->prof_nprod = s1 ? 1 : (h3 ? 3 : 6);
  }
  return ASX_OK;
}

// ---- MhaArgs (HTDemucs transformer, LocalState of HDemucs / Demucs v3 with a.decay) -----------------------------------------
// Whether `v` (one of AV_MHA .. AV_MHA6H_WIDE) is built for these arguments: mha_kernel reads 16-byte rows (leading dimensions
// multiples of 4) and is built for dh 48 / 64 without decay, dh 16, 32, 48, 64, 96 with it (DB: dh 48); mha6_kernel for dh 48 / 64
// without decay.
static bool mha_variant_ok(int v, const MhaArgs &a, int dh) {
  const bool ld4 = (a.ldq & 3) == 0 && (a.ldk & 3) == 0 && (a.ldv & 3) == 0 && (a.ldo & 3) == 0;
  const bool dec = a.decay != nullptr;
  switch (v) {
    case AV_MHA: return ld4 && (dec ? (dh % 16 == 0 && (dh <= 64 || dh == 96)) : (dh == 48 || dh == 64));
    case AV_MHA_DB: return ld4 && dh == 48;
    case AV_MHA6:
    case AV_MHA6_WIDE:
    case AV_MHA6H:
    case AV_MHA6H_WIDE: return ld4 && !dec && (dh == 48 || dh == 64);
    default: return false;
  }
}

// Fills a.nqt / a.heads and launches `v` over B batch items; the caller has checked mha_variant_ok.
static void mha_launch(asx_engine *e, int v, MhaArgs a, int B, int heads, int dh, hipStream_t s) {
  const bool wide = v == AV_MHA6_WIDE || v == AV_MHA6H_WIDE;   // 128 queries per workgroup
  a.nqt = wide ? (a.nq + 127) / 128 : (a.nq + 63) / 64;
  a.heads = heads;
  const dim3 grid((unsigned)(a.nqt * heads * B));   // 1-D, XCD-aware (kernels_ht.h)
  if (v == AV_MHA || v == AV_MHA_DB) {
    if (a.decay) {
      switch (dh / 16) {
        case 1: hipLaunchKernelGGL((mha_kernel<1, true>), grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL((mha_kernel<2, true>), grid, dim3(256), 0, s, a); break;
        case 3:
          if (v == AV_MHA_DB) hipLaunchKernelGGL((mha_kernel<3, true, true>), grid, dim3(256), 0, s, a);
          else hipLaunchKernelGGL((mha_kernel<3, true>), grid, dim3(256), 0, s, a);
          break;
        case 4: hipLaunchKernelGGL((mha_kernel<4, true>), grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((mha_kernel<6, true>), grid, dim3(256), 0, s, a); break;
      }
    } else if (v == AV_MHA_DB) hipLaunchKernelGGL((mha_kernel<3, false, true>), grid, dim3(256), 0, s, a);
    else if (dh == 48) hipLaunchKernelGGL((mha_kernel<3>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((mha_kernel<4>), grid, dim3(256), 0, s, a);
    return;
  }
  const bool h3 = v == AV_MHA6H || v == AV_MHA6H_WIDE;         // fp16 x 3 arithmetic (kernels_ht.h: template parameter H)
  if (h3) {
    if (dh == 48) {
      if (wide) hipLaunchKernelGGL((mha6_kernel<3, 2, true>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((mha6_kernel<3, 1, true>), grid, dim3(256), 0, s, a);
    } else {
      if (wide) hipLaunchKernelGGL((mha6_kernel<4, 2, true>), grid, dim3(256), 0, s, a);
      else hipLaunchKernelGGL((mha6_kernel<4, 1, true>), grid, dim3(256), 0, s, a);
    }
    g_attn6h_launches.fetch_add(1);
  } else if (dh == 48) {
    if (wide) hipLaunchKernelGGL((mha6_kernel<3, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((mha6_kernel<3, 1>), grid, dim3(256), 0, s, a);
  } else {
    if (wide) hipLaunchKernelGGL((mha6_kernel<4, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((mha6_kernel<4, 1>), grid, dim3(256), 0, s, a);
  }
  g_attn6_launches.fetch_add(1);
  e->prof_nprod = h3 ? 3 : 6;
}

// ---- LocalState with narrow heads (kernels_hd.h): qkvd [B * T, ld] = query | key | content (H = 4 * dh each) | decay logits [16] ---
static bool hd_local_ok(int dh) { return dh == 4 || dh == 8 || dh == 12 || dh == 24; }

template <int DH>
static void hd_launch_attn(const float *qkvd, int ld, int T, int H, float *out, int B, hipStream_t s) {
  hipLaunchKernelGGL((hd_local_attn_kernel<DH>), dim3((unsigned)((T + 63) / 64), 4, (unsigned)B), dim3(64), 0, s, qkvd, ld, T, H, out);
}

// out [B * T, H]; the caller has checked hd_local_ok(H / 4)
static void hd_local_launch(const float *qkvd, int ld, int T, int H, float *out, int B, hipStream_t s) {
  switch (H / 4) {
    case 4: hd_launch_attn<4>(qkvd, ld, T, H, out, B, s); break;
    case 8: hd_launch_attn<8>(qkvd, ld, T, H, out, B, s); break;
    case 12: hd_launch_attn<12>(qkvd, ld, T, H, out, B, s); break;
    default: hd_launch_attn<24>(qkvd, ld, T, H, out, B, s); break;
  }
}
