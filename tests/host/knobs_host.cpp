// Host driver of csrc/knobs.h (tests/test_host_knobs.py).
//   knobs_host <scenario>...   a scenario is NAME=VALUE (set NAME for this scenario only) or NAME (leave it unset); for each one, a line
//                              "field=value ..." with every field of a fresh Knobs and EngineKnobs, read with that environment
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../python-audio-separator_amd/csrc/knobs.h"

static void put(const char *f, double v) { printf(" %s=%.17g", f, v); }
static void put(const char *f, int64_t v) { printf(" %s=%lld", f, (long long)v); }
static void put(const char *f, int v) { printf(" %s=%d", f, v); }
static void put(const char *f, bool v) { printf(" %s=%d", f, v ? 1 : 0); }
#define F(obj, field) put(#field, obj.field)

int main(int argc, char **argv) {
  for (int i = 1; i < argc; ++i) {
    const char *eq = strchr(argv[i], '=');
    const std::string name = eq ? std::string(argv[i], (size_t)(eq - argv[i])) : std::string(argv[i]);
    if (eq) setenv(name.c_str(), eq + 1, 1);
    const Knobs k;
    const EngineKnobs ek;
    F(k, poison); F(k, prof_dump); F(k, no_dma); F(k, nt); F(k, fft_radix4); F(k, fft3_gs); F(k, fft3_g); F(k, istft_abl); F(k, finalize4);
    F(k, up_nrep); F(k, conv_kc4); F(k, conv_kc4_n2); F(k, down_kc2); F(k, down6_wide); F(k, winos_abl); F(k, wino_abl); F(k, wino_cfg);
    F(k, gemm_bk64); F(k, gemm_t128); F(k, tdf2); F(k, tdf2_sbit); F(k, tdf2_abl); F(k, tdf2_bk16); F(k, tdf2_small); F(k, tdf3_map);
    F(k, tdf3_nw8); F(k, tdf3_abl); F(k, tdf3_abl_set); F(k, f16x3_n); F(k, f16x3_n_set); F(k, tdf3_eff128); F(k, tdf3_eff128_set);
    F(k, tdf_inplace); F(k, halo); F(k, halo_nt); F(k, halo_split128); F(k, halo_minblk); F(k, gg_lowai); F(k, gg_smallgrid);
    F(k, gg_legacy); F(k, gg_m128); F(k, gather6); F(k, gather6_minn); F(k, gather6_glu); F(k, gather6_strided); F(k, gather6_partial);
    F(k, ht_linear_small); F(k, hd_groups); F(k, hd_mha_db); F(k, ht_mha_db); F(k, mha6); F(k, attn_exact); F(k, attn_db); F(k, attn_qw);
    F(k, attn6); F(k, attn6_qw); F(k, attn_v1); F(k, rof_normfuse); F(k, rof_gelu); F(k, rof_fuse);
    F(ek, winograd); F(ek, winos); F(ek, pair_images); F(ek, gemm_bf16x6); F(ek, gemm_f16x3); F(ek, wino6); F(ek, conv3h); F(ek, down6);
    F(ek, up6); F(ek, fft3); F(ek, fft3p);
    printf("\n");
    unsetenv(name.c_str());
  }
  return 0;
}
