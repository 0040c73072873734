// Every environment knob libasx.so reads, with its parse rule, its default and what it steers -- the only place in the library that calls
// getenv.  Plain C++17 without HIP: tests/host/knobs_host.cpp compiles it with g++ and prints every field.
//
// Two snapshots:
//  - knobs(): the process-wide knobs, read once, at the first asx_engine_create of the process;
//  - EngineKnobs: the defaults of one engine's options, read afresh by every asx_engine_create (asx.hip applies the asx_set_option
//    normalisers to them).
// The comment at a use site explains the dispatch rule it implements; the meaning of the knob itself is stated here.  Most of them are
// A/B switches or tuning and bisection aids that leave the default run as it is.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>

// second-generation row GEMM mode when ASX_TDF2 is unset (a build may pass -DASX_TDF2_DEFAULT=n)
#ifndef ASX_TDF2_DEFAULT
#define ASX_TDF2_DEFAULT 1
#endif

// chunk groups of one length that advance together through the Demucs v3 BLSTMs (engine_hd.h); ASX_HD_GROUPS may only lower it
constexpr int HD_MAX_GROUPS = 6;

// the parse rules: one per idiom, each exactly as the library has always read its knobs (atoi / atof: "" and "abc" read 0)
namespace knob {
// "set at all": any value, "" and "0" included
inline bool set(const char *name) { return getenv(name) != nullptr; }
// "int with default": the value when set, else `def`
inline int num(const char *name, int def) { return set(name) ? atoi(getenv(name)) : def; }
inline int64_t num64(const char *name, int64_t def) { return set(name) ? atoll(getenv(name)) : def; }
inline double real(const char *name, double def) { return set(name) ? atof(getenv(name)) : def; }
// "on unless 0": only a value that reads 0 turns it off
inline bool on_unless_0(const char *name) { return !(set(name) && atoi(getenv(name)) == 0); }
// "off unless non-zero": only a value that reads non-zero turns it on
inline bool off_unless_nonzero(const char *name) { return set(name) && atoi(getenv(name)) != 0; }
// "clamped": the value held to [lo, hi] when set, else `def`
inline int clamped(const char *name, int def, int lo, int hi = INT_MAX) { return set(name) ? std::max(lo, std::min(hi, atoi(getenv(name)))) : def; }
}  // namespace knob

struct Knobs {
  // ---- memory and debugging --------------------------------------------------------------------------------------------------------
  int poison = knob::num("ASX_POISON", -1);                       // >= 0: fill every fresh device allocation with this byte (255 = NaN floats)
  bool prof_dump = knob::set("ASX_PROF_DUMP");                    // asx_profile_read prints one line per launch on stderr
  bool no_dma = knob::set("ASX_NO_DMA");                          // no LDS-DMA conv / row-GEMM kernels (presence only: ASX_NO_DMA=0 turns DMA off too)
  int nt = knob::num("ASX_NT", 0);                                // non-temporal memory ops, bit 0: conv stores, 1: TDF stores, 2: TDF residual loads
  // ---- FFT ------------------------------------------------------------------------------------------------------------------------
  bool fft_radix4 = knob::off_unless_nonzero("ASX_FFT_RADIX4");   // generic FFT plans of radix 4 / 2 only (no radix-16 / 8 passes)
  int fft3_gs = knob::clamped("ASX_FFT3_GS", 16, 1);              // frames per workgroup of stft3p_kernel
  int fft3_g = knob::clamped("ASX_FFT3_G", 16, 5);                // frames per workgroup of the fused inverse (istft3 / istft3p)
  int istft_abl = knob::num("ASX_ISTFT_ABL", 0);                  // 1..3: istft3p_kernel ablation probes (timing only, results invalid)
  bool finalize4 = knob::on_unless_0("ASX_FINALIZE4");            // the vector (4-sample) path of the chunk fold
  // ---- MDX convolutions -----------------------------------------------------------------------------------------------------------
  int up_nrep = knob::num("ASX_UP_NREP", 0);                      // 4: four virtual tiles per workgroup of the transposed conv wherever they divide
  int conv_kc4 = knob::num("ASX_CONV_KC4", 1 << 30);              // 3x3 convs with at most this many input channels stage four channels at a time
  int conv_kc4_n2 = knob::num("ASX_CONV_KC4_N2", 1);              // ... also in two-tile channel groups (0: eight-channel stages there)
  int down_kc2 = knob::num("ASX_DOWN_KC2", 1);                    // 2x2 / stride-2 convs stage two channels at a time (0: four)
  int down6_wide = knob::num("ASX_DOWN6_WIDE", 1);                // conv_down6_kernel: 96-channel workgroups where Cout % 96 == 0
  int winos_abl = knob::num("ASX_WINOS_ABL", 0);                  // experimental builds: conv_winos_kernel ablation probes (results invalid)
  int wino_abl = knob::num("ASX_WINO_ABL", 0);                    // experimental builds: conv_wino3_kernel ablation probes (results invalid)
  int wino_cfg = knob::num("ASX_WINO_CFG", 6);                    // experimental builds: conv_wino3_kernel stage / buffer form (6 = the default one)
  // ---- row GEMMs ------------------------------------------------------------------------------------------------------------------
  bool gemm_bk64 = knob::set("ASX_GEMM_BK64");                    // tdf_dma_kernel 128 x 192 tiles with 64-float K stages
  int gemm_t128 = knob::num("ASX_GEMM_T128", 1);                  // wide-output tile: 1 = cost model, 0 = 128 x 192 always, 2 = 128 x 128 always
  int tdf2 = knob::num("ASX_TDF2", ASX_TDF2_DEFAULT);             // tdf2_kernel: 0 = off, 1 = on, 2 = + persistent on short K, 3 = + start stagger
  int tdf2_sbit = knob::num("ASX_TDF2_SBIT", 8);                  // block-id bit of the tdf2 start stagger (mode 3)
  int tdf2_abl = knob::num("ASX_TDF2_ABL", 0);                    // experimental builds: tdf2_kernel ablation probes
  int tdf2_bk16 = knob::num("ASX_TDF2_BK16", 0);                  // experimental builds: 16-float stages, 1 = 128 x 192 tile, 2 = 64 x 192
  int tdf2_small = knob::num("ASX_TDF2_SMALL", 0);                // > 0: 64 x 128 tiles on layers with K up to this
  int tdf3_map = knob::num("ASX_TDF3_MAP", -1);                   // >= 0: tdf3 tile -> XCD map, digits "<narrow><wide>"; -1 = by column tiles
  bool tdf3_nw8 = knob::on_unless_0("ASX_TDF3_NW8");              // N = 384 on one 8-wave workgroup per row block (fp16 x 3)
  int tdf3_abl = knob::num("ASX_TDF3_ABL", 0);                    // non-zero: launch_tdf3 stays on bf16 x 6; experimental builds: tdf3_kernel ablation probes
  bool tdf3_abl_set = knob::set("ASX_TDF3_ABL");                  // ... set at all, even to 0: no pair images
  int f16x3_n = knob::num("ASX_F16X3_N", 0);                      // bisection aid: fp16 x 3 row GEMMs only with this N (< 0: all but -N)
  bool f16x3_n_set = knob::set("ASX_F16X3_N");                    // ... set at all, even to 0: no pair images
  double tdf3_eff128 = knob::real("ASX_TDF3_EFF128", 0.96);       // relative efficiency charged to tdf3's 128-column tile
  bool tdf3_eff128_set = knob::set("ASX_TDF3_EFF128");            // ... set at all: charged on short-K fp16 x 3 layers too (else 1.0 there)
  bool tdf_inplace = knob::off_unless_nonzero("ASX_TDF_INPLACE"); // the TDF block's x + tdf(x) written over x where no skip copy is needed
  // ---- HTDemucs / Demucs / VR -----------------------------------------------------------------------------------------------------
  bool halo = knob::on_unless_0("ASX_HALO");                      // the halo-tile packing of stride-1 k3 / 3x3 convs (hg_kernel)
  int halo_nt = knob::num("ASX_HALO_NT", 0);                      // 32 / 64 / 96 / 128: force hg_kernel's N tile
  bool halo_split128 = knob::off_unless_nonzero("ASX_HALO_SPLIT128");   // 64-column hg tiles where 128 would fit
  int64_t halo_minblk = knob::num64("ASX_HALO_MINBLK", 0);        // halo launches of fewer workgroups stay on gg_kernel
  double gg_lowai = knob::real("ASX_GG_LOWAI", 90.0);             // gg launches under this flop / byte take 64-row tiles
  int64_t gg_smallgrid = knob::num64("ASX_GG_SMALLGRID", 1024);   // ... and so do those with fewer 128-row workgroups than this
  bool gg_legacy = knob::set("ASX_GG_LEGACY");                    // the old gg N tiles (64 / 128 only)
  bool gg_m128 = knob::on_unless_0("ASX_GG_M128");                // 128-row (not 256-row) gg tiles on narrow outputs
  bool gather6 = knob::on_unless_0("ASX_GATHER6");                // stride-1 dense convs on tdf3_kernel's GATHER mode
  int gather6_minn = knob::num("ASX_GATHER6_MINN", 48);           // ... from this many output columns
  bool gather6_glu = knob::on_unless_0("ASX_GATHER6_GLU");        // ... the GLU convs too
  bool gather6_strided = knob::on_unless_0("ASX_GATHER6_STRIDED");   // ... the strided ones too
  bool gather6_partial = knob::on_unless_0("ASX_GATHER6_PARTIAL");   // ... channel counts off the 32-grid too (zero-padded chunks)
  bool ht_linear_small = knob::on_unless_0("ASX_HT_LINEAR_SMALL");   // 64 x 128 row-GEMM tiles on the transformer linears
  int hd_groups = knob::clamped("ASX_HD_GROUPS", HD_MAX_GROUPS, 1, HD_MAX_GROUPS);   // chunk groups that share the BLSTM launches
  // ---- attention --------------------------------------------------------------------------------------------------------------------
  // ASX_MHA_DB has two meanings, one per engine: on by default for the Demucs v3 LocalState attention, off by default for HTDemucs
  bool hd_mha_db = knob::on_unless_0("ASX_MHA_DB");               // Demucs v3 LocalState (dh 48): the double-buffered mha build
  bool ht_mha_db = knob::off_unless_nonzero("ASX_MHA_DB");        // HTDemucs (dh 48, fp32 kernels): the double-buffered mha build
  bool mha6 = knob::on_unless_0("ASX_MHA6");                      // HTDemucs attention on mha6_kernel while "gemm_bf16x6" is on
  int attn_exact = knob::set("ASX_ATTN_EXACT");                   // 1: libm expf in every attention softmax
  bool attn_db = knob::off_unless_nonzero("ASX_ATTN_DB");         // Roformer fp32 attention: the double-buffered build
  int attn_qw = knob::num("ASX_ATTN_QW", 1);                      // Roformer fp32 attention: 2 = 128 queries per workgroup
  bool attn6 = knob::on_unless_0("ASX_ATTN6");                    // Roformer attention on attention6_kernel while "gemm_bf16x6" is on
  int attn6_qw = knob::num("ASX_ATTN6_QW", 2);                    // ... 2: 128 queries per workgroup on sequences over 128
  bool attn_v1 = knob::off_unless_nonzero("ASX_ATTN_V1");         // experimental builds: the 4-byte-fragment Roformer attention_kernel
  // ---- Roformer ---------------------------------------------------------------------------------------------------------------------
  bool rof_normfuse = knob::on_unless_0("ASX_ROF_NORMFUSE");      // RMSNorms folded into the projections behind them
  int rof_gelu = knob::num("ASX_ROF_GELU", 2);                    // feed-forward activation code: 2 = libm erff, 6 = fast_erf, 1 = ReLU (timing probe)
  bool rof_fuse = knob::on_unless_0("ASX_ROF_FUSE");              // rotary embedding in the q / k projection's epilogue
};

// the process-wide snapshot (asx_engine_create takes it first)
inline const Knobs &knobs() {
  static const Knobs k;
  return k;
}

// The defaults of one engine's options, before the normaliser of asx_set_option (asx.hip), read by every asx_engine_create.
struct EngineKnobs {
#ifdef ASX_EXPERIMENTAL_KERNELS
  int winograd = knob::clamped("ASX_WINOGRAD", 3, 0);             // "winograd": 3x3 conv kernel, 0 / 1 / 2 / 3
  int winos = knob::clamped("ASX_WINOS", 0, 0);                   // "winograd_stationary"
  int pair_images = knob::num("ASX_PAIR_IMAGES", 0);              // "gemm_pair_images"
#else   // generations 1 / 2, the stationary form and pair images are not in this build: any positive ASX_WINOGRAD means 3
  int winograd = knob::num("ASX_WINOGRAD", 3) <= 0 ? 0 : 3;
  int winos = 0;
  int pair_images = 0;
#endif
  int gemm_bf16x6 = knob::num("ASX_GEMM_BF16X6", 1);              // "gemm_bf16x6"
  int gemm_f16x3 = knob::num("ASX_GEMM_F16X3", 1);                // "gemm_f16x3"
  int gemm_f16x1 = 0;                                             // "gemm_f16x1": an option only (no environment name: tests/test_host_knobs.py pins their set), off unless a caller asks
  int wino6 = knob::clamped("ASX_WINO6", 144, 0);                 // "winograd_bf16x6"
  int conv3h = knob::clamped("ASX_CONV3H", 144, 0);               // "conv_direct_f16x3"
  int conv_fuse_input = 1;                                        // "conv_fuse_input": an option only -- tests/test_host_knobs.py pins the set of environment names this header reads
  int tdf_fuse_output = 1;                                        // "tdf_fuse_output": an option only, as the one above
  int conv3h_ps = 1;                                              // "conv3h_partial_scratch": an option only, as the one above
  int conv3h_walk = 1;                                            // "conv3h_walk": an option only, too
  int conv3h_tiled = 1;                                           // "conv3h_tiled": an option only, too
  int conv3h_merge = 144;                                         // "conv3h_merge_out": an option only, too
  int down6 = knob::num("ASX_DOWN6", 1);                          // "conv_down_bf16x6"
  int up6 = knob::num("ASX_UP6", 1);                              // "conv_up_bf16x6"
  bool fft3 = knob::on_unless_0("ASX_FFT3");                      // the fast FFT path where the geometry allows it (n_fft 6144 / hop 1024)
  bool fft3p = knob::on_unless_0("ASX_FFT3P");                    // ... with its LDS-DMA prefetching forms (stft3p / istft3p)
};
