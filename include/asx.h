/*
 * asx.h -- C ABI of the MI355X-native demix engine (libasx.so).
 *
 * Drop-in boundary for ONE hot path of nomadkaraoke/python-audio-separator: the
 * chunked-spectrogram demix loop behind its architecture plugins.  Primary: the MDX
 * plugin (audio_separator/separator/architectures/mdx_separator.py, MDXSeparator.demix
 * :293-412 and run_model :414-450, with uvr_lib_v5/stft.py:20-126 and the ConvTDFNet
 * graph of uvr_lib_v5/mdxnet.py:30-120 that the reference executes through onnxruntime
 * at mdx_separator.py:122-123).  Sibling loops behind the same handle: MDXC (TFC-TDF v3,
 * BS / Mel-Band Roformer: mdxc_separator.py:257-468), Demucs v4 / v3
 * (demucs_separator.py:162-194, uvr_lib_v5/demucs/apply.py:124-260), VR
 * (vr_separator.py:255-375), and the normalise / quantise / ensemble / invert edges
 * (common_separator.py:309-337, ensembler.py, uvr_lib_v5/spec_utils.py:99,573).
 *
 * Plain C: pointers and sizes only, no torch/STL types.  Every function returns
 * ASX_OK (0) or a positive error code and never throws; the message of the last
 * failing call on the calling thread is available from asx_last_error().
 *
 * Ownership: the caller owns every buffer it passes in; the engine owns its
 * device workspace and copies weights at asx_net_commit().  One engine is bound
 * to one GPU; calls on one engine must be serialised by the caller (the
 * reference object is not re-entrant either).  "host" pointers are
 * pageable or pinned host memory, "dev" pointers are HIP device pointers on the
 * engine's GPU.  `stream` is a hipStream_t passed as void* (NULL = the null
 * stream).  asx_demix_dev / asx_demix_chunks_dev / asx_finalize_dev / asx_separate_dev, the
 * asx_mdxc_*_dev, asx_rof_*_dev, asx_ht_*_dev and asx_hd_*_dev calls only enqueue work on `stream` once the
 * engine's workspace has reached its size and the split weight images of the bf16 x 6 kernels exist (both happen in the first
 * call after weights were loaded: the images are built lazily, with one stream synchronisation each): no host copy, no host
 * synchronisation afterwards (chunk / segment
 * start tables are built by a kernel or travel in the kernel arguments) -- they can be captured into a hipGraph
 * and a collective on step k can overlap the compute of step k + 1.  asx_vr_separate_dev synchronises `stream`
 * only when enable_post_process asks for merge_artifacts (its run-length pass is host code).
 *
 * All audio is float32.  Layouts are C-order.
 */
#ifndef ASX_H
#define ASX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASX_OK 0
#define ASX_ERR_INVALID 1 /* bad argument / inconsistent configuration       */
#define ASX_ERR_HIP 2     /* a HIP runtime call failed (no GPU, OOM, launch) */
#define ASX_ERR_STATE 3   /* call order violated (e.g. demix before commit)  */

#define ASX_ABI_VERSION 8

/* flags of asx_demix*(): */
#define ASX_FLAG_MATCH_MIX 1u /* demix(mix, is_match_mix=True): overlap 0.02, no net (mdx_separator.py:308-313, :429-432) */

typedef struct asx_engine asx_engine;

/* Scalars of MDXSeparator that shape the path.
 *   n_fft        model_data["mdx_n_fft_scale_set"]   mdx_separator.py:72
 *   hop_length   arch_config["hop_length"]           mdx_separator.py:59
 *   dim_f        model_data["mdx_dim_f_set"]         mdx_separator.py:70
 *   segment_size arch_config["segment_size"]         mdx_separator.py:31   (frames per chunk)
 *   overlap      arch_config["overlap"]              mdx_separator.py:36
 *   enable_denoise arch_config["enable_denoise"]     mdx_separator.py:62
 *   max_batch    chunks processed per device batch.  Engine knob: the reference's
 *                batch_size never batches chunks and results do
 *                not depend on it.  0 = engine default.
 */
typedef struct asx_mdx_config {
  int32_t n_fft;
  int32_t hop_length;
  int32_t dim_f;
  int32_t segment_size;
  double overlap;       /* a Python float: step = int((1 - overlap) * chunk_size) is evaluated in double, mdx_separator.py:335 */
  int32_t enable_denoise;
  int32_t max_batch;
  int32_t win_length;   /* torch.stft / istft win_length: a periodic Hann window of this length, zero padded to n_fft at both
                         * ends (BSRoformer stft_win_length, bs_roformer.py:376-377); 0 = n_fft */
  int32_t reserved;     /* 0 */
} asx_mdx_config;

/* ConvTDFNet hyper-parameters (uvr_lib_v5/mdxnet.py:31-52); dim_t must equal
 * segment_size, dim_f must equal asx_mdx_config.dim_f.  tdf_bias != 0 when the
 * TDF Linear layers carry a bias (modules.py:57-66).
 * bn (modules.py:52-70): > 0 = Linear(f, f / bn) + norm + ReLU + Linear(f / bn, f) + norm + ReLU; 0 = ONE Linear(f, f) + norm + ReLU
 * (tensors <blk>.tdf0.* only); -1 = `bn is None`, no TDF branch (ABI 6).
 * norm (ABI 6; mdxnet.py:45-49): 0 = BatchNorm2d (optimizer 'rmsprop'), folded into the weights by the host; 1 = GroupNorm(2, c)
 * (optimizer 'adamw'): statistics depend on the input, so every conv / linear tensor arrives UNFOLDED and each normalised layer
 * carries its affine as "<layer>.gn_w" / "<layer>.gn_b" [channels] (layers: first, <blk>.tfc<j>, <blk>.tdf0, <blk>.tdf1, ds<i>, us<i>);
 * the TDF tensors then have no .scale / .shift. */
typedef struct asx_net_config {
  int32_t dim_c;
  int32_t dim_f;
  int32_t dim_t;
  int32_t g;
  int32_t l;
  int32_t num_blocks;
  int32_t k;
  int32_t bn;
  int32_t tdf_bias;
  int32_t norm;
} asx_net_config;

/* Index arithmetic of one demix() call (mdx_separator.py:308-348). */
typedef struct asx_plan {
  int64_t n_samples;  /* N                                    */
  int64_t padded_len; /* L = trim + N + pad                   */
  int64_t chunk_size; /* hop * (segment_size - 1)             */
  int64_t gen_size;   /* chunk_size - 2 * trim                */
  int64_t pad;
  int64_t step;       /* int((1 - overlap) * chunk_size)      */
  int32_t trim;       /* n_fft / 2                            */
  int32_t n_chunks;   /* len(range(0, L, step))               */
  int32_t n_frames;   /* frames per chunk = segment_size      */
  int32_t reserved;
} asx_plan;

/* Per-kernel-class device time, collected with hipEvents on the launch stream
 * while profiling is enabled. */
#define ASX_PROF_STFT 0
#define ASX_PROF_CONV3X3 1
#define ASX_PROF_TDF 2
#define ASX_PROF_DOWN 3
#define ASX_PROF_UP 4
#define ASX_PROF_CONV1X1 5
#define ASX_PROF_ISTFT 6
#define ASX_PROF_OLA 7
#define ASX_PROF_FINALIZE 8
#define ASX_PROF_MISC 9
#define ASX_PROF_NCLASS 10
typedef struct asx_profile {
  int64_t launches[ASX_PROF_NCLASS];
  double ms[ASX_PROF_NCLASS];    /* summed kernel time                       */
  double flops[ASX_PROF_NCLASS]; /* algorithmic 2*MAC of those launches      */
  double bytes[ASX_PROF_NCLASS]; /* algorithmic HBM bytes of those launches  */
} asx_profile;

/* ---- lifetime ---------------------------------------------------------- */
int asx_abi_version(void);
const char *asx_last_error(void);
/* Number of visible HIP devices (0 when there is none; never fails). */
int asx_device_count(void);
int asx_engine_create(int device, const asx_mdx_config *cfg, asx_engine **out);
void asx_engine_destroy(asx_engine *e);
/* The `window=` of torch.stft / istft (ABI 6): `n` = n_fft floats -- a window function evaluated over win_length and zero padded to
 * n_fft at both ends, as torch does -- replacing the periodic Hann the engine builds.  BSRoformer's `stft_window_fn`
 * (uvr_lib_v5/roformer/bs_roformer.py:333, 386).  Call it before the first forward (it synchronises the device). */
int asx_set_stft_window(asx_engine *e, const float *window_host, int32_t n);

/* ---- model weights: replaces ort.InferenceSession(model_path)  mdx_separator.py:122 ----
 * The host hands over BatchNorm-folded fp32 tensors by canonical name, the
 * engine packs them into its kernel layouts and uploads them at commit.
 * Names (blk = enc<i> | mid | dec<i>, i counted like mdxnet.py:63-93):
 *   first.w [g,dim_c]  first.b [g]                       first_conv   mdxnet.py:54-58
 *   <blk>.tfc<j>.w [c,c,k,k]  <blk>.tfc<j>.b [c]         TFC convs    modules.py:11-17
 *   <blk>.tdf0.w [f/bn,f]  .bias [f/bn]  .scale [c]  .shift [c]   TDF  modules.py:62-70
 *   <blk>.tdf1.w [f,f/bn]  .bias [f]     .scale [c]  .shift [c]
 *   ds<i>.w [c+g,c,2,2]  ds<i>.b [c+g]                   mdxnet.py:66-72
 *   us<i>.w [c,c-g,2,2]  us<i>.b [c-g]                   mdxnet.py:80-86 (ConvTranspose2d layout)
 *   final.w [dim_c,g]  final.b [dim_c]                   mdxnet.py:93-95
 * TDF epilogue: relu(scale[c] * (x @ w.T + bias) + shift[c]).
 */
int asx_net_begin(asx_engine *e, const asx_net_config *cfg);
int asx_net_set_tensor(asx_engine *e, const char *name, const float *host, int64_t numel);
int asx_net_commit(asx_engine *e);
/* Algorithmic FLOPs (2*MAC, conv + linear) of one forward over `batch` chunks. */
double asx_net_flops(const asx_engine *e, int32_t batch);

/* ---- the path ---------------------------------------------------------- */
/* Index plan of demix() for a mix of n_samples per channel. */
int asx_plan_query(const asx_engine *e, int64_t n_samples, uint32_t flags, asx_plan *out);

/* MDXSeparator.demix (mdx_separator.py:293): mix [2,N] -> out [2,N]. */
int asx_demix(asx_engine *e, const float *mix_host, int64_t n_samples, float *out_host, uint32_t flags);
int asx_demix_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, float *out_dev, uint32_t flags,
                  void *stream);

/* Sharded form: chunks [chunk_begin, chunk_end) of the plan are
 * run and their windowed outputs written to chunk_out_dev[(k - chunk_begin), 2, chunk_size];
 * asx_finalize_dev() then folds ALL n_chunks windowed chunks (gathered by the
 * caller) into out [2,N] = (result / divider)[trim:-trim][:N]  (mdx_separator.py:386-401). */
int asx_demix_chunks_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t chunk_begin,
                         int32_t chunk_end, float *chunk_out_dev, uint32_t flags, void *stream);
int asx_finalize_dev(asx_engine *e, const float *chunk_out_dev, int64_t n_samples, float *out_dev,
                     uint32_t flags, void *stream);

/* The array part of MDXSeparator.separate (mdx_separator.py:155-182) without leaving the device:
 *   peak = max|mix|; normalize(mix, max_peak, min_peak) IN PLACE (uvr_lib_v5/spec_utils.py:99-115);
 *   primary = demix(mix).T * peak; secondary = (-primary * compensate) + mix.T.
 * mix [2,N] is overwritten with the normalised mix (like the reference's in-place normalize);
 * primary / secondary are [N,2] (interleaved stereo, the layout write_audio consumes,
 * common_separator.py:330-337).  has_min_peak = 0 mirrors min_peak=None. */
int asx_separate(asx_engine *e, float *mix_host, int64_t n_samples, float max_peak, float min_peak,
                 int32_t has_min_peak, float compensate, float *primary_host, float *secondary_host);
int asx_separate_dev(asx_engine *e, float *mix_dev, int64_t n_samples, float max_peak, float min_peak,
                     int32_t has_min_peak, float compensate, float *primary_dev, float *secondary_dev, void *stream);

/* A batch of songs in one call.  The chunks of all songs form one list that runs through the STFT / net / iSTFT launches in
 * batches of up to max_batch chunks, whichever song a chunk belongs to: the launch count depends on the total chunk count, not on
 * the number of songs (64 clips of 20 s are 6 net passes of 64 chunks, not 64 passes of 6).  One segmented fold then writes every
 * song's out [2, n_samples]; each equals what asx_demix_dev writes for that song alone, bit for bit.  `songs` is a HOST array,
 * read during the call; the mixes may have different lengths.  flags as for asx_demix_dev.  The chunk tables are built on the
 * device from launch arguments: like asx_demix_chunks_dev the call only enqueues work on `stream`.  Nothing is enqueued when any
 * song is invalid (null pointer, n_samples < 1); n_songs == 0 is ASX_OK.  The engine's chunk buffer grows to the pool's total
 * chunk count (2 * chunk_size floats per chunk).  (Added within ABI 7: new functions and structs only.) */
typedef struct asx_song {
  const float *mix_dev;   /* [2, n_samples] */
  float *out_dev;         /* [2, n_samples] */
  int64_t n_samples;
} asx_song;
int asx_demix_batch_dev(asx_engine *e, const asx_song *songs, int32_t n_songs, uint32_t flags, void *stream);

/* asx_separate_dev for a batch: per song its own peak, in-place normalise of mix_dev, primary = demix * peak,
 * secondary = mix - compensate * primary ([n_samples, 2] each); all songs share ONE pooled demix as above. */
typedef struct asx_song_stems {
  float *mix_dev;         /* [2, n_samples], normalised in place */
  float *primary_dev;     /* [n_samples, 2] */
  float *secondary_dev;   /* [n_samples, 2] */
  int64_t n_samples;
} asx_song_stems;
int asx_separate_batch_dev(asx_engine *e, const asx_song_stems *songs, int32_t n_songs, float max_peak, float min_peak,
                           int32_t has_min_peak, float compensate, void *stream);

/* ---- MDXC / TFC-TDF v3 (MDX23C): uvr_lib_v5/tfc_tdf_v3.py + the TFC branch of MDXCSeparator.demix ----
 * The engine's n_fft / hop_length / dim_f / segment_size (asx_mdx_config) are config.audio.* and
 * inference.dim_t (or the overridden segment size, mdxc_separator.py:354-359).
 *   norm (tfc_tdf_v3.py:55-69, model.norm):
 *         0       = None / Identity (also any unrecognised norm string)
 *         1       = InstanceNorm (affine)
 *         2       = BatchNorm (eval: running statistics; needs "<prefix>.running_mean" / ".running_var",
 *                   num_batches_tracked is ignored)
 *         256 + G = GroupNorm<G> (G >= 1 groups; G must divide every normalised channel count, else
 *                   asx_v3_commit fails)
 *   act (tfc_tdf_v3.py:72-80, model.act):
 *         0 = relu, 1 = gelu, 2 = elu<alpha>: alpha is the one-element tensor "__act_alpha__", set with
 *         asx_net_set_tensor() between asx_v3_begin() and asx_v3_commit()
 * Weights are handed over with asx_net_set_tensor() under the reference's own state_dict keys
 * (e.g. "encoder_blocks.0.tfc_tdf.blocks.1.tfc1.2.weight"); scale is fixed to [2, 2]. */
typedef struct asx_v3_config {
  int32_t num_channels;         /* config.audio.num_channels (2)        */
  int32_t num_subbands;         /* config.model.num_subbands            */
  int32_t num_scales;           /* config.model.num_scales              */
  int32_t num_blocks_per_scale; /* config.model.num_blocks_per_scale    */
  int32_t num_channels_model;   /* config.model.num_channels            */
  int32_t growth;               /* config.model.growth                  */
  int32_t bottleneck_factor;    /* config.model.bottleneck_factor       */
  int32_t norm;
  int32_t act;
  int32_t num_targets;          /* 1 if training.target_instrument else len(training.instruments) */
} asx_v3_config;
int asx_v3_begin(asx_engine *e, const asx_v3_config *cfg);
int asx_v3_commit(asx_engine *e);
double asx_v3_flops(const asx_engine *e, int32_t batch);
/* TFC_TDF_net.forward (tfc_tdf_v3.py:230): wave [B,2,chunk] -> [B,S,2,chunk] (S = num_targets). */
int asx_v3_forward(asx_engine *e, const float *wave_host, int32_t batch, float *out_host);
/* Index arithmetic of the TFC branch (mdxc_separator.py:361-372): chunk_size, step = hop_size,
 * pad = pad_size, trim = chunk_size - hop_size (front zeros), padded_len, n_chunks. */
int asx_mdxc_plan(const asx_engine *e, int64_t n_samples, int32_t overlap, asx_plan *out);
/* MDXCSeparator.demix, TFC branch (mdxc_separator.py:345-404): mix [2,N] -> out [S,2,N]
 * (= accumulated[..., chunk-hop : -(pad+chunk-hop)] / overlap). */
int asx_mdxc_demix(asx_engine *e, const float *mix_host, int64_t n_samples, int32_t overlap, float *out_host);
/* halves of asx_mdxc_demix_dev for multi-GPU sharding: chunk_out [n_chunks (asx_mdxc_plan), S, 2, chunk_size].  The three single-song
 * calls run a pool of ONE song through the loop and the fold of asx_mdxc_demix_batch_dev (below): chunks_dev runs chunks [k0, k1) into
 * the caller's buffer in passes of up to max_batch chunks, finalize_dev folds the caller's buffer, demix_dev does both on the engine's. */
int asx_mdxc_chunks_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t overlap, int32_t k0, int32_t k1,
                        float *chunk_out_dev, void *stream);
int asx_mdxc_finalize_dev(asx_engine *e, const float *chunk_out_dev, int64_t n_samples, int32_t overlap, float *out_dev, void *stream);
int asx_mdxc_demix_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t overlap, float *out_dev,
                       void *stream);

/* ---- BS-Roformer: uvr_lib_v5/roformer/bs_roformer.py + the Roformer branch of MDXCSeparator.demix ----
 * Engine geometry (asx_mdx_config): n_fft = stft_n_fft (= stft_win_length), hop_length =
 * stft_hop_length, dim_f = n_fft/2 + 1, segment_size = inference.dim_t (mdxc_separator.py:276-300).
 * Weights come in under the reference's own state_dict keys.  dim_head must be 64.  Covers BSRoformer and
 * MelBandRoformer (cfg.mel). */
typedef struct asx_rof_config {
  int32_t dim, depth, heads, dim_head;        /* roformer_loader.py:123-135 */
  int32_t num_stems;
  int32_t time_depth, freq_depth;             /* time_/freq_transformer_depth */
  int32_t mlp_expansion_factor, mask_estimator_depth;
  int32_t n_bands;
  int32_t n_out;                              /* len(training.instruments): rows of the result (mdxc_separator.py:316) */
  int32_t freqs_per_bands[128];
  /* Mel-Band Roformer (uvr_lib_v5/roformer/mel_band_roformer.py): overlapping mel bands -- band j covers frequency bins
   * [band_start[j], band_start[j] + freqs_per_bands[j]) (the support of librosa.filters.mel, computed by the host); band
   * masks are summed onto their bins and divided by the number of covering bands (:404-416); every Transformer ends
   * with its own RMSNorm ("layers.i.k.norm.gamma") instead of one final_norm; the mask MLP has depth+1 linears of
   * hidden width 4*dim. */
  int32_t mel;
  int32_t band_start[128];
  int32_t stft_normalized;                    /* ABI 6: torch.stft / istft normalized=True (bs_roformer.py:332, 384) */
} asx_rof_config;
int asx_rof_begin(asx_engine *e, const asx_rof_config *cfg);
int asx_rof_commit(asx_engine *e);
double asx_rof_flops(const asx_engine *e, int32_t batch);
/* BSRoformer.forward (bs_roformer.py:418): wave [B,2,chunk] -> [B,S,2,chunk]. */
int asx_rof_forward(asx_engine *e, const float *wave_host, int32_t batch, float *out_host);
/* Roformer branch of MDXCSeparator.demix (mdxc_separator.py:272-343): Hamming-weighted fold with the last
 * chunk re-anchored at the tail; `step` = min(int(overlap * sample_rate), chunk_size) in samples.
 * mix [2,N] (N >= chunk_size) -> out [n_out,2,N]. */
int asx_rof_demix(asx_engine *e, const float *mix_host, int64_t n_samples, int64_t step, float *out_host);
int asx_rof_demix_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int64_t step, float *out_dev,
                      void *stream);
/* halves of asx_rof_demix_dev for multi-GPU sharding: chunk_out [n_chunks, S, 2, chunk_size]; as on the TFC branch, the single-song
 * calls are a pool of one song on asx_rof_demix_batch_dev's loop and fold */
int asx_rof_plan(const asx_engine *e, int64_t n_samples, int64_t step, int32_t *n_chunks, int64_t *chunk_size);
int asx_rof_chunks_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int64_t step, int32_t k0, int32_t k1,
                       float *chunk_out_dev, void *stream);
int asx_rof_finalize_dev(asx_engine *e, const float *chunk_out_dev, int64_t n_samples, int64_t step, float *out_dev, void *stream);

/* ---- MDXC: a batch of songs in one call (the sibling of asx_demix_batch_dev for both MDXC loops) ----
 * The chunks of all songs form one list, in song order, that runs through the STFT / net / iSTFT launches in passes of up to
 * max_batch chunks (8 when max_batch is 0, as the single-song calls), whichever song a chunk belongs to: a Roformer pass over a
 * folder of short clips is as full as one over a long song.  One segmented fold then writes every song's out; each equals what
 * asx_mdxc_demix_dev / asx_rof_demix_dev writes for that song alone, bit for bit (those calls ARE this one with n_songs = 1).  `songs` is a HOST array, read during the call;
 * the mixes may have different lengths.  The chunk tables are built on the device from launch arguments: the call only enqueues
 * work on `stream`.  Every argument is checked on the host first and nothing is enqueued when any song is invalid (null pointer,
 * n_samples < 1, on the Roformer branch n_samples < chunk_size -- the message names the song's index); n_songs == 0 is ASX_OK.
 * The net's chunk buffer grows to the pool's total chunk count (S * 2 * chunk_size floats per chunk).
 * (Added within ABI 7: new functions and structs only.) */
typedef struct asx_mdxc_song {
  const float *mix_dev;   /* [2, n_samples] */
  float *out_dev;         /* [S, 2, n_samples]  (Roformer: [n_out, 2, n_samples]) */
  int64_t n_samples;
} asx_mdxc_song;
int asx_mdxc_demix_batch_dev(asx_engine *e, const asx_mdxc_song *songs, int32_t n_songs, int32_t overlap, void *stream);
int asx_rof_demix_batch_dev(asx_engine *e, const asx_mdxc_song *songs, int32_t n_songs, int64_t step, void *stream);

/* ---- Demucs v4 / HTDemucs -----------------------------------------------------
 * Replaces HTDemucs(**kwargs) + load_state_dict (uvr_lib_v5/demucs/htdemucs.py:32-382, demucs_separator.py:121-134),
 * HTDemucs.forward (htdemucs.py:483-620), apply_model (uvr_lib_v5/demucs/apply.py:124-260) and
 * DemucsSeparator.demix_demucs (architectures/demucs_separator.py:162-194).
 * The engine's asx_mdx_config is not used by this path.  Built structure: every layer a frequency layer
 * (nfft/2 / stride^depth > 1), kernel 8 / stride 4, DConv in the encoders, CaC, sinusoidal embeddings, norm_first
 * transformer with LayerScale and norm_out, head dim 48 or 64.  Weights come in under the checkpoint's own
 * state_dict keys; optional "pos_emb_freq" [T*Fr, C] / "pos_emb_time" [L, C] override the sinusoidal tables. */
typedef struct asx_ht_config {
  int32_t n_sources;                     /* len(sources) */
  int32_t channels, growth, nfft, depth; /* htdemucs.py:40-47 */
  int32_t kernel_size, stride;           /* 8, 4 */
  int32_t dconv_depth, dconv_comp;       /* 2, 8 */
  int32_t bottom_channels;               /* 0 = none */
  int32_t t_layers, t_heads, t_hidden;   /* t_hidden = int(C * t_hidden_scale) */
  int32_t samplerate;
  int32_t segment_samples;               /* int(segment * samplerate): training length = split segment */
  float freq_emb_scale;                  /* freq_emb (0.2); 0 = no embedding */
  int32_t max_batch;                     /* segments per forward batch (0 = 16) */
} asx_ht_config;
#define ASX_HT_STANDARDIZE 1u /* (mix - ref.mean()) / ref.std() before, * std + mean after (demucs_separator.py:171-185) */
#define ASX_HT_SWAP01 2u      /* sources[[0, 1]] = sources[[1, 0]] (demucs_separator.py:187) */
int asx_ht_begin(asx_engine *e, const asx_ht_config *cfg);
int asx_ht_commit(asx_engine *e);
double asx_ht_flops(const asx_engine *e);   /* 2*MAC of one segment */
/* HTDemucs.forward: mix [B, 2, length] (length <= segment_samples, zero padded like htdemucs.py:497-502)
 * -> out [B, S, 2, length]. */
int asx_ht_forward(asx_engine *e, const float *mix_host, int32_t batch, int64_t length, float *out_host);
/* apply_model(model, mix[None], shifts, split=True, overlap) (+ the demix_demucs framing selected by `flags`):
 * mix [2, N] -> out [S, 2, N].  offsets[shifts]: the random.randint(0, samplerate/2) draws (apply.py:209) made by
 * the host; shifts = 0 -> no shift trick. */
int asx_ht_demix(asx_engine *e, const float *mix_host, int64_t n_samples, int32_t shifts, const int64_t *offsets,
                 double overlap, uint32_t flags, float *out_host);
int asx_ht_demix_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t shifts, const int64_t *offsets,
                     double overlap, uint32_t flags, float *out_dev, void *stream);
/* The two halves of asx_ht_demix_dev for multi-GPU sharding: the segment-forwards of a call form one list
 * (shift 0's chunks, shift 1's, ...; asx_ht_plan gives its length); a rank runs any sub-range, the folding rank needs all
 * of them: chunk_out [n_segments, S, 2, segment_samples]. */
int asx_ht_plan(const asx_engine *e, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap, int32_t *n_segments,
                int64_t *segment_samples);
int asx_ht_segments_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap,
                        uint32_t flags, int32_t k0, int32_t k1, float *chunk_out_dev, void *stream);
int asx_ht_fold_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap,
                    uint32_t flags, const float *chunk_out_dev, float *out_dev, void *stream);

/* ---- Demucs v3 (HDemucs: the `hdemucs_mmi` entry of the reference's Demucs list) --------------------------
 * Replaces HDemucs(**kwargs) + load_state_dict (uvr_lib_v5/demucs/hdemucs.py:362-571) and HDemucs.forward
 * (:670-782) under the same apply_model / demix_demucs framing as Demucs v4 (apply.py:124-260,
 * architectures/demucs_separator.py:162-194).  Structure built: the class defaults -- CaC, depth - 2 strided levels
 * on both branches, the last-frequency level with the waveform branch injected, one time-only level; GroupNorm,
 * BLSTM(max_steps 200) and LocalState on those two innermost levels.  HDemucs has no valid_length: every chunk
 * of apply_model runs at its own length (apply.py:251-256), so asx_hd_forward takes any length >= 1 (short inputs get
 * pad1d's zero extension before the reflection, hdemucs.py:21-34).
 * Weights come in under the checkpoint's own state_dict keys (asx_net_set_tensor). */
typedef struct asx_hd_config {
  int32_t n_sources;
  int32_t channels, growth, nfft, depth;     /* 48, 2, 4096, 6 */
  int32_t kernel_size, stride, time_stride;  /* 8, 4, 2 */
  int32_t norm_starts, norm_groups;          /* depth - 2, 4 */
  int32_t dconv_depth, dconv_comp;           /* 2, 4 */
  int32_t dconv_attn, dconv_lstm;            /* depth - 2 */
  int32_t samplerate;
  int32_t segment_samples;                   /* int(samplerate * segment): the split length of apply_model */
  float freq_emb_scale;                      /* freq_emb (0.2); 0 = no embedding */
  int32_t max_batch;                         /* equal-length chunks per forward batch (0 = 16) */
} asx_hd_config;
int asx_hd_begin(asx_engine *e, const asx_hd_config *cfg);
int asx_hd_commit(asx_engine *e);
double asx_hd_flops(const asx_engine *e, int64_t length);   /* 2*MAC of one chunk of `length` samples */
/* HDemucs.forward: mix [B, 2, length] -> out [B, S, 2, length] */
int asx_hd_forward(asx_engine *e, const float *mix_host, int32_t batch, int64_t length, float *out_host);
/* apply_model(model, mix[None], shifts, split=True, overlap) + the demix_demucs framing in `flags` (ASX_HT_*):
 * mix [2, N] -> out [S, 2, N]; offsets as for asx_ht_demix. */
int asx_hd_demix(asx_engine *e, const float *mix_host, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap,
                 uint32_t flags, float *out_host);
int asx_hd_demix_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap,
                     uint32_t flags, float *out_dev, void *stream);
/* sharded halves, as asx_ht_plan / asx_ht_segments_dev / asx_ht_fold_dev: chunk_out [n_segments, S, 2, segment_samples],
 * row k holds the chunk's own length of valid samples from column 0 */
int asx_hd_plan(const asx_engine *e, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap, int32_t *n_segments,
                int64_t *segment_samples);
int asx_hd_segments_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap,
                        uint32_t flags, int32_t k0, int32_t k1, float *chunk_out_dev, void *stream);
int asx_hd_fold_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, int32_t shifts, const int64_t *offsets, double overlap,
                    uint32_t flags, const float *chunk_out_dev, float *out_dev, void *stream);

/* ---- Demucs v4 / v3: a batch of songs in one call (the sibling of asx_demix_batch_dev) ----
 * The segments of ALL songs form one list (song-major, each song's in the order of asx_ht_plan) and share the forwards: v4 runs
 * the list in batches of up to max_batch (default 32) segments whichever song a segment belongs to; v3 groups equal chunk
 * lengths across songs (up to max_batch per group).  Every song keeps its own standardisation statistics; one segmented fold per
 * shift index (and 32 songs) writes every song's out [S, 2, n_samples], which equals what asx_ht_demix_dev / asx_hd_demix_dev
 * writes for that song alone, bit for bit.  `songs` and every `offsets` array are HOST memory, read during the call; shifts,
 * overlap and flags (ASX_HT_*) hold for all songs.  The call only enqueues work on `stream`.  Nothing is enqueued when any song
 * is invalid (null pointer, n_samples < 2 as for the single-song calls, an offset outside [0, samplerate / 2], offsets == NULL
 * with shifts > 0); n_songs == 0 is ASX_OK.  Memory: the engine's chunk slab grows to the pool's TOTAL segment count (S * 2 *
 * segment_samples floats per segment): a caller with more songs than that allows splits them over several calls.  v3 also
 * grows its group workspaces: the chunk groups that advance together are full-length ones here, where one song has a single
 * full-length group and short tails, so the groups of one round are bounded to 2 * max_batch segments' worth of samples
 * (about 70 GB of workspace for 44-s chunks at the default max_batch of 16, against about 30 GB for one 4-minute song).  With
 * more than 32 songs the fold takes one launch per shift index and 32 songs.  (Added within ABI 7: new functions and a new
 * struct only.) */
typedef struct asx_apply_song {
  const float *mix_dev;     /* [2, n_samples] */
  float *out_dev;           /* [S, 2, n_samples] */
  int64_t n_samples;
  const int64_t *offsets;   /* HOST: `shifts` draws for this song; NULL iff shifts == 0 */
} asx_apply_song;
int asx_ht_demix_batch_dev(asx_engine *e, const asx_apply_song *songs, int32_t n_songs, int32_t shifts, double overlap, uint32_t flags,
                           void *stream);
int asx_hd_demix_batch_dev(asx_engine *e, const asx_apply_song *songs, int32_t n_songs, int32_t shifts, double overlap, uint32_t flags,
                           void *stream);

/* ---- VR architecture -----------------------------------------------------------------
 * Replaces nets.determine_model_capacity(...) + load_state_dict (architectures/vr_separator.py:168-176,
 * uvr_lib_v5/vr_network/nets.py:65-93), VRSeparator.loading_mix (:255-291), inference_vr (:293-366) and spec_to_wav
 * (:368-375) with the spec_utils functions they call (wave_to_spectrogram, combine_spectrograms, preprocess,
 * make_padding, adjust_aggr, merge_artifacts, cmb_spectrogram_to_wave, spectrogram_to_wave, fft_lp/hp_filter).
 * band[d-1] = modelparams JSON "band"[d] (uvr_lib_v5/vr_network/modelparams/ *.json).  Resampling between bands (ABI 5):
 *   ASX_VR_RES_POLYPHASE     scipy.signal.resample_poly as librosa.resample(res_type="polyphase") calls it;
 *   ASX_VR_RES_SINC_FASTEST  libsamplerate's SRC_SINC_FASTEST as librosa.resample(res_type="sinc_fastest") reaches it through
 *                            python-samplerate (float32 in / out, src_simple): the library's published algorithm (src_sinc.c) on a
 *                            regenerated Kaiser-sinc coefficient table -- the library and fastest_coeffs.h are not available, so this
 *                            converter is "parity unpinned" (INTEGRATION.md "VR resampler").
 * band[d-1].res_type converts band d+1 -> d in loading_mix (vr_separator.py:267,282: the band's own "res_type"; every type other
 * than "sinc_fastest" is served by the polyphase filter); synth_res_type converts band d -> d+1 in cmb_spectrogram_to_wave
 * (spec_utils.py:374,390: the module-level `wav_resolution`, "sinc_fastest" everywhere except macOS on ARM, :33-38).
 */
#define ASX_VR_RES_POLYPHASE 0
#define ASX_VR_RES_SINC_FASTEST 1
typedef struct asx_vr_band {
  int32_t sr, hl, n_fft, crop_start, crop_stop, hpf_start, hpf_stop, lpf_start, lpf_stop;
  int32_t convert;        /* VR 5.1 "convert_channels" (spec_utils.py:232-247): 0 none, 1 mid_side, 4 mid_side_c, 5 stereo_n */
  int32_t res_type;       /* ASX_VR_RES_*: analysis converter of this band (band d+1 -> d); ABI 5 */
} asx_vr_band;
typedef struct asx_vr_config {
  int32_t bins, n_bands, pre_filter_start, pre_filter_stop;
  int32_t channel_mode;   /* 0 stereo, 1 mid_side, 2 mid_side_b2, 3 reverse (model_param_init.py:62-65) */
  int32_t arch;           /* nn_arch_size (vr_separator.py:161-164) */
  int32_t cap[6];         /* stage-1 width, stage-2 bridge out, stage-2 width, stage-3 bridge out, stage-3 width, 0 (nets.py:74-86) */
  int32_t window_size;    /* arch_config["window_size"] */
  int32_t offset;         /* CascadedASPPNet.offset = 128 */
  int32_t max_batch;      /* patches per forward batch (0 = 4); no effect on the result */
  int32_t v51;            /* 1: VR 5.1 -- nets_new.CascadedNet(n_fft, nn_arch_size, nout = cap[0], nout_lstm = cap[1]) and the
                             is_v51_model branches of spec_utils (per-band convert_channels, get_lp/hp_filter_mask); offset 64 */
  int32_t synth_res_type; /* ASX_VR_RES_*: converter of the synthesis chain (`wav_resolution`, spec_utils.py:33-38); ABI 5 */
  asx_vr_band band[8];
} asx_vr_config;
typedef struct asx_vr_params {
  float aggr_value;        /* aggressiveness["value"] = int(aggression) / 100 */
  int32_t split_bin;       /* band[1].crop_stop */
  int32_t is_non_accom;    /* primary stem in CommonSeparator.NON_ACCOM_STEMS */
  int32_t has_corr;
  float corr_left, corr_right;   /* aggr_correction */
  int32_t enable_tta, enable_post_process;
  float post_thres;
  int32_t high_end_process;   /* arch_config["high_end_process"]: spec_utils.mirroring("mirroring") of the input's high end */
} asx_vr_params;
int asx_vr_begin(asx_engine *e, const asx_vr_config *cfg);
int asx_vr_commit(asx_engine *e);
double asx_vr_flops(const asx_engine *e);   /* 2*MAC of the net on one window */
/* frames of the combined spectrogram and length of the separated waves for n_samples input samples */
int asx_vr_plan(const asx_engine *e, int64_t n_samples, int32_t *n_frames, int64_t *n_out);
/* CascadedASPPNet.forward, eval (nets.py:132-161): x [B, 2, bins+1, window_size] -> mask, same shape. */
int asx_vr_forward(asx_engine *e, const float *x_host, int32_t batch, float *out_host);
/* loading_mix: wave [2, n] (float32 at the top band's rate) -> X_spec [2, n_frames, bins+1] complex64 (re, im pairs;
 * note: frames outer, bins inner -- the transpose of the reference's [2, bins+1, n_frames]). */
int asx_vr_analysis(asx_engine *e, const float *wave_host, int64_t n_samples, float *spec_host);
/* the array part of VRSeparator.separate: wave [2, n] -> spec_to_wav(y_spec) [2, n_out], spec_to_wav(v_spec) [2, n_out]
 * (either output may be NULL). */
int asx_vr_separate(asx_engine *e, const float *wave_host, int64_t n_samples, const asx_vr_params *params, float *primary_host,
                    float *secondary_host);
int asx_vr_separate_dev(asx_engine *e, const float *wave_dev, int64_t n_samples, const asx_vr_params *params, float *primary_dev,
                        float *secondary_dev, void *stream);

/* A pool of songs in one call: the patches of all songs share the net passes -- the flat patch list of the pool (song after song,
 * first every song's plain pass, then, with enable_tta, every song's TTA pass with one more patch each) runs in passes of
 * even_batches(total, max_batch) patches, so a pass may hold patches of several songs and a song's patches may span several
 * passes.  The reference separates file by file; a folder of short clips (about 8 patches per 20 s on the 4band_44100 layout,
 * where the cascade wants 48 per pass) is what this is for.  wave_dev [2, n_samples] at the top band's rate; primary_dev /
 * secondary_dev [2, n_out] with n_out from asx_vr_plan, either may be NULL (that stem is not synthesised); every output equals
 * what asx_vr_separate_dev writes for that song alone.  `songs` is HOST memory, read during the call; one asx_vr_params holds for
 * all songs.  Analysis, peak, mask post-processing and synthesis run per song; enable_post_process synchronises `stream` once
 * for the pool (asx_vr_separate_dev: twice per song).  Every song is checked before anything is enqueued -- a NULL wave_dev,
 * fewer than 2 frames, or a refusal of high_end_process reject the call with ASX_ERR_INVALID, the message names the song's
 * index and no output byte is written; n_songs == 0 is ASX_OK.  Memory: the engine keeps the spectrogram and the mask of EVERY
 * song of the pool at once (24 * (bins + 1) bytes per frame), the net workspace stays max_batch patches: a caller with more
 * songs than that allows splits them over several calls.  A pass that touches more than ASX_VR_POOL_SEGMENTS songs takes one
 * gather and one scatter launch per that many.  (Added within ABI 7: a new function, a new struct and a new counter only.) */
#define ASX_VR_POOL_SEGMENTS 16
typedef struct asx_vr_song {
  const float *wave_dev;    /* [2, n_samples] */
  int64_t n_samples;
  float *primary_dev;       /* [2, n_out] or NULL */
  float *secondary_dev;     /* [2, n_out] or NULL */
} asx_vr_song;
int asx_vr_separate_batch_dev(asx_engine *e, const asx_vr_song *songs, int32_t n_songs, const asx_vr_params *params, void *stream);

/* librosa.resample(y, orig_sr, target_sr, res_type="sinc_fastest") for ANY ratio = float(target_sr) / orig_sr, i.e. libsamplerate's
 * SRC_SINC_FASTEST through python-samplerate as above (restated algorithm, regenerated table: parity unpinned).  Replaces
 * spec_utils.change_pitch_semitones (uvr_lib_v5/spec_utils.py:783-790; MDXC pitch_shift, mdxc_separator.py:230-243,268-270) and
 * is the test hook of the converter.  x [channels, n_in] planar -> y [channels, n_out], n_out = ceil(n_in * ratio) (librosa's
 * fix_length; frames the library does not generate are zero).  mono_calls != 0: every channel is its own one-channel call -- the
 * library's end-of-input test then drops the last frame when n_in * ratio is an integer (change_pitch_semitones resamples channel
 * by channel); 0: the channels are the interleaved channels of one call (the VR chain).  ABI 5.
 * n_out is the caller's: it need not be ceil(n_in * ratio).  The converter generates int(n_in * ratio) frames (one fewer in the
 * end-of-input case above); frames of y at or beyond that count are zero, frames the caller leaves out are not computed.  Passing the
 * length of another array is therefore spec_utils.match_array_shapes' trim or zero pad in the same pass (the way back of the pitch
 * round trip passes the original mix's length). */
int asx_resample_sinc(asx_engine *e, const float *x_host, int32_t channels, int64_t n_in, double ratio, int32_t mono_calls,
                      float *y_host, int64_t n_out);
int asx_resample_sinc_dev(asx_engine *e, const float *x_dev, int32_t channels, int64_t n_in, double ratio, int32_t mono_calls,
                          float *y_dev, int64_t n_out, void *stream);

/* asx_resample_sinc_dev for a list of jobs at ONE ratio (the pitched mixes of a batch of songs, or all stems of all songs on the way
 * back) in one launch of the converter over all jobs; the job table travels to an engine-owned device buffer in launch arguments
 * (a small table launch per 32 jobs), so the call only enqueues work on `stream` and never waits for the device -- but for an engine's
 * FIRST sinc call of either kind, which builds the coefficient table with a blocking copy and allocates the job table, at once for the
 * 65,535-job limit (3.7 MB), so that it never grows: growing would free it, and a free waits for the device.  Every job's y
 * equals, bit for bit, what asx_resample_sinc_dev(x_dev, channels, n_in, ratio, mono_calls, y_dev, n_out) writes; n_out is free per
 * job, as above.  Every argument is checked before anything is enqueued -- ASX_ERR_INVALID, asx_last_error() naming the job: a null
 * pointer, n_in or n_out outside 1 .. 2^40, channels outside 1 .. 65535, a ratio outside (1/256, 256), more than 65,535 jobs, more than
 * 2^31 - 1 blocks of 256 output frames in all.  n_jobs == 0 is ASX_OK.  The jobs' outputs must not overlap, nor any input an output;
 * two calls on one engine share the table, so they belong on one stream.  `reserved` is ignored.  Additive within ABI 7. */
typedef struct asx_sinc_job {
  const float *x_dev;       /* [channels, n_in] planar */
  float *y_dev;             /* [channels, n_out] planar */
  int64_t n_in;
  int64_t n_out;
  int32_t channels;
  int32_t reserved;
} asx_sinc_job;
int asx_resample_sinc_batch_dev(asx_engine *e, const asx_sinc_job *jobs, int32_t n_jobs, double ratio, int32_t mono_calls, void *stream);

/* High-quality rational polyphase converter for input files whose sample rate is not the model's (the step librosa.load delegates to
 * soxr_hq, common_separator.py:252; the plugins' opt-in "asx_input_resample" = "device").  This project's own design in that converter's
 * published class -- Kaiser-windowed sinc, 125 dB, pass band to 0.913 of the lower Nyquist frequency; parity with soxr unpinned.  With
 * g = gcd(sr_in, sr_out), L = sr_out / g, M = sr_in / g:  y[m] = sum_i x[i] h[m M - i L] over 0 <= i < n_in, zero history at both ends, zero
 * delay, n_out = ceil(n_in L / M) (librosa's length).  Taps float32, float32 FMA accumulation in a fixed order (bit-identical runs).
 *   asx_resample_rational_plan  pure host: n_out for n_in (n_out may be NULL; n_in is then ignored), L, M and the taps per output.
 *                               ASX_ERR_INVALID + asx_last_error() for equal rates and for pairs whose coefficient table L x taps
 *                               would exceed 2^20 floats (44056 -> 44100 Hz and the like).
 *   asx_resample_rational_dev   x [channels, n_in] planar -> y [channels, n_out] on the device, one launch on `stream`; n_out must be
 *                               the plan's.  The table of a pair is built at its first call and kept on the engine.
 *   asx_resample_rational       the same for host arrays.
 * Additive within ABI 7. */
int asx_resample_rational_plan(int32_t sr_in, int32_t sr_out, int64_t n_in, int64_t *n_out, int32_t *L, int32_t *M, int32_t *taps_per_phase);
int asx_resample_rational_dev(asx_engine *e, const float *x_dev, int32_t channels, int64_t n_in, int32_t sr_in, int32_t sr_out, float *y_dev,
                              int64_t n_out, void *stream);
int asx_resample_rational(asx_engine *e, const float *x_host, int32_t channels, int64_t n_in, int32_t sr_in, int32_t sr_out, float *y_host,
                          int64_t n_out);

/* The writer-side form of the converter: stems back at the input file's sample rate and frame count (the plugins' opt-in
 * "asx_output_rate" = "input"; the reference writes every stem at the model's rate).
 * x: layout 0 = planar [channels, n_in], layout 1 = rows [n_in, channels] (the MDX stem layout); y: planar [channels, n_out].
 * Same definition, taps and summation order as asx_resample_rational_dev: y[m] = sum_i x[i] h[m M - i L], zero history at both ends.
 * n_out is FREE (1 .. 2^40): outputs past the plan's length follow from the definition (they reach exactly 0 once the filter
 * has left the input); a shorter n_out simply stops earlier.  One launch on `stream`, grid (tiles of n_out, channels) -- all S stems of a
 * planar [S, 2, N] tensor go in one call with channels = 2 S; only enqueues (but for the first call of a pair, which builds its table).
 * Bits: planar input gives, for m < the plan's n_out, the bits of asx_resample_rational_dev; rows input gives the bits of planar input of
 * the transposed data; a result does not depend on the launch.
 * Checked before anything is enqueued, ASX_ERR_INVALID + asx_last_error() naming the argument: null pointers, a layout other than 0 or 1,
 * channels outside 1 .. 65535, n_in or n_out outside 1 .. 2^40, equal rates, a pair the plan refuses.  Additive within ABI 7. */
int asx_resample_rational_stem_dev(asx_engine *e, const float *x_dev, int32_t layout, int32_t channels, int64_t n_in,
                                   int32_t sr_in, int32_t sr_out, float *y_dev, int64_t n_out, void *stream);
int asx_resample_rational_stem(asx_engine *e, const float *x_host, int32_t layout, int32_t channels, int64_t n_in,
                               int32_t sr_in, int32_t sr_out, float *y_host, int64_t n_out);   /* host arrays, same kernel */

/* The complement form of the writer-side converter (the plugins' opt-in "asx_complement_rate" = "input"): the complement stem of a file
 * formed at the FILE's rate, against the file's own mix, inside the converter's pass.  With y[ch][m] exactly what
 * asx_resample_rational_stem_dev gives for the same x, layout, channels, n_in, rates and n_out (bit for bit), one launch writes
 *   y                (when y is not NULL), and
 *   c[ch][m] = fl( fl(mix_scale * mix[ch * mix_stride + m]) - fl(stem_scale * y[ch][m]) ),  0 <= m < n_out,
 * fl one float32 rounding each, never contracted into an FMA.  Outputs whose tile lies past the input (y = 0) give c = fl(mix_scale * mix).
 *   mix   planar [channels, mix_stride] at sr_out Hz, mix_stride >= n_out (the decoded file: its frame count)
 *   c     planar [channels, n_out];  y: planar [channels, n_out] or NULL
 * mix, y and c must not overlap.  One launch on `stream`, grid (tiles of n_out, channels); only enqueues (but for the first call of a
 * pair, which builds its table).  Checked before anything is enqueued, ASX_ERR_INVALID + asx_last_error() naming the argument: everything
 * asx_resample_rational_stem_dev checks (y excepted), a null mix or c, mix_stride < n_out, a scale that is not finite.
 * Additive within ABI 8. */
int asx_resample_rational_complement_dev(asx_engine *e, const float *x_dev, int32_t layout, int32_t channels, int64_t n_in,
                                         int32_t sr_in, int32_t sr_out, const float *mix_dev, int64_t mix_stride,
                                         float mix_scale, float stem_scale, float *y_dev /* may be NULL */, float *c_dev,
                                         int64_t n_out, void *stream);
int asx_resample_rational_complement(asx_engine *e, const float *x_host, int32_t layout, int32_t channels, int64_t n_in,
                                     int32_t sr_in, int32_t sr_out, const float *mix_host, int64_t mix_stride,
                                     float mix_scale, float stem_scale, float *y_host /* may be NULL */, float *c_host,
                                     int64_t n_out);   /* host arrays, same kernel */

/* *scale = the float32 factor asx_normalize_dev(wave_dev, numel, max_peak, min_peak, has_min) would multiply the array by -- max_peak / peak,
 * min_peak / peak, or 1 where it leaves the array alone (the mix_scale of the entry above for a mix that is about to be normalised, which
 * is also what asx_separate_dev / asx_separate_batch_dev apply to their mix).  The array is only read; four bytes come back, so the
 * call waits for `stream`.  ASX_ERR_INVALID + asx_last_error() naming the argument: a null engine, wave or scale, numel < 1, a threshold
 * that is not finite, and a silent array under a minimum peak (the factor would be infinite).  Additive within ABI 8. */
int asx_normalize_scale_dev(asx_engine *e, const float *wave_dev, int64_t numel, float max_peak, float min_peak, int32_t has_min,
                            float *scale, void *stream);

/* BagOfModels on the device (uvr_lib_v5/demucs/apply.py:169-196 + demucs_separator.py:171-189; ABI 4).  Every member of a
 * bag keeps its own engine (weights resident across files); the caller demixes the STANDARDISED mix with each member
 * (flags 0) and combines without a host round trip:
 *   asx_ht_standardize_dev     out = (mix - ref.mean()) / ref.std(), ref = mix.mean(0)          [2, N] -> [2, N]
 *   asx_ht_bag_accumulate_dev  est = first ? member * w[k] : est + member * w[k]                 [S, 2, N]; w: S host floats
 *   asx_ht_bag_finish_dev      out = est / totals[k] (* ref.std() + ref.mean() with ASX_HT_STANDARDIZE; sources 0 / 1 swapped
 *                              with ASX_HT_SWAP01); est and out are different buffers.
 * The engine passed in only provides the device, the stream plumbing and the mix statistics (any member's engine). */
int asx_ht_standardize_dev(asx_engine *e, const float *mix_dev, int64_t n_samples, float *out_dev, void *stream);
int asx_ht_bag_accumulate_dev(asx_engine *e, float *est_dev, const float *member_dev, const float *weights, int32_t n_sources,
                              int64_t n_samples, int32_t first, void *stream);
int asx_ht_bag_finish_dev(asx_engine *e, const float *est_dev, const float *totals, int32_t n_sources, const float *mix_dev,
                          int64_t n_samples, uint32_t flags, float *out_dev, void *stream);

/* Writer edge: spec_utils.normalize + (stem * 32767).astype(np.int16) + channel interleave of
 * CommonSeparator.write_audio_pydub (common_separator.py:309-337).  stem [2, N] planar -> pcm [N, 2]; bit-exact.
 * *peak_after (optional) = max |stem| after normalisation: the reference skips the file when it is < 1e-6. */
int asx_pcm16(asx_engine *e, const float *stem_host, int64_t n_samples, float max_peak, float min_peak, int32_t has_min,
              int16_t *pcm_host, float *peak_after);
int asx_pcm16_dev(asx_engine *e, const float *stem_dev, int64_t n_samples, float max_peak, float min_peak, int32_t has_min,
                  int16_t *pcm_dev, float *peak_after, void *stream);

/* The same edge for a stem that is ALREADY [N, 2] interleaved on the device -- the layout asx_separate_dev writes and
 * write_audio receives (common_separator.py:330-337) -- so that a file-level caller never brings the float stem to the host:
 * stem_rows [N, 2] -> pcm [N, 2]; bit-identical to asx_pcm16 on the transposed array.  (ABI 4) */
int asx_pcm16_rows_dev(asx_engine *e, const float *stem_rows_dev, int64_t n_samples, float max_peak, float min_peak, int32_t has_min,
                       int16_t *pcm_dev, float *peak_after, void *stream);

/* FLAC encoder for the writer edge (RFC 9639; CommonSeparator.write_audio_pydub with a .flac path): interleaved int16 [n, 2] -> the audio
 * frames of a fixed-blocksize, 2-channel stream, lossless.  bits_per_sample 16, or 24 = every value shifted left by 8 with the wasted
 * bits flagged per subframe (what ffmpeg's -sample_fmt s32 makes of 16-bit input).  Per block: constant, verbatim, fixed orders 0..4 and
 * LPC orders 1..8 at 15-bit coefficients per candidate channel, exact Rice bits for partition orders 0..6 (method 0, no escapes), the
 * cheapest of L/R, L/S, S/R and M/S.  Runs of one input are byte-identical.  The caller writes "fLaC" and STREAMINFO.
 *   asx_flac_plan        pure host: frames, the stride of the per-frame scratch slots (the worst case of a frame: header + 2 x (16 + 17 x
 *                        block_size) bits + padding + CRC-16, rounded up to 16), the worst case of the output and the engine scratch the call
 *                        will hold (any out pointer may be NULL).  ASX_ERR_INVALID + asx_last_error() for channels != 2, bits_per_sample
 *                        other than 16 / 24, block_size outside 16 .. 4608 and n_samples < 1.
 *   asx_flac_encode_dev  pcm16_dev [n, 2] -> out_dev: the frames back to back; frame_bytes_dev [n_blocks] int32: their sizes;
 *                        *total_bytes: their sum.  out_capacity >= the plan's max_bytes.  Every argument is checked before anything is
 *                        enqueued; the call synchronises `stream` once, for the total.
 *   asx_flac_encode      the same for host arrays.
 * With the profile on (asx_profile_enable) lane 0 of every block stamps the shader clock; asx_counter "flac_block_cycles" and
 * "flac_crc16_cycles" are the sums over all blocks this engine has encoded that way: the whole block, and its CRC-16 phases.
 * Additive within ABI 7. */
int asx_flac_plan(int64_t n_samples, int32_t channels, int32_t bits_per_sample, int32_t block_size, int64_t *n_blocks, int32_t *frame_stride,
                  int64_t *max_bytes, int64_t *scratch_bytes);
int asx_flac_encode_dev(asx_engine *e, const int16_t *pcm16_dev, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample, int32_t block_size,
                        uint8_t *out_dev, int64_t out_capacity, int32_t *frame_bytes_dev, int64_t *total_bytes, void *stream);
int asx_flac_encode(asx_engine *e, const int16_t *pcm16_host, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample, int32_t block_size,
                    uint8_t *out_host, int64_t out_capacity, int32_t *frame_bytes_host, int64_t *total_bytes);

/* The same encoder for samples of 16 or 24 REAL bits (CommonSeparator.write_audio_soundfile with a .flac path, where the reference's
 * sf.write keeps a PCM_24 input's width): interleaved int32 [n, 2], every value inside bits_per_sample bits (the host form checks, the device
 * form trusts its caller).  No wasted bits; the side channel is L - R at bits_per_sample + 1, the mid channel (L + R) >> 1.  Against the int16
 * form: exact Rice bits for the parameters 0 .. 23 at partition orders 0 .. 5; a subframe takes Rice method 1 (5-bit parameters) only where
 * that is smaller than method 0 restricted to 0 .. 14; a predictor with a residual outside 32 bits is no candidate.  The worst case of a
 * frame, hence stride and max_bytes, is header + 2 x (16 + (bits_per_sample + 1) x block_size) bits + padding + CRC-16.  Arguments, refusals
 * and outputs as for asx_flac_plan / asx_flac_encode_dev / asx_flac_encode.  Additive within ABI 7. */
int asx_flac_plan_pcm(int64_t n_samples, int32_t channels, int32_t bits_per_sample, int32_t block_size, int64_t *n_blocks, int32_t *frame_stride,
                      int64_t *max_bytes, int64_t *scratch_bytes);
int asx_flac_encode_pcm_dev(asx_engine *e, const int32_t *pcm_dev, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample,
                            int32_t block_size, uint8_t *out_dev, int64_t out_capacity, int32_t *frame_bytes_dev, int64_t *total_bytes,
                            void *stream);
int asx_flac_encode_pcm(asx_engine *e, const int32_t *pcm_host, int64_t n_samples, int32_t sample_rate, int32_t bits_per_sample, int32_t block_size,
                        uint8_t *out_host, int64_t out_capacity, int32_t *frame_bytes_host, int64_t *total_bytes);

/* Writer edge of CommonSeparator.write_audio_soundfile (common_separator.py:399-461) for a stem in HBM: spec_utils.normalize exactly as
 * asx_normalize_dev computes it, then the samples in the file's own format, interleaved [n, 2] -- the body of a WAVE data chunk.
 *   stem_dev       float32, planar [2, n] (ASX_STEM_PLANAR) or rows [n, 2] (ASX_STEM_ROWS); only read
 *   sample_format  16, 24 (3-byte packed), 32: little-endian integer PCM = clip(rint((double)x * (2^(b-1) - 1)), -2^(b-1), 2^(b-1) - 1), ties
 *                  to even (audio_io.write_wav's rule and libsndfile's scale factor; not asx_pcm16's truncating x * 32767);
 *                  0x120: float32, the normalised value; ASX_PCM_S16_IN_32 / ASX_PCM_S24_IN_32: the 16- / 24-bit integers in int32
 *                  containers, the input of asx_flac_encode_pcm_dev
 *   out_dev        n x 4, 6 or 8 bytes, 16-byte aligned
 *   *peak_after    (optional; synchronises) max |stem| after normalisation, float32: the writer skips the file below 1e-6
 * Non-finite samples are outside the contract.  Every argument is checked before anything is enqueued (ASX_ERR_INVALID + asx_last_error():
 * null pointers, n_samples < 1, unknown layout, unknown format).  asx_pcm_encode: the same for host arrays.  Additive within ABI 7. */
#define ASX_PCM_S16_IN_32 0x410
#define ASX_PCM_S24_IN_32 0x418
int asx_pcm_encode_dev(asx_engine *e, const float *stem_dev, int64_t n_samples, int32_t layout, float max_peak, float min_peak, int32_t has_min,
                       int32_t sample_format, void *out_dev, float *peak_after, void *stream);
int asx_pcm_encode(asx_engine *e, const float *stem_host, int64_t n_samples, int32_t layout, float max_peak, float min_peak, int32_t has_min,
                   int32_t sample_format, void *out_host, float *peak_after);

/* FLAC decoder for the input edge (RFC 9639): the audio part of a native FLAC stream -- everything behind the last metadata block, already in
 * HBM -- -> the planar float32 mix [2, n] = x / 2^(bits_per_sample - 1), which is what librosa.load / libsndfile give for the file at its own
 * rate (a mono stream feeds both rows).  The arguments are STREAMINFO's fields.  Taken: 1 or 2 channels, 8 .. 24 bits per sample, fixed or
 * variable block sizes up to 16384, any sample rate.  A stream has no frame index and the sync code also occurs inside frames, so: every
 * byte position whose header passes all checks (its CRC-8 included) becomes a candidate; every candidate is decoded, one wave each, with its
 * CRC-16; the host keeps the chain of valid candidates that follow each other from byte 0 and drops the rest; the chain's frames are
 * converted.  The chain ends at the end of the data or at the first frame that is damaged or cut: *bytes_consumed < audio_bytes tells.  The
 * frame CRCs are the integrity check (STREAMINFO's MD5 and total_samples are not used).
 *   asx_flac_decode_plan        pure host: the capacity of the candidate list (audio_bytes / 5 + 1: two headers are at least 5 bytes apart),
 *                               the bytes of one candidate's slot and the fixed scratch; the slots of the candidates found come on top (any
 *                               out pointer may be NULL).  ASX_ERR_INVALID + asx_last_error() for 32-bit (or any width outside 8 .. 24)
 *                               streams, more than two channels, a maximum block size outside 16 .. 16384 and empty input.
 *   asx_flac_decode_scan_dev    sync, frame decode and chain walk; *n_samples (may be 0), *n_frames, *bytes_consumed.  The decoded frames stay
 *                               in engine scratch.  audio_dev is 4-byte aligned.  Synchronises `stream` twice (the candidate count sizes the
 *                               slots; the records feed the walk).
 *   asx_flac_decode_finish_dev  the frames of the last scan -> mix_dev [2, n_samples]; *peak (optional, synchronises) = max |mix|.
 *                               ASX_ERR_INVALID unless a scan on this engine came before it and found n_samples >= 1 samples.
 *   asx_flac_decode             the same for host arrays; mix_host holds [2, *n_samples], at most `capacity` samples per row (ASX_ERR_INVALID
 *                               with *n_samples set when the stream holds more).
 * Every argument is checked before anything is enqueued.  Additive within ABI 7. */
int asx_flac_decode_plan(int64_t audio_bytes, int32_t channels, int32_t bits_per_sample, int32_t max_blocksize, int32_t max_framesize,
                         int64_t *max_candidates, int64_t *slot_bytes, int64_t *scratch_bytes);
int asx_flac_decode_scan_dev(asx_engine *e, const uint8_t *audio_dev, int64_t audio_bytes, int32_t sample_rate, int32_t channels,
                             int32_t bits_per_sample, int32_t max_blocksize, int32_t max_framesize, int64_t *n_samples, int64_t *n_frames,
                             int64_t *bytes_consumed, void *stream);
int asx_flac_decode_finish_dev(asx_engine *e, float *mix_dev, int64_t n_samples, float *peak, void *stream);
int asx_flac_decode(asx_engine *e, const uint8_t *audio_host, int64_t audio_bytes, int32_t sample_rate, int32_t channels, int32_t bits_per_sample,
                    int32_t max_blocksize, int32_t max_framesize, float *mix_host, int64_t capacity, int64_t *n_samples, int64_t *n_frames,
                    int64_t *bytes_consumed, float *peak);

/* Decode edge (common_separator.py:217-282 prepare_mix -> librosa.load -> libsndfile): the `data` chunk of a RIFF/WAVE file,
 * [frames, channels] interleaved little-endian samples already copied to the device, -> float32 planar mix [2, frames]
 * (a mono file feeds both rows, :278-280; channels beyond the second are ignored).  sample_format: 16 / 24 / 32 = integer
 * PCM bits (x / 2^(bits-1), PCM_32 through double like libsndfile), 0x120 = IEEE float32.  *peak (optional, synchronises)
 * = max |mix|: prepare_mix raises on a silent file (:268-271).  (ABI 4) */
int asx_pcm_decode_dev(asx_engine *e, const void *raw_dev, int64_t frames, int32_t channels, int32_t sample_format, float *mix_dev,
                       float *peak, void *stream);

/* spec_utils.normalize(wave, max_peak, min_peak) (uvr_lib_v5/spec_utils.py:99-115) in place on any float32 array of
 * `numel` values (MDXCSeparator.separate applies it to the mix and to every stem, mdxc_separator.py:147,170-190);
 * *peak_before (optional) = max |wave| before scaling.  has_min_peak = 0 mirrors min_peak=None. */
int asx_normalize(asx_engine *e, float *wave_host, int64_t numel, float max_peak, float min_peak, int32_t has_min, float *peak_before);

/* The same on an array already in HBM, in place, no host synchronisation (ABI 4); and the residual stem of a single-target
 * MDXC / Roformer model, out = mix - stem (mdxc_separator.py:406-468). */
int asx_normalize_dev(asx_engine *e, float *wave_dev, int64_t numel, float max_peak, float min_peak, int32_t has_min, void *stream);
int asx_residual_dev(asx_engine *e, const float *mix_dev, const float *stem_dev, float *out_dev, int64_t numel, void *stream);

/* Spectral edges, librosa STFT(2048, 1024) semantics:
 * asx_ensemble   = Ensembler.ensemble (audio_separator/separator/ensembler.py:12-160) over K equal-length stereo waves
 *                  [K, 2, N]; algorithm: 0 avg_wave, 1 median_wave, 2 min_wave, 3 max_wave, 4 avg_fft, 5 median_fft,
 *                  6 min_fft, 7 max_fft, 8 uvr_max_spec, 9 uvr_min_spec, 10 ensemble_wav (spec_utils.py:1245-1266: each
 *                  channel from the input with the smallest mean |x|); weights [K] (avg_* only) or NULL; out [2, *n_out]
 *                  (*n_out = N, or 1024 * (N / 1024) for the uvr_* algorithms, which do not pass a length to istft).
 * asx_invert_stem = spec_utils.invert_stem(mixture, stem) (uvr_lib_v5/spec_utils.py:573-580), planar [2, *n_out],
 *                  *n_out = 1024 * (N / 1024).
 * 2 <= K <= 8 and N >= 1, else ASX_ERR_INVALID.  *n_out = 0 (N < 1024 for uvr_* and asx_invert_stem) is a result, not an
 * error: nothing is launched or written and the call returns ASX_OK, as the reference returns an empty array there.
 * Outside the parity domain: ensemble_wav compares sums of |x| held in float64, numpy's means are float32 sums; two
 * inputs whose channel means agree to float32 rounding but not exactly may be ranked differently (the engine by the
 * float64 sums).  Exactly equal sums keep the first input, as np.argmin does. */
int asx_ensemble(asx_engine *e, const float *waves_host, int32_t k, int64_t n_samples, int32_t algorithm, const double *weights,
                 float *out_host, int64_t *n_out);
int asx_ensemble_dev(asx_engine *e, const float *waves_dev, int32_t k, int64_t n_samples, int32_t algorithm, const double *weights,
                     float *out_dev, int64_t *n_out, void *stream);
int asx_invert_stem(asx_engine *e, const float *mix_host, const float *stem_host, int64_t n_samples, float *out_host, int64_t *n_out);

/* The edge between one ensemble member and asx_ensemble_dev (separator.py:1286, :1335; ensembler.py:29-30): what the member's
 * stem becomes on its way through write_audio and librosa.load, written into slot k of a device stack [K, 2, n_max].
 *   stem_dev   the stem as a plugin leaves it: planar [2, n] (ASX_STEM_PLANAR) or rows [n, 2] (ASX_STEM_ROWS), float32
 *   mode       ASX_SLOT_PCM16:   slot[c, i] = (float)q[i, c] / 32768 with q the int16 asx_pcm16_dev / asx_pcm16_rows_dev write
 *                                for the same stem and thresholds (bit for bit); *peak_after as those calls return it
 *              ASX_SLOT_FLOAT32: slot[c, i] = stem value, no normalisation, no quantisation; *peak_after = max |stem|
 *              ASX_SLOT_FILE_PCM16 / _PCM24 / _PCM32 / _FLOAT: the round trip of a member that writes with soundfile
 *                                (write_audio_soundfile + audio_io.load): slot = the float32 array asx_pcm_decode_dev returns for the
 *                                bytes asx_pcm_encode_dev writes for the same stem, layout and thresholds in that sample format, bit
 *                                for bit -- spec_utils.normalize, then clip(rint((double)x * (2^(b-1) - 1))) read back as
 *                                int / 2^(b-1), or the normalised float itself; *peak_after as asx_pcm_encode_dev reports it.  The
 *                                values are that call's sample_format codes.  ASX_SLOT_FILE_PCM16 rounds where ASX_SLOT_PCM16
 *                                (pydub's writer) truncates: they are different modes.
 *   padding    slot[c, i] = 0 for n <= i < n_max, written by this call: the stack need not be cleared
 * Requires 0 <= n <= n_max (stem_dev may be NULL when n == 0), n_max >= 1, k >= 0; the caller owns a stack of at least
 * (k + 1) * 2 * n_max floats.  peak_after may be NULL (then the call only enqueues work).  Additive to ABI 7; the file modes are
 * additive within ABI 8. */
#define ASX_STEM_PLANAR 0
#define ASX_STEM_ROWS 1
#define ASX_SLOT_PCM16 0
#define ASX_SLOT_FLOAT32 1
#define ASX_SLOT_FILE_PCM16 16
#define ASX_SLOT_FILE_PCM24 24
#define ASX_SLOT_FILE_PCM32 32
#define ASX_SLOT_FILE_FLOAT 0x120
int asx_ensemble_slot_dev(asx_engine *e, const float *stem_dev, int64_t n_samples, int32_t layout, float max_peak, float min_peak,
                          int32_t has_min, int32_t mode, float *stack_dev, int32_t k, int64_t n_max, float *peak_after, void *stream);

/* The ensembles of many (file, stem group) jobs in one call: per job exactly what asx_ensemble_slot_dev for each contributor
 * followed by asx_ensemble_dev over the stack gives (bit for bit), with one launch per stage over all jobs, no stack in memory
 * and one wait of the host (for the peaks).
 *   peaks      peak_after[c] is what asx_ensemble_slot_dev reports for contributor c under `mode` and the thresholds
 *   live set   a contributor with (double)peak_after < silent_below takes no part (its 16-bit file would not have been written); the
 *              others are zero padded to the longest of THEM (n_max); live = how many took part
 *   result     live == 0: none (n_out = 0, out_dev untouched); live == 1: that contributor's slot image (n_out = its n);
 *              else asx_ensemble_dev's: n_out = n_max, or 1024 * (n_max / 1024) for the uvr_* algorithms (0, and nothing
 *              written, below two frames).  out_dev receives planar [2, n_out] and nothing beyond 2 * n_out floats.
 *   weights    [n_weights] or NULL, for avg_* only: a job with live == n_weights gives weights[i] to its i-th live contributor,
 *              any other job uses equal weights -- what Ensembler.ensemble does with a weights list (ensembler.py:32-44)
 * Every argument of every job is checked before anything is enqueued; the message names the job.  n_jobs == 0 does nothing.
 * At most ASX_ENS_MAX_JOBS jobs per call.  Additive to ABI 7.
 *
 * asx_ensemble_batch_modes_dev: the same call with the slot mode a property of each contributor -- the members of one ensemble can
 * write the same file's stems in different formats (one with soundfile beside one without: PCM_24 beside pcm16; a FLOAT input that
 * one member writes as FLOAT and another as PCM_32).  modes[j * ASX_ENS_MAX_K + c] is the ASX_SLOT_* mode of contributor c of job j
 * (entries from k on are not read); peak_after[c] and the silent_below rule follow that contributor's own mode.  An unknown mode
 * is refused before anything is enqueued, naming the job and the contributor.  asx_ensemble_batch_dev is this call with every
 * mode equal to `mode`.  Additive within ABI 8. */
#define ASX_ENS_MAX_K 8
#define ASX_ENS_MAX_JOBS 8191
typedef struct asx_ens_job {
  int32_t k;                              /* contributors, 1 .. ASX_ENS_MAX_K */
  int32_t live;                           /* written: contributors that took part */
  const float *stem_dev[ASX_ENS_MAX_K];   /* planar [2, n] or rows [n, 2]; may be NULL where n == 0 */
  int64_t n_samples[ASX_ENS_MAX_K];
  int32_t layout[ASX_ENS_MAX_K];          /* ASX_STEM_PLANAR / ASX_STEM_ROWS */
  float *out_dev;                         /* planar, room for [2, out_capacity] */
  int64_t out_capacity;                   /* >= the longest n_samples of the job */
  int64_t n_out;                          /* written: samples per channel of the result; 0 = no result */
  float peak_after[ASX_ENS_MAX_K];        /* written */
} asx_ens_job;
int asx_ensemble_batch_dev(asx_engine *e, asx_ens_job *jobs, int32_t n_jobs, int32_t algorithm, const double *weights, int32_t n_weights,
                           int32_t mode, float max_peak, float min_peak, int32_t has_min, double silent_below, void *stream);
int asx_ensemble_batch_modes_dev(asx_engine *e, asx_ens_job *jobs, int32_t n_jobs, const int32_t *modes, int32_t algorithm, const double *weights,
                                 int32_t n_weights, float max_peak, float min_peak, int32_t has_min, double silent_below, void *stream);

/* Weighted sums of stereo stems that are already in HBM -- the mix-downs of workflow.ChainSeparator ("instrumental + backing vocals").
 * Per job, frame i < n_out and channel, a source shorter than n_out read as zeros behind its end (one longer is read up to n_out):
 *   acc = fl(w_0 * x_0[i]);  acc = fl(acc + fl(w_k * x_k[i])), k = 1 .. K-1 in list order
 * in float32 with one rounding per operation and no contraction: bit for bit the numpy float32 restatement.
 *   src[k].x       float32, planar [2, n] (ASX_STEM_PLANAR) or rows [n, 2] (ASX_STEM_ROWS), 4-byte aligned, only read; may be NULL where n == 0
 *   out            planar [2, n_out] or rows [n_out, 2] (out_layout), 4-byte aligned; must not overlap a source of another layout or offset
 * asx_mixdown_batch_dev serves all jobs with ONE launch and only enqueues work on `stream` (it waits for the previous call's launch on this
 * engine before it reuses the job table, and for nothing of its own).  Accesses are 16 bytes wide wherever a group of four floats is whole
 * and 16-byte aligned; the groups are anchored at the output's alignment.  Every argument of every job is checked before anything is
 * enqueued (ASX_ERR_INVALID + asx_last_error(): k outside 1 .. ASX_MIX_MAX_K, n_out < 1, n < 0, null or misaligned pointers, unknown layouts,
 * a weight that is not finite); n_jobs == 0 does nothing.  asx_mixdown: one job on host arrays (upload, launch, download).
 * Additive within ABI 8. */
#define ASX_MIX_MAX_K 8
typedef struct asx_mix_src {
  const float *x;
  int32_t layout;   /* ASX_STEM_PLANAR / ASX_STEM_ROWS */
  int64_t n;        /* samples per channel, >= 0 */
  float w;
} asx_mix_src;
typedef struct asx_mix_job {
  asx_mix_src src[ASX_MIX_MAX_K];
  int32_t k;        /* sources, 1 .. ASX_MIX_MAX_K */
  float *out;
  int32_t out_layout;
  int64_t n_out;    /* samples per channel of the result, >= 1 */
} asx_mix_job;
int asx_mixdown_batch_dev(asx_engine *e, const asx_mix_job *jobs, int32_t n_jobs, void *stream);
int asx_mixdown(asx_engine *e, const float *const *x_host, const int32_t *layouts, const int64_t *n_samples, const float *weights, int32_t k,
                float *out_host, int32_t out_layout, int64_t n_out);

/* asx_invert_stem with every array in HBM: spec_utils.invert_stem(mix, stem * stem_scale).
 *   mix_dev      planar [2, n_samples], float32, only read
 *   stem_dev     planar [2, n_samples] (ASX_STEM_PLANAR) or rows [n_samples, 2] (ASX_STEM_ROWS, as asx_separate_dev leaves the primary
 *                stem), only read; stem_scale is applied as one float32 multiplication of every sample read (numpy's
 *                primary * compensate), 1.0f changes nothing
 *   out_dev      rows [*n_out, 2], *n_out = 1024 * (n_samples / 1024) <= out_capacity; nothing beyond 2 * *n_out floats is written
 * The call only enqueues work on `stream`: no copy from or to the host, no synchronisation.  *n_out = 0 (n_samples < 1024) is a
 * result: nothing is launched and out_dev may be NULL.  For a planar stem the result is, bit for bit, asx_invert_stem's for the stem
 * multiplied on the host, transposed.  ASX_ERR_INVALID + asx_last_error() for null pointers, n_samples outside 1 .. 2^38, an unknown
 * layout or out_capacity < *n_out, before anything is enqueued.
 *
 * asx_invert_stem_batch_dev: the same for a list of songs of any lengths with ONE launch per stage (frames, fold) over all of
 * them; a song of fewer than 1024 samples takes part in neither and gets n_out = 0.  Every song's result is bit for bit that of
 * asx_invert_stem_dev for that song alone.  Every argument of every song is checked before anything is enqueued or any n_out
 * written; the message names the song.  One table upload from pinned memory per call.  The host does
 * not wait for the work it enqueues; it may wait for the table copy of the previous pooled call on this engine (this one's or
 * asx_ensemble_batch_dev's: they share the staging area and its event).  The first spectral call on an engine, of either form,
 * uploads the window and twiddle tables once.  Additive within ABI 7. */
typedef struct asx_invert_song {
  const float *mix_dev;     /* planar [2, n_samples] */
  const float *stem_dev;    /* planar [2, n_samples] or rows [n_samples, 2] */
  float *out_dev;           /* rows, room for [out_capacity, 2]; may be NULL where n_out == 0 */
  int64_t n_samples;
  int64_t out_capacity;     /* >= 1024 * (n_samples / 1024) */
  int64_t n_out;            /* written */
  int32_t stem_layout;      /* ASX_STEM_PLANAR / ASX_STEM_ROWS */
} asx_invert_song;
int asx_invert_stem_dev(asx_engine *e, const float *mix_dev, const float *stem_dev, int64_t n_samples, int32_t stem_layout, float stem_scale,
                        float *out_dev, int64_t out_capacity, int64_t *n_out, void *stream);
int asx_invert_stem_batch_dev(asx_engine *e, asx_invert_song *songs, int32_t n_songs, float stem_scale, void *stream);

/* Phase fix ("phase swapper"): the STFT magnitudes of a target stem on phases blended towards a source stem's, with every array in HBM.
 * Per channel, with T and S the librosa STFTs (n_fft 2048, hop, periodic Hann, centred, zero padding, 1 + n / hop frames) of the target
 * (n samples) and of the source zero-extended or cut to n, per frame and bin k with z = S conj(T):
 *   delta = atan2(Im z, Re z)   (0 where z == 0);   O_k = T_k (cos(w_k delta) + j sin(w_k delta));   out = istft(O, length = n)
 * -- the blend runs along the shorter arc from the target's phase to the source's: w = 0 keeps the target, w = 1 is |T| S / |S|, w > 1
 * extrapolates.  Only the real parts of bins 0 and 1024 enter the inverse transform.  Im z = fl(S_i T_r) - fl(S_r T_i) without
 * contraction, so source = -target gives delta = +pi in every bin.  A bin whose rotation angle w_k delta is zero is the target's, bit for bit.
 *   bin_weights  host array of ASX_PHASE_BINS floats, w_k for bin k (frequency k * rate / 2048): the engine knows no cutoffs
 *   hop          256, 512 or 1024
 *   target_dev   planar [2, n] (ASX_STEM_PLANAR) or rows [n, 2] (ASX_STEM_ROWS), float32, 4-byte aligned, only read; n >= 1
 *   source_dev   the same for its own n >= 0 (may be NULL where n == 0: a silent source, the result is the target's round trip)
 *   out_dev      planar [2, n] or rows [n, 2], n the target's; must not share a byte with any input or other output of the call (the
 *                source may be the target)
 * asx_phase_fix_batch_dev serves all jobs with ONE launch per stage (frames, fold) and only enqueues work on `stream` (it waits for the
 * previous phase-fix call's launches on this engine before it reuses its tables, and for nothing of its own).  The workspace is
 * 2 * T * 2048 floats per job.  Every job's result is bit for bit that of asx_phase_fix_dev for that job alone (the single form: the same
 * device functions, the job passed by value).  Every argument of every job is checked before anything is enqueued (ASX_ERR_INVALID +
 * asx_last_error(): null or misaligned pointers, unknown layouts, a weight that is not finite, an unknown hop, n outside 1 .. 2^38, a
 * source n outside 0 .. 2^38, more than ASX_ENS_MAX_JOBS jobs, an output that overlaps an input or another output); n_jobs == 0 does
 * nothing.  asx_phase_fix: one job on host arrays (upload, the same launches, download).  Additive within ABI 8. */
#define ASX_PHASE_BINS 1025
typedef struct asx_phase_job {
  const float *target_dev;
  const float *source_dev;
  float *out_dev;
  int64_t n_samples;          /* of the target and of the result, >= 1 */
  int64_t source_n_samples;   /* >= 0 */
  int32_t target_layout;      /* ASX_STEM_PLANAR / ASX_STEM_ROWS */
  int32_t source_layout;
  int32_t out_layout;
  int32_t reserved;           /* ignored */
} asx_phase_job;
int asx_phase_fix_batch_dev(asx_engine *e, const asx_phase_job *jobs, int32_t n_jobs, const float *bin_weights, int32_t hop, void *stream);
int asx_phase_fix_dev(asx_engine *e, const asx_phase_job *job, const float *bin_weights, int32_t hop, void *stream);
int asx_phase_fix(asx_engine *e, const float *target_host, int32_t target_layout, int64_t n_samples, const float *source_host,
                  int32_t source_layout, int64_t source_n_samples, const float *bin_weights, int32_t hop, float *out_host, int32_t out_layout);

/* Launch counters of this process (tests use them to prove which kernel family ran; ABI 6 -- until ABI 5 they travelled through a
 * float of asx_debug_fetch, which stops resolving single launches past 2^24): "tdf3_launches" (split-operand row GEMM, either arithmetic),
 * "tdf3h_launches" (those of them, plain or GATHER mode, that ran the fp16 x 3 arithmetic),
 * "tdf3_gather_launches" (its GATHER mode: channels-last convolutions), "attn6_launches" (attention6_kernel / mha6_kernel),
 * "attn6h_launches" (those of them on the fp16 x 3 arithmetic),
 * "tdf3s_launches" / "attn6s_launches" (additive: those on the single-product arithmetic of option "gemm_f16x1"; each such launch is counted
 * by "tdf3h_launches" / "attn6h_launches" and "tdf3_launches" / "attn6_launches" as well),
 * "wino6_launches" (conv_wino6_kernel: Winograd F(2x2,3x3) on the 16-bit pipe), "wino6h_launches" (those on the fp16 x 3 arithmetic),
 * "conv3h_launches" (ABI 7: conv3h_kernel, the direct fp16 x 3 convolution of the 48-channel level),
 * "conv3h_fin_launches" (those of them in the fused-input form, option "conv_fuse_input": one per net pass where it applies),
 * "tdf_fused_output_launches" (additive: the tdf3_kernel launches in the fused-output form, option "tdf_fuse_output": one per net pass where it applies),
 * "conv3h_tiled_launches" (additive: those of them with a tile-order input or output, option "conv3h_tiled"),
 * "conv3h_merged_dispatches" (additive: dispatches of conv3h_kernel that ran all n output slices of a layer on one input slice, option
 * "conv3h_merge_out"; "conv3h_launches" and "conv3h_tiled_launches" count such a dispatch as its n (output slice, input slice) pairs),
 * "down6_launches" / "up6_launches" (ABI 7: conv_down6_kernel / conv_up6_kernel, the level-change convs on the 16-bit matrix pipe),
 * "hd_rounds" (ABI 7: rounds of chunk groups the Demucs v3 forward has run -- the groups of a round share the BLSTM launches),
 * "vr_net_passes" (ABI 7, additive: passes of the VR net, CascadedASPPNet or CascadedNet, on a batch of patches -- asx_vr_separate_batch_dev runs
 * fewer of them than a loop of asx_vr_separate_dev over the same songs),
 * "v3_net_passes" / "rof_net_passes" (ABI 7, additive: passes of the TFC-TDF v3 net / of the Roformer net on a batch of chunks, single-song calls
 * included -- asx_mdxc_demix_batch_dev / asx_rof_demix_batch_dev run fewer of them than a loop of the single-song call over the same songs),
 * "tdf3_pair_image_launches" (ABI 7: the tdf3_kernel launches that read their x operand as a pair image -- option "gemm_pair_images", experimental builds),
 * "phasefix_launches" (additive within ABI 8: launches of the phase-fix kernels, two -- frames and fold -- per call of either form).
 * ASX_ERR_INVALID for an unknown name. */
int asx_counter(const asx_engine *e, const char *name, int64_t *out);

/* bring-up hook: copy a named engine workspace buffer ("vr.hc", "vr.D0", ...) to the host. */
int asx_debug_fetch(asx_engine *e, const char *name, float *host, int64_t numel);
/* measurement hook: the s_memtime timeline the ASX_TDF2_ABL=16 build of the row GEMM records (8 x uint64 per workgroup). */
int asx_debug_trace(uint64_t *host, int64_t n_u64);

/* ---- stage hooks (host buffers; mirror the reference's own test surface) ---- */
/* STFT.__call__ (stft.py:20): wave [B,2,C] -> spec [B,4,dim_f,C/hop+1]. */
int asx_stft(asx_engine *e, const float *wave_host, int32_t batch, int64_t n_time, float *spec_host);
/* STFT.inverse (stft.py:99): spec [B,4,dim_f,T] -> wave [B,2,hop*(T-1)]. */
int asx_istft(asx_engine *e, const float *spec_host, int32_t batch, int32_t n_frames, float *wave_host);
/* model_run(spek) (mdx_separator.py:123): spec [B,dim_c,dim_f,dim_t] -> same shape. */
int asx_net_forward(asx_engine *e, const float *spec_host, int32_t batch, float *out_host);
/* MDXSeparator.run_model (mdx_separator.py:414): wave [B,2,chunk_size] -> [B,2,chunk_size]. */
int asx_run_model(asx_engine *e, const float *wave_host, int32_t batch, float *out_host, uint32_t flags);

/* Single-layer hooks used by the parity tests (activations [B,C,T,F], F fastest):
 *   op = "conv3x3"  w [cout,cin,3,3]  b [cout]                 -> relu(conv(x)+b)
 *   op = "down"     w [cout,cin,2,2]  b [cout]   stride 2      -> relu(conv(x)+b)         [B,cout,T/2,F/2]
 *   op = "up"       w [cin,cout,2,2]  b [cout]   stride 2, aux = skip [B,cout,2T,2F]  -> relu(convT(x)+b)*skip
 *   op = "conv1x1"  w [cout,cin]      b [cout]
 *   op = "conv3x3_to_tiled" / "conv3x3_tiled" / "conv3x3_from_tiled": "conv3x3" with its output / both sides / its input in conv3h_kernel's tile
 *        order (option "conv3h_tiled": every 48-channel slice laid out by Conv3hCfg::tl_off, csrc/kernels_conv3h.h; the slice's size is the planar
 *        one's) -- the raw buffer goes to or comes from the host.  An error where conv3h_kernel does not take the layer, T % 4 != 0, or a sliced
 *        layer would run with "conv3h_partial_scratch" = 0.
 * `relu` = 0 drops the ReLU of any of them (ABI 6; until ABI 5 only conv1x1 honoured it): the GroupNorm variant of the net runs its
 * convolutions bare.
 *   op = "tdf"      w [n,k] bias [n] with x viewed as rows of length k=F;
 *                   aux0 = scale [C], aux1 = shift [C], aux2 = residual or NULL -> relu(scale*(xW^T+bias)+shift) (+res)
 */
int asx_op_conv(asx_engine *e, const char *op, const float *x_host, int32_t batch, int32_t cin, int32_t t,
                int32_t f, const float *w_host, const float *b_host, int32_t cout, const float *aux_host,
                int32_t relu, float *y_host);
int asx_op_tdf(asx_engine *e, const float *x_host, int32_t batch, int32_t c, int32_t t, int32_t k,
               const float *w_host, const float *bias_host, int32_t n, const float *scale_host,
               const float *shift_host, const float *res_host, float *y_host);
/* (ABI 7) The two linears of a TDF block with a bottleneck, launched the way the net launches them (reference: TFC_TDF.tdf, modules.py:61-70 --
 * Linear(f, f / bn) + norm + ReLU + Linear(f / bn, f) + norm + ReLU, then x + tdf(x)): y = x + relu(scale1 (relu(scale0 (x W0^T) + shift0) W1^T) + shift1)
 * on x [B, c, t, f] viewed as rows of length f, W0 [n8, f], W1 [f, n8], scales / shifts per channel [c].  With option "gemm_pair_images" and shapes
 * the fp16 x 3 row GEMM takes, the bottleneck activations travel between the two launches as a pair image.  h_host (optional, [B, c, t, n8]):
 * the bottleneck activations as fp32 (decoded from the pair image when one was written) -- single-op test hook like asx_op_tdf. */
int asx_op_tdf_block(asx_engine *e, const float *x_host, int32_t batch, int32_t c, int32_t t, int32_t f, const float *w0_host,
                     const float *scale0_host, const float *shift0_host, int32_t n8, const float *w1_host, const float *scale1_host,
                     const float *shift1_host, float *y_host, float *h_host);
/* (ABI 7) One attention launch of the Roformer transformers (bs_roformer.py: Attention.forward -- softmax(q k^T / 8) v, times sigmoid(gate)
 * per (token, head); dim_head 64), through the engine's own launch code (csrc/engine_attn.h) -- single-op test hook like asx_op_tdf.
 * qkv [M, 3 * heads * 64] (q | k | v, head h owning columns [h * 64, h * 64 + 64) of each part, rotary already applied), gate [M, gate_ld]
 * (pre-sigmoid, column h), out [M, heads * 64].  The tokens are the matrix [B, T, Fb] (row (b * T + t) * Fb + f); axis 0 attends along time
 * (one sequence of length T per (b, f)), axis 1 along frequency (one of length Fb per (b, t)).  Rows M > B * T * Fb are padding that no
 * sequence touches.  `exact` 1: libm expf in the softmax; 0: the hardware exp unit.  `out` is read as well as written: its contents are
 * uploaded first, so elements the kernel does not own keep them.
 * variant: "attn2" / "attn2_qw2" / "attn2_db" (attention2_kernel: fp32 MFMA; 64 or 128 queries per workgroup; double-buffered K / V),
 * "attn6" / "attn6_qw2" (attention6_kernel on the bf16 x 6 arithmetic), "attn6h" / "attn6h_qw2" (on the fp16 x 3 arithmetic), or "auto":
 * the kernel the engine picks for this sequence length under its options and environment.  resolved (optional): the index of the variant
 * that ran in the list "auto", "attn2", "attn2_qw2", "attn2_db", "attn6", "attn6_qw2", "attn6h", "attn6h_qw2", "mha", "mha_db", "mha6",
 * "mha6_wide", "mha6h", "mha6h_wide", "hd_local", "attn6s", "attn6s_qw2".  "attn6s" / "attn6s_qw2" (additive, appended to the list): attention6_kernel
 * on the single-product arithmetic of option "gemm_f16x1" (reduced precision); "auto" resolves to them when and only when that option is on.
 * ASX_ERR_INVALID for an unknown variant or one of the other family. */
int asx_op_attention(asx_engine *e, const float *qkv_host, const float *gate_host, int64_t m, int32_t batch, int32_t t, int32_t fb,
                     int32_t axis, int32_t heads, int32_t gate_ld, int32_t exact, const char *variant, float *out_host, int32_t *resolved);
/* (ABI 7) One multi-head attention launch of the HTDemucs transformer (self and cross attention, nq != nk allowed) or of the LocalState
 * of HDemucs / Demucs v3 (decay_host set; demucs.py:197-221) -- through the engine's own launch code, single-op test hook like asx_op_tdf.
 * q [batch * nq, ldq], k [batch * nk, ldk], v [batch * nk, ldv], out [batch * nq, ldo]; head h owns columns [h * dh, h * dh + dh).
 * Scores are q . k / sqrt(dh); with decay logits [batch * nq, ldd] (4 per head, nq == nk) every query gets the slope
 * D = 1/4 sum_f (f + 1) sigmoid(logit_f), the score loses |key - query| * D and the diagonal is set to -100.  `out` is read as well as
 * written (its padding columns beyond heads * dh keep what the caller put there).  variant: "mha" (mha_kernel: fp32 MFMA; dh 48 / 64,
 * with decay 16 / 32 / 48 / 64 / 96), "mha_db" (its double-buffered build, dh 48), "mha6" / "mha6_wide" (mha6_kernel on the bf16 x 6
 * arithmetic, 64 / 128 queries per workgroup; dh 48 / 64, no decay), "mha6h" / "mha6h_wide" (on the fp16 x 3 arithmetic), "hd_local"
 * (hd_local_attn_kernel: decay, 4 heads of dh 4 / 8 / 12 / 24, ldo == heads * dh), or "auto": the engine's rule (the HTDemucs one
 * without decay, the LocalState one with it).  All but "hd_local" need leading dimensions that are multiples of 4.  A variant that is
 * not built for the arguments is ASX_ERR_INVALID, never a launch.  resolved: as in asx_op_attention. */
int asx_op_mha(asx_engine *e, const float *q_host, int64_t ldq, const float *k_host, int64_t ldk, const float *v_host, int64_t ldv,
               const float *decay_host, int64_t ldd, int32_t batch, int32_t nq, int32_t nk, int32_t heads, int32_t dh, int32_t exact,
               const char *variant, float *out_host, int64_t ldo, int32_t *resolved);
/* (ABI 7) Single launches of the recurrent kernels, through the engines' own launch code -- single-op test hooks like asx_op_mha: host
 * buffers, no net needed; every output is read as well as written (its contents are uploaded first, so elements the kernel does not own
 * keep them); a shape the kernels are not built for is ASX_ERR_INVALID, never a launch.
 *
 * asx_op_hd_lstm_layer: the recurrence of one bidirectional nn.LSTM layer of the BLSTM of HDemucs / Demucs v3 (demucs.py:19-66) for n
 * independent sequences of `steps` steps from zero state: h and c are zeroed, then hd_lstm_step_kernel runs `steps` times.
 * xp [steps * n, 2, 4h] (row step * n + sequence; the input projection plus both biases of direction 0 | 1, gate order i, f, g, o),
 * whh [2, 4h, h], out [steps * n, 2h] (forward half | reverse half; the reverse direction walks steps-1 .. 0), c_host (optional)
 * [2, n, h]: the final cell state.  h must be a multiple of 16. */
int asx_op_hd_lstm_layer(asx_engine *e, const float *xp_host, const float *whh_host, int32_t n, int32_t h, int32_t steps, float *out_host,
                         float *c_host);
/* asx_op_hd_lstm_frames: the framing of that BLSTM.  A sequence of t <= 200 frames is one sequence of t steps; a longer one is cut into
 * nfr = ceil(t / 100) frames of 200 steps with stride 100, zero padded.  Rows are sequence-major: row step * ntot + n_off + b * nfr + k
 * for frame k of batch item b, where ntot >= n_off + b * nfr counts the sequences of every group that shares the recurrence launches.
 * dir 0 (hd_lstm_frame_kernel): h [b, t, hdim] -> rows [steps * ntot, hdim]; rows of other groups keep the caller's contents.
 * dir 1 (hd_lstm_unframe_kernel): h [b, t, hdim] += the rows BLSTM.forward stitches (frame 0 gives steps [0, 150), the last [50, 200),
 * the others [50, 150)); h_host is updated.  steps_out / nfr_out (optional): the step and frame counts the engine derives from t. */
int asx_op_hd_lstm_frames(asx_engine *e, int32_t dir, float *h_host, int32_t b, int32_t t, int32_t hdim, int32_t ntot, int32_t n_off,
                          float *rows_host, int32_t *steps_out, int32_t *nfr_out);
/* asx_op_vr_lstm: the recurrence of the LSTMModule of VR 5.1 (layers_new.py:129-149), one vr_lstm_seq_kernel<hs> launch over w frames
 * of b sequences from zero state: xp [w, b, 2, 4 * hs] (as above), whh [2, 4 * hs, hs], out [w, b, 2 * hs].  hs is 4, 8, 16, 32, 64
 * or 128. */
int asx_op_vr_lstm(asx_engine *e, const float *xp_host, const float *whh_host, int32_t w, int32_t b, int32_t hs, float *out_host);
/* asx_op_vr_lstm_layout: the two layout kernels around it.  dir 0 (vr_lstm_in_kernel): channel ch0 of src [b, h, w, ld] -> dst [w, b, h].
 * dir 1 (vr_lstm_out_kernel): src [w, b, h] -> channel ch0 of dst [b, h, w, ld] with channels ch0+1 .. ch0+3 zeroed and every other
 * channel left alone; ld and ch0 must be multiples of 4 with ch0 + 4 <= ld (one 16-byte store per pixel). */
int asx_op_vr_lstm_layout(asx_engine *e, int32_t dir, const float *src_host, int32_t b, int32_t h, int32_t w, int32_t ld, int32_t ch0,
                          float *dst_host);
/* (ABI 7) One gathered-convolution launch of the channels-last nets (HTDemucs, HDemucs / Demucs v3, VR), through ht_gg of
 * csrc/engine_ht.h unchanged -- single-op test hook like asx_op_mha: host buffers, no net needed; y (and nothing else) is read as well
 * as written: its contents are uploaded first, so elements the launch does not own keep them; a descriptor or variant the launch code
 * would not take is ASX_ERR_INVALID, never a launch.
 * x is the view [B, O, I, Cin] at column x_col0 of a tensor [B][x_bs floats] whose pixels are ldc floats apart (x_bs 0: O * I * ldc);
 * output row (b, oo, j), oo < OR (0: O), j < IR, gathers the KO x KI taps at input pixel (oo SO - PO + to DO, j SI - PI + ti DI), zero
 * outside the image.  mode 0 (dense): y view [B, OR, IR, Cout] at column y_col0 of [B][y_bs floats] with rows of ldy floats (y_bs 0:
 * OR * IR * ldy), y = act(conv + bias) (+ res); w [Cout, Cin, KI, KO] (the first kernel axis is the INNER one), bias [Cout].  mode 1
 * (GLU): w [2 Cout, Cin, KI, KO], bias [2 Cout], y = value * sigmoid(gate) (+ res), act must be 0.  mode 2 (ConvTranspose along the
 * inner axis, kernel 2 So, stride So, as two taps: KO 1, KI 2, SO = SI = 1): w [Cin, Cout, 2 So], bias [Cout]; row j scatters to
 * positions So j - crop + r, r < So, of y [B * O, Iout, ldy] (y_bs must be 0), positions outside [0, Iout) dropped; y = act(.) (+ res).
 * res (res = 1; ldr floats per row): the residual -- [B * OR * IR, ldr] for modes 0 / 1, [B * O, Iout, ldr] for mode 2, or with
 * res_mod > 0 (modes 0 / 1) the table [res_mod, ldr] read at row % res_mod.  act: 0 none, 1 ReLU, 2 GELU (erf), 3 tanh, 4 leaky ReLU
 * (0.01), 5 sigmoid, 6 GELU on the fast erf.  Channel counts, strides and column offsets are multiples of 4.  Weights are packed by
 * the engine's own packers (ht_pack_conv / ht_pack_convtr / ht_glu_perm / ht_halo_pack).
 * variant: "auto" = ht_gg's own rule -- with the halo-tile packing the Demucs decoder rewrites and the VR 3x3 layers carry wherever the
 * layer is eligible for it, or without one (no_halo = 1), as the encoder and DConv convolutions are loaded; "gg" / "halo" / "gather" = only gg_kernel / the halo-tile kernel (csrc/kernels_halo.h) / the
 * GATHER mode of the split-operand row GEMM (csrc/kernels_gemm3.h; bf16 x 6 or fp16 x 3 by the options "gemm_bf16x6" / "gemm_f16x3")
 * may run.  resolved (optional, 3 ints): {1 gg / 2 halo / 3 gather, the N tile (gg, halo; 0 for gather), gg_kernel's lowai flag}. */
typedef struct asx_gconv_desc {
  int32_t B, O, I, Cin, ldc, Cout, ldy;
  int32_t KO, KI, DO, DI, PO, PI, SO, SI, OR, IR;
  int32_t x_col0, y_col0;
  int32_t mode, act;
  int32_t res, ldr, res_mod;
  int32_t Iout, crop, So;
  int32_t no_halo;
  int64_t x_bs, y_bs;
} asx_gconv_desc;
int asx_op_gconv(asx_engine *e, const asx_gconv_desc *d, const float *x_host, const float *w_host, const float *b_host,
                 const float *res_host, const char *variant, float *y_host, int32_t *resolved);
/* (ABI 7) One DConv layer of the Demucs encoders (demucs.py:99-179) through ht_dconv_layer of csrc/engine_ht.h -- single-op test hook
 * like asx_op_gconv -- on y [b, o, i, c] channels-last, in place: part 1 = conv k3 with dilation 2^d (along the outer axis when
 * along_outer, else the inner) + GroupNorm(1, hid) + GELU -> h [b * o * i, hp = hid rounded up to 4]; part 2 = conv 1x1 +
 * GroupNorm(1, 2 c) + GLU + LayerScale, added into y; 3 = both.  GroupNorm runs per (b, i) over (o, c) when along_outer (the
 * spectrogram branch), else per b over (o, i, c).  Torch tensors: w1 [hid, c, 3], b1 [hid], g1w / g1b [hid], w2 [2 c, hid], b2 [2 c],
 * g2w / g2b [2 c], ls [c].  h_host [b * o * i, hp]: uploaded first; the result of part 1, the input of part 2 alone; may be NULL for
 * part 3.  The workspace ht_dconv_layer reads (h, the per-row partial sums, the float64 group sums, (mean, rstd), the arrival
 * counters) is built for exactly this case.  ticket_left (optional): how many arrival counters are non-zero afterwards. */
int asx_op_dconv(asx_engine *e, float *y_host, int32_t b, int32_t o, int32_t i, int32_t c, int32_t hid, int32_t along_outer, int32_t d,
                 int32_t part, const float *w1, const float *b1, const float *g1w, const float *g1b, const float *w2, const float *b2,
                 const float *g2w, const float *g2b, const float *ls, float *h_host, int32_t *ticket_left);
/* (ABI 8) Single launches of the STFT / iSTFT kernels, through the engines' own launch helpers (stft_launch; istft_launch + ola_launch
 * or istft_ola_launch, csrc/engine_mdx.h) and the argument builders the nets use (csrc/engine_v3.h, csrc/engine_rof.h) -- single-op
 * test hooks like asx_op_gconv: host buffers in and out; the output buffer is uploaded first, so elements the launch does not own keep
 * their contents.  n_fft, hop_length, dim_f, win_length, the window (asx_set_stft_window) and whether the 6144 / 1024 fast path is on
 * come from the engine; the descriptor carries the rest:
 *   b, t: chunks and frames per chunk; c: samples per chunk (n_fft / 2 < c, and (t - 1) hop + n_fft / 2 - 1 <= 2 (c - 1) so that one
 *     reflection suffices, forward; 1 <= c <= hop (t - 1), inverse).
 *   layout: 0 = [b, 4, F, t]; 1 = [b, 4, t, F]; 2 = the Roformers' `b t (f s c)` (the inverse multiplies by mask_host [b, n_inst, t, F, 2, 2]).
 *   subbands (layout 1): 0 = the MDX chunk loop's launch, which takes the fast path where the engine has it; k >= 1 = the TFC-TDF v3
 *     launch: plane p of k F / k-bin subbands, always the generic kernels.  bstride: floats between batch items of the spectrum
 *     (layout 1 with subbands >= 1; 0 = dense).  n_inst (inverse): S stems per batch item, b * S spectra in all.
 *   zero_low, sign (forward); combine (inverse: 1 = 0.5 spec[i] - 0.5 spec[i + b], the spectrum holds 2 b items).
 *   stft_normalized (layout 2): the forward scales by n_fft^-1/2 and the inverse takes the synthesis window x n_fft^1/2.
 *   mode (forward): 0 = wave_host is [b, 2, c]; 1 = one song [2, song_len[0]], chunk i starting at padded position starts[i], `front`
 *     zeros in front of the song; 2 = a pool of n_songs songs, wave_host their [2, song_len[s]] arrays one after the other, chunk i a
 *     window of song song_of[i] (the *_pool_kernel twins).
 *   n_act (inverse; NULL = none): per chunk, >= 0 = np.hanning(n_act) over the first n_act samples and zeros behind them, < 0 = none.
 *   spec_floats: floats of spec_host.
 * resolved (optional, 2 ints): {what ran -- 1 stft, 2 stft_pool, 3 stft3, 4 stft3_pool, 5 stft3p, 6 stft3p_pool, 7 istft + ola,
 * 8 istft3, 9 istft3p --, seam3_kernel launches}. */
typedef struct asx_stft_desc {
  int32_t b, t;
  int32_t layout, subbands, zero_low, n_inst, combine, stft_normalized;
  int32_t mode, front, n_songs;
  float sign;
  int64_t c, bstride, spec_floats;
  const int64_t *starts;
  const int32_t *song_of;
  const int64_t *song_len;
  const int64_t *n_act;
} asx_stft_desc;
int asx_op_stft(asx_engine *e, const asx_stft_desc *d, const float *wave_host, float *spec_host, int32_t *resolved);
/* wave_host [b * max(n_inst, 1), 2, c] */
int asx_op_istft(asx_engine *e, const asx_stft_desc *d, const float *spec_host, const float *mask_host, float *wave_host, int32_t *resolved);
/* (ABI 8) The spectrogram launches of the Demucs nets (csrc/kernels_ht.h), as csrc/engine_ht.h / engine_hd.h launch them -- plan, window,
 * per-hop envelope and LDS grant from the same builders; no network needs to be loaded.  asx_op_ht_spec: one ht_stft_kernel launch,
 * seg_host [b, 2, l] -> spec_host [b, t = ceil(l / hop), nfft / 2, 2, 2] with hop = nfft / 4; el / lv: pad1d's zero extension (el zeros
 * in front, lv samples in all; 0 / l for none).  asx_op_ht_ispec: ht_istft_kernel + ht_ola_kernel, x_host [b, t, nfft / 2, 4 s] and
 * xt_host [b, l, 2 s] -> out_host [b, s, 2, l]; acc_f / acc_t [b, 2]: the float64 (sum, sum of squares) pairs the kernels de-standardise
 * with, over n_stat values of the spectrogram and 2 l samples of the waveform. */
int asx_op_ht_spec(asx_engine *e, int32_t nfft, const float *seg_host, int32_t b, int64_t l, int64_t el, int64_t lv, float *spec_host);
int asx_op_ht_ispec(asx_engine *e, int32_t nfft, const float *x_host, int32_t b, int32_t t, int32_t s, const double *acc_f, double n_stat,
                    const float *xt_host, const double *acc_t, int64_t l, float *out_host);
/* (ABI 8) Single launches of the normalisation and statistics kernels, through the engines' own launch helpers -- single-op test hooks
 * like asx_op_dconv / asx_op_stft: host buffers in and out; the output buffer is uploaded first, so elements the launch does not own
 * keep their contents; no network needs to be loaded; arguments the launch code would not take are ASX_ERR_INVALID, never a launch.
 *
 * asx_op_rownorm: one row normalisation over x_host [m, lda], by kind:
 *   "rms"         rof_rmsnorm (csrc/engine_rof.h): y_host [m, ldy] = x / max(||x||, 1e-12) sqrt(d) gamma_host [d] on the first d columns.
 *                 in_place: one device buffer, uploaded from x_host, is both x and y (lda == ldy); y_host receives it.
 *   "rms_factor"  rof_rownorm: y_host [m] = sqrt(d) / max(||x||, 1e-12); gamma_host, ldy unused.
 *   "layer"       ht_ln (csrc/engine_ht.h): LayerNorm(d), eps 1e-5, gamma_host / beta_host [d], dense rows (lda == ldy == d), plus
 *                 pos_host [pos_mod, d] read at row % pos_mod when not NULL. */
int asx_op_rownorm(asx_engine *e, const char *kind, const float *x_host, int64_t m, int32_t d, int64_t lda, const float *gamma_host,
                   const float *beta_host, const float *pos_host, int64_t pos_mod, int32_t in_place, float *y_host, int64_t ldy);
/* asx_op_group_stats: ht_stats (csrc/engine_ht.h) with its own arguments.  x_host [g1, r, p]; plane element i belongs to group
 * i / gdiv of g2 and counts when i % ld < cn; acc_host [g1, g2, 2] receives the float64 (sum, sum of squares) pairs.  Shapes that need
 * more than the kernel's 66 group slots per workgroup are refused. */
int asx_op_group_stats(asx_engine *e, const float *x_host, int32_t g1, int64_t r, int64_t p, int64_t gdiv, int32_t ld, int32_t cn,
                       int32_t g2, double *acc_host);
/* asx_op_group_norm: statistics + apply as the nets launch them, by family (fields of the descriptor a family does not name are ignored):
 *   "ht"       ht_stats + ht_gn mode 2, the HTDemucs norm_out: GroupNorm(1, c) per item over x_host [b, r, c] -> y_host [b, r, c].
 *   "hd"       the core of hd_group_norm (csrc/engine_hd.h): GroupNorm(g, c) over x_host [b, rin, c] (rin = 0: rin = r), y_host
 *              [b, r, ce] = rows [r0, r0 + r); mode 0 gelu(norm) / 1 GLU over channel halves (ce = c / 2) / 2 norm; aux_host
 *              [b, r, ce] (optional): the skip added last.  in_place (mode 0 / 2, rin = r): one device buffer is x and y.
 *   "std"      ht_stats + std_norm_kernel: x_host [b, r, c] (r frames of c = 4 F floats) -> (x - mean) / (1e-5 + std), unbiased.
 *   "time"     ht_stats + time_norm_kernel: x_host [b, 2, p] -> y_host [b, p, 2], same formula over the 2 p samples of an item.
 *   "hd_time"  ht_stats + hd_time_norm_kernel: y_host [b, p rounded up to even, 2], the pad sample zero.
 *   "v3"       the core of v3_norm_act (csrc/engine_v3.h): norm as asx_v3_config.norm, act 0 relu / 1 gelu / 2 elu(alpha); the input is
 *              the view of channels [c0, c0 + c) of x_host [b, ctot, p]; y_host [b, c, p]; gamma_host / beta_host [c] (BatchNorm: the
 *              folded scale / shift; None: unused); stats_host [b, c, 2] (optional) receives the (mean, rstd) table.
 *   "mdx"      gn_launch (csrc/engine_mdx.h): GroupNorm(2, c) + ReLU over x_host [b, c, p], then + aux_host, then * mul_host (both
 *              optional, [b, c, p]); in_place: one device buffer is x and y. */
typedef struct asx_group_norm_desc {
  int32_t b, c, g, mode;
  int32_t norm, act, ctot, c0;
  int32_t in_place;
  float alpha;
  int64_t r, rin, r0, p;
} asx_group_norm_desc;
int asx_op_group_norm(asx_engine *e, const char *family, const asx_group_norm_desc *d, const float *x_host, const float *gamma_host,
                      const float *beta_host, const float *aux_host, const float *mul_host, float *y_host, float *stats_host);

/* ---- options ------------------------------------------------------------ */
/* Engine options.  Each engine takes its defaults from the environment variable named beside the option when it is created (values go
 * through the same normalisation as asx_set_option); asx_set_option changes one for this engine only.
 * "winograd": kernel of the 3x3 / pad-1 TFC convolutions.  3 (default; also ASX_WINOGRAD in the environment) = Winograd
 * F(2x2,3x3) in fp32 (2.25x fewer multiply-accumulates; results differ from the direct kernel by a few float32 ulps per
 * layer, whole-song deviation from the CPU oracle stays below 1e-5 relative RMS, profiles/r03_fullsong_parity.json);
 * 0 = the direct MFMA kernel; 1 / 2 = earlier Winograd generations kept for A/B measurements, in experimental builds only (the default
 * library refuses them from asx_set_option, and reads any positive ASX_WINOGRAD as 3).
 * "winograd_stationary" (experimental builds only -- the default library accepts 0 and refuses 1): 1 (also ASX_WINOS) = layers with at most 96 input channels run the weight-stationary form of the same
 * transform (csrc/kernels_winos.h: the transformed weights stay in registers, positions split over eight waves) when "winograd"
 * is 3; 0 (default: the stationary form measured slower, profiles/NOTES.md) = conv_wino3_kernel for every layer.
 * "winograd_bf16x6" (ABI 6; also ASX_WINO6): minimum input-channel count from which a 3x3 TFC convolution runs Winograd F(2x2,3x3) on the
 * bf16 matrix pipe (conv_wino6_kernel, csrc/kernels_wino6.h: the sixteen transform-domain GEMMs as six bf16 MFMA products on exactly
 * split operands -- the arithmetic of "gemm_bf16x6", which must be on) instead of conv_wino3_kernel; needs "winograd" = 3.  Default 144
 * (levels 2 .. 5 of the HQ_3 net: measured 1.08-1.24x faster there, equal at 96 channels, slower at 48); 0 = never.
 * "conv_direct_f16x3" (ABI 7; also ASX_CONV3H): a channel-count threshold.  N > 0 (default 144) = a 3x3 TFC convolution of 48n -> 48n channels
 * with 48n <= N (at most 144: the weight image is packed up to 144 channels) on planes whose width is a multiple of 32 (levels 0, 1 and 2 of
 * the HQ_3 geometry) runs conv3h_kernel (csrc/kernels_conv3h.h): a DIRECT implicit GEMM on the fp16
 * matrix pipe with the arithmetic of "gemm_f16x3" (which must be on, as "gemm_bf16x6" and "winograd" = 3) -- the two-part weight image stays in
 * LDS for the whole launch, producer waves fetch four input rows per step into a ring walked down T and split them under one
 * power-of-two exponent per four-row block, consumer waves multiply; n x n launches over 48-channel slices; 5.3-5.8 ms per launch of 55 chunks against
 * 8.5-8.9 on conv_wino3_kernel at 48 channels.  0 = never (conv_wino3_kernel / conv_wino6_kernel).
 * "conv_fuse_input" (an option only, no environment variable): 1 (default) = where the first 3x3 TFC convolution of a BatchNorm ConvTDFNet runs
 * conv3h_kernel at 48 channels, its producer waves compute the net's 1x1 input convolution (4 -> 48 channels, folded BatchNorm, ReLU) themselves
 * from the four spectrogram planes: no launch of its own, no 48-channel activation written to memory and read back.  0 = two launches.  A
 * GroupNorm net, another width or another 3x3 kernel: two launches either way.
 * "tdf_fuse_output" (an option only, no environment variable): 1 (default) = the net's 1x1 output convolution (48 -> 4 channels, no activation) is
 * computed in the epilogue of the last TDF block's second linear: that launch runs tdf3_kernel on channel-grouped row tiles (all 48 channels of
 * four consecutive frames of one batch item per 192 x 128 tile), sums w_out[oc][c] * (relu(...) + x) over the channels in registers and two
 * cross-lane steps, and writes the four output planes -- the block's 48-channel output is never written to memory and read back, and the conv has
 * no launch of its own.  One fixed summation order: two runs give the same bits; the result differs from the two launches' in the last bits (the
 * conv's sum runs in another order), a NaN stays inside its (batch item, frame).  0 = two launches.  Applies to a BatchNorm ConvTDFNet with a
 * bottleneck whose last block has 48 channels, dim_t % 4 == 0 and dim_f % 128 == 0 and whose second linear runs the "gemm_f16x3" row GEMM; a
 * GroupNorm net, another width, a ragged dim_t, "gemm_f16x3" = 0 or the TFC-TDF v3 nets: two launches either way, bit for bit as with 0.
 * "conv3h_partial_scratch" (an option only, no environment variable): how the n launches that make one 48-channel output slice of a 96- or
 * 144-channel conv3h_kernel layer hand their partial sum on.  1 (default) = through a private scratch buffer of the engine in the consumer
 * waves' fragment order (every lane stores and re-loads its own accumulator quads, 1 KB contiguous per instruction; only the last launch of a
 * slice writes the planar output); 0 = through the output tensor itself, in the planar layout.  The values and the order of the additions are
 * the same: results are equal bit for bit, and "conv3h_launches" counts n x n per layer either way.  The scratch (24576 bytes per 4 x 32 tile of
 * the largest sliced layer, times the batch, times its n output slices: "conv3h_merge_out") is allocated with the engine's workspaces, never at a launch.
 * "conv3h_walk" (an option only, no environment variable): how conv3h_kernel's 256 persistent workgroups share the (batch item, band of strips,
 * tile rows) of a launch -- a table planned on the host (csrc/conv3h_walk_plan.h) and uploaded with the engine's workspaces, never at a launch.
 * 1 (default) = balanced: whole planes to every group of workgroups while whole rounds remain, the leftover items cut into equal shares of tile
 * rows over all groups; 0 = the arithmetic walk (XCD x takes items x, x + 8, ..., a fixed segment of T per group).  A block's exponent is a
 * function of the block alone, so the results are equal bit for bit under either schedule and for a chunk alone or in any batch.
 * "conv3h_tiled" (an option only, no environment variable): 1 (default) = the outputs of the first and second 3x3 conv of a TFC block, which
 * only the block's next conv reads, are written and read in conv3h_kernel's tile order -- 1-KB blocks of sixteen channels x sixteen pixels in the
 * consumer waves' own lane order, so a store instruction is 1 KB contiguous and a producer item one 128-byte line -- wherever the kernel runs both
 * layers, T % 4 == 0 and no GroupNorm pass stands between them; 0 = planar.  The block's input and output, every other level and kernel, and the
 * TFC-TDF v3 nets stay planar.  Same accumulators and values, another address: the results are equal bit for bit.  No buffer grows.
 * "conv3h_merge_out" (an option only, no environment variable): the largest channel count whose conv3h_kernel layers run ONE dispatch per
 * 48-channel input slice with the n output slices side by side -- the groups of workgroups dealt into walkers of n groups that take the same
 * tiles at the same time, each group with its own weight image, bias, output slice and partial-sum scratch -- so a layer is n dispatches
 * instead of n x n and an input slice is fetched from memory once instead of n times.  Default 144 (96- and 144-channel layers); 96 = the
 * 96-channel layers only; 0 = n x n launches.  Needs "conv3h_partial_scratch" = 1: with 0 a layer runs n x n launches whatever this option
 * says.  A lane adds the same values in the same order: the results are equal bit for bit.  "conv3h_launches" keeps counting (output slice,
 * input slice) pairs, n x n per layer either way; "conv3h_merged_dispatches" counts the merged dispatches, n per merged layer.  The scratch is
 * one per output slice (n times 24576 bytes per 4 x 32 tile of the largest sliced layer, times the batch) whatever the option says.
 * "conv_down_bf16x6" / "conv_up_bf16x6" (ABI 7; also ASX_DOWN6 / ASX_UP6): 1 (default) = the 2 x 2 / stride-2 convolutions between the levels
 * (mdxnet.py:66-72) and the transposed ones of the decoder with their `x *= skip` (mdxnet.py:80-86, 113) run conv_down6_kernel / conv_up6_kernel
 * (csrc/kernels_updown6.h) while "gemm_bf16x6" is on: the arithmetic of that option -- both fp32 operands split EXACTLY into three bf16 parts, six
 * bf16 MFMA products per multiply-add, fp32 accumulation; the weights pre-split into a fragment-ordered image when they are loaded -- on
 * input planes the LDS-DMA brings in as fp32; 5.5 against 8.9 ms and 8.4 against 10.2 ms per 4-minute song, closer to float64 than the
 * fp32-MFMA kernels they replace.  0 = conv_dma_kernel<2, 2, 2, 0, ...> / <1, 1, 1, 0, ..., EPI_UP> (fp32 MFMA).
 * "gemm_pair_images" (ABI 7; experimental builds only -- the default library accepts 0 and refuses 1): a matrix whose only reader is a row GEMM
 * on the "gemm_f16x3" arithmetic written by its producer (the epilogue of the row GEMM in front of it) as the two fp16 parts the reader
 * multiplies -- four consecutive elements as h0 h1 h2 h3 l0 l1 l2 l3 in the 16 bytes of their fp32 values, one power-of-two exponent per
 * (row, column tile of the producer) in a table beside it -- so that no column tile of the reader splits its rows again (the bottleneck
 * activations of every TDF block, the hidden activations of the Roformer feed-forward).  Measured round 6: the reading launch alone 3-17 %
 * faster, the nets unchanged (profiles/NOTES.md); default 0.
 * "gemm_bf16x6" (per engine since ABI 6 -- it was process-wide; also ASX_GEMM_BF16X6 in the environment): 1 (default) = every row GEMM whose shape allows it
 * (K % 32 == 0, K >= 64, N > 64, N % 8 == 0, 16-byte aligned rows) runs csrc/kernels_gemm3.h -- both fp32 operands split EXACTLY into three
 * bf16 parts, six bf16 MFMA products with fp32 accumulation, the dropped cross terms below 2^-24 of a product: fp32-grade results
 * (closer to a float64 GEMM than the fp32-MFMA kernel on every measured shape) at 1.7-1.9x its speed; the same switch covers the
 * GATHER mode of that kernel (stride-1 / strided convolutions of the channels-last VR and Demucs nets with Cin % 32 == 0 and at least
 * 48 output channels) and the attention kernels of the Roformer / HTDemucs transformers (attention6_kernel, mha6_kernel);
 * 0 = the fp32-MFMA kernels (csrc/kernels_gemm2.h, kernels_halo.h, kernels_ht.h, kernels_rof.h) everywhere.
 * "gemm_f16x3" (also ASX_GEMM_F16X3): which split the row GEMMs and GATHER-mode convolutions above use while "gemm_bf16x6" is on.
 * 1 (default) = fp16 x 3: every row of x scaled by its own running power of two, every group of four output columns of W by one chosen at load, both
 * split into TWO fp16 parts (11 + 11 significand bits), three fp16 MFMA products per multiply-add instead of six, the dropped term
 * below 2^-22 of a product; elements more than 2^14 below their row's (tile's) largest keep an absolute error of 2^-37 of that
 * largest instead of a relative one.  Measured against a float64 GEMM: closer than the bf16 x 6 form on every shape (fewer accumulator
 * roundings), 1.1-1.5x its speed (profiles/r05_gemm_f16x3.txt).  The attention kernels follow the same switch (one exponent per query,
 * per 64-key tile of K, a running one per tile of V, none for the probabilities; 1.16-1.31x, profiles/r05_attention_f16x3.txt).
 * conv_wino6_kernel too (U scaled per (position, output channel) at load, V by one running exponent per (wave, tile row);
 * 1.04-1.11x, profiles/r05_wino6_f16x3.txt).  0 = bf16 x 6 (exact three-way split) in all of them.
 * "gemm_f16x1" (an option only, no environment variable; default 0): REDUCED PRECISION, OPT-IN, not the reference's bits.  1 = "fp16 x 1":
 * where the fp16 x 3 form of the plain row GEMM (fp32 operands; not its GATHER mode, not the fused-output form) and of the Roformer attention
 * (attention6_kernel; not mha6_kernel) would run -- so only while "gemm_bf16x6" and "gemm_f16x3" are on -- ONE fp16 product per multiply-add
 * instead of three.  The arithmetic contract: operands are scaled by the SAME power-of-two block exponents as fp16 x 3 (x: one running
 * exponent per row; W: one per group of four output columns, its largest |w| in [2^14, 2^15); attention: one per query, per 64-key tile of K,
 * a running one per tile of V, 2^14 for the probabilities); each scaled operand is rounded ONCE, round-to-nearest-even, to fp16,
 * h = RNE_f16(v 2^e), and there is no l part; a product is wh xh on v_mfma_f32_16x16x32_f16; accumulation, exponent drops and rises, epilogue
 * (bias, scale, shift, activation, residual, rotary, gates), softmax (online max, exp, sum) and normalisation are the fp32 code of the
 * fp16 x 3 form, expression for expression.  Hence: an element that stays in fp16's normal range under its block exponent (every non-zero x
 * within 2^-26 of its row's running maximum, every w within 2^-28 of its group's) enters as itself rounded to 11 significant bits
 * (m, ex = frexp(v); ldexp(rint(m * 2048) / 2048, ex)), and for such inputs a launch gives the float64 product of the rounded operands up to
 * fp32 accumulation; smaller elements carry an absolute error of at most 2^-25 in scaled units (below 2^-37 of the row maximum); no overflow
 * and no flush of a whole row, unlike a plain half() cast; Inf / NaN rows poison themselves only.  In attention Q, K, V and the
 * probabilities handed to the PV product are rounded once each (P relative to the running maximum of its key tile); logits, max, exp, sums
 * and the rescale between key tiles stay fp32.  Activations, norms, softmax, rotary, STFT / iSTFT stay fp32 as under every setting.  The
 * h-only weight image (half the bytes) is cached beside the two-part one per weight tensor and dropped with it.  0 (default): every launch is
 * what it is without the option, bit for bit.  A captured hipGraph keeps the arithmetic it was captured with.
 * The split weight images these kernels read are built on the FIRST forward after a load (one small kernel + one stream
 * synchronise per weight tensor) and belong to the engine: they are freed only when this engine's weights are re-loaded or the engine
 * is destroyed, never by another engine of the process -- so a hipGraph captured after one warm-up call stays valid while other
 * engines load and unload.  Non-finite inputs are outside the parity domain of either setting and behave differently: an Inf / NaN
 * in a GEMM row makes that row's accumulators NaN under 1 (h = Inf, v - h = NaN) and +-Inf / NaN under 0; the ReLU epilogues then
 * return 0 for NaN (maxNum).  No other row is affected (tests/test_gpu_parity.py::test_rowgemm_bf16x6_nonfinite_rows). */
int asx_set_option(asx_engine *e, const char *key, int32_t value);
/* The value an option of this engine has now, after normalisation ("gemm_*" / "conv_*_bf16x6": 0 / 1; the others: >= 0) -- the
 * environment's default or the last asx_set_option.  Unknown key: ASX_ERR_INVALID.  (ABI 7, additive) */
int asx_get_option(const asx_engine *e, const char *key, int32_t *value);

/* ---- profiling ---------------------------------------------------------- */
int asx_profile_enable(asx_engine *e, int32_t on); /* clears the counters */
int asx_profile_read(asx_engine *e, asx_profile *out); /* synchronises the device */
/* The launches behind those sums, one record each (class, hipEvent milliseconds, algorithmic flops and bytes), in launch order:
 * a profile class can mix MFMA-bound and HBM-bound launches (the Demucs "conv" class does), and a roofline is a per-launch
 * statement.  Writes min(*n, cap) records, *n = launches recorded.  Synchronises the device.  (ABI 4) */
/* ABI 7: bits 8..15 of `cls` carry the number of 16-bit MFMA products per multiply-add the launch's kernel executed -- 6 (bf16 x 6: exactly
 * split operands), 3 (fp16 x 3) or 0 (an fp32-MFMA / VALU kernel); the class is `cls & 0xff`.  A roofline fraction of a class that mixes
 * pipes is executed work over the peak of the pipe that executed it, launch by launch. */
typedef struct asx_launch_rec {
  int32_t cls;
  float ms;
  double flops, bytes;
} asx_launch_rec;
int asx_profile_launches(asx_engine *e, asx_launch_rec *out, int32_t cap, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* ASX_H */
