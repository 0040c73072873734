// TFC-TDF v3 normalisation helpers that run on the host (no HIP): the encoding of asx_v3_config.norm, the
// BatchNorm fold and the split rule of the GroupNorm statistics pass.  Included by engine_v3.h and, for the
// host tests, by tests/host/v3_norm_host.cpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

// asx_v3_config.norm (include/asx.h): 0 None / Identity, 1 InstanceNorm, 2 BatchNorm, 256 + G GroupNorm(G)
enum { V3_NORM_NONE = 0, V3_NORM_INSTANCE = 1, V3_NORM_BATCH = 2, V3_NORM_GROUP = 256 };
// asx_v3_config.act: 0 relu, 1 gelu, 2 elu (alpha: the one-element tensor V3_ACT_ALPHA_TENSOR)
enum { V3_ACT_RELU = 0, V3_ACT_GELU = 1, V3_ACT_ELU = 2 };
#define V3_ACT_ALPHA_TENSOR "__act_alpha__"

static inline bool v3_norm_valid(int norm) {
  return norm == V3_NORM_NONE || norm == V3_NORM_INSTANCE || norm == V3_NORM_BATCH || norm > V3_NORM_GROUP;
}
static inline int v3_norm_groups(int norm) { return norm > V3_NORM_GROUP ? norm - V3_NORM_GROUP : 0; }

// nn.BatchNorm2d in eval(): y = (x - running_mean) / sqrt(running_var + eps) * weight + bias = x * scale + shift,
// folded in float64 and rounded once.
static inline void v3_bn_fold(int c, const float *weight, const float *bias, const float *mean, const float *var, double eps,
                              float *scale, float *shift) {
  for (int i = 0; i < c; ++i) {
    const double sc = (double)weight[i] / std::sqrt((double)var[i] + eps);
    scale[i] = (float)sc;
    shift[i] = (float)((double)bias[i] - (double)mean[i] * sc);
  }
}

// Slices per (group, batch item) of the GroupNorm statistics pass: enough workgroups for ~8 per CU on 256 CUs over the
// whole pass, but no slice shorter than 16 Ki floats (64 KiB) and at most V3_GN_MAX_SPLIT of them.
enum { V3_GN_MAX_SPLIT = 1024, V3_GN_MIN_SLICE = 16384, V3_GN_TARGET_BLOCKS = 2048 };
static inline int v3_gn_splits(int B, int G, int64_t len) {
  const int64_t bg = std::max<int64_t>(1, (int64_t)B * G);
  const int64_t want = (V3_GN_TARGET_BLOCKS + bg - 1) / bg;
  const int64_t cap = std::max<int64_t>(1, len / V3_GN_MIN_SLICE);
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, cap), V3_GN_MAX_SPLIT));
}
