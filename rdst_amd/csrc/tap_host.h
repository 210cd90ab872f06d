// The host side of the tap-table kernels (sampler.hip, resample.hip, consistency.hip): the constants their plans share, the
// argument checks of the sampler entry points and of a K-tap table, and the LDS fit of the sums-and-chunk layout.  Every
// refusal is made before anything is launched and leaves its text behind rdst_last_error().
#pragma once
#include "common.h"

constexpr int NT = 256;                 // threads of every workgroup
constexpr int LDS_BUDGET = 64 * 1024;   // the default dynamic-LDS limit of a workgroup
constexpr int BC_MAX = 8;               // columns per band of the sums hs [rows][BC + 1]
constexpr int RC_MAX = 32;              // rows per staged chunk raw [RC][pitch]
constexpr int SG = 8;                   // staging loads a thread issues before it stores them

// the argument checks of the four sampler entry points
static inline int sample_refusal(const char* who, const float* stack, const uint8_t* labels, const int32_t* index, const float* hr,
                                 const float* lr, const uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp) {
  if (S <= 0 || C <= 0 || H <= 0 || W <= 0 || B <= 0 || hp <= 0 || lp <= 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape S=%d C=%d H=%d W=%d B=%d hp=%d lp=%d", who, S, C, H, W, B, hp, lp);
  if (hp > H || hp > W) return rdst_fail(RDST_EINVAL, "%s: a %d x %d patch does not fit a %d x %d slice", who, hp, hp, H, W);
  if (!stack || !index || !hr || !lr) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if ((labels != nullptr) != (label_out != nullptr))
    return rdst_fail(RDST_EINVAL, "%s: labels and label_out go together", who);
  if ((int64_t)B * C * hp * hp > ((int64_t)1 << 40) || (int64_t)B * C > (1 << 20))
    return rdst_fail(RDST_EINVAL, "%s: B=%d C=%d hp=%d is too large for one launch", who, B, C, hp);
  return 0;
}

// a table of K taps per output, read as int4 / float4; `axis` names it in the text (" y", " xT", "")
static inline int table_refusal(const char* who, const char* axis, int K, const int32_t* tap_index, const float* tap_weight) {
  if (K <= 0 || K % 4 != 0) return rdst_fail(RDST_EINVAL, "%s: K%s=%d must be a positive multiple of 4", who, axis, K);
  if (!tap_index || !tap_weight) return rdst_fail(RDST_EINVAL, "%s: null tap table%s", who, axis);
  if (!rdst_aligned(16, {tap_index, tap_weight}, {}))
    return rdst_fail(RDST_EINVAL, "%s: the tap table%s must be 16-byte aligned", who, axis);
  return 0;
}

// sums [rows][BC + 1] and raw [RC][pitch] within `budget` bytes of LDS: shorter chunks first, then narrower bands
static inline bool fit_lds(int rows, int& BC, int& RC, int pitch, int budget, int64_t& bytes) {
  auto need = [&]() { return ((int64_t)rows * (BC + 1) + (int64_t)RC * pitch) * (int64_t)sizeof(float); };
  while (need() > budget && RC > 1) RC >>= 1;
  while (need() > budget && BC > 1) BC >>= 1;
  bytes = need();
  return bytes <= budget;
}
