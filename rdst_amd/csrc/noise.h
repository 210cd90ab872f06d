// The noise term of the device data path (include/rdst_hip_noise.h carries the definition): one value of LR = A(HR) + n.
// noise_apply() is the only place the models are written; the whole-image kernel (noise.hip) and the sampler's final store
// (resample.hip) both call it, and every step is an explicit fmaf / __fmul_rn, so contraction cannot make the two call sites
// differ: the same value at the same (seed, plane, y, x) under the same levels gives the same bits.
#pragma once
#include "common.h"
#include "philox.h"
#include "../../include/rdst_hip_noise.h"

namespace {

// what the two entry points that add noise pass to their kernels
struct NoiseArgs {
  int model;                        // RDST_NOISE_HETERO / RDST_NOISE_RICIAN
  const float* levels;              // (images, 2) fp32, device
  const unsigned long long* seed;   // device
  float clip_lo, clip_hi;
};

// two independent standard normals from words 0 and 1 (Box-Muller): u1 in (0, 1], u2 in [0, 1), both exact in fp32, as is the
// argument 2 u2 of sincospif; |z| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) < 5.77, so nothing here is inf or nan
__device__ __forceinline__ void noise_normals(const PhiloxWords& w, float& z0, float& z1) {
  const float u1 = __fmul_rn((float)((w.w0 >> 8) + 1u), 0x1p-24f);
  const float u2 = __fmul_rn((float)(w.w1 >> 8), 0x1p-24f);
  const float r = sqrtf(__fmul_rn(-2.0f, logf(u1)));
  float s, c;
  sincospif(__fmul_rn(2.0f, u2), &s, &c);
  z0 = __fmul_rn(r, c);
  z1 = __fmul_rn(r, s);
}

// v with the noise of pixel (y, x) of plane `plane`; p0, p1 are the image's two levels as read from device memory
__device__ __forceinline__ float noise_apply(float v, unsigned long long seed, uint32_t plane, uint32_t y, uint32_t x, int model,
                                             float p0, float p1, float clip_lo, float clip_hi) {
  float z0, z1;
  noise_normals(philox_pixel(seed, plane, y, x), z0, z1);
  p0 = fmaxf(p0, 0.0f);
  p1 = fmaxf(p1, 0.0f);
  float out;
  if (model == RDST_NOISE_RICIAN) {   // sigma = p0: complex Gaussian noise around the real value v, then the modulus
    const float re = fmaf(p0, z0, v), im = __fmul_rn(p0, z1);
    out = sqrtf(fmaf(re, re, __fmul_rn(im, im)));
  } else {                            // gain a = p0, floor b = p1: variance a max(v, 0) + b^2
    const float sd = sqrtf(fmaf(p0, fmaxf(v, 0.0f), __fmul_rn(p1, p1)));
    out = fmaf(sd, z0, v);
  }
  return fminf(fmaxf(out, clip_lo), clip_hi);
}

// the refusals the two entry points that add noise share: returned before any launch
inline int noise_refusal(const char* who, int model, const float* levels, const unsigned long long* seed, float clip_lo,
                         float clip_hi) {
  if (!levels) return rdst_fail(RDST_EINVAL, "%s: null levels", who);
  if (!seed) return rdst_fail(RDST_EINVAL, "%s: null seed", who);
  if (model != RDST_NOISE_HETERO && model != RDST_NOISE_RICIAN)
    return rdst_fail(RDST_EINVAL, "%s: model=%d is neither RDST_NOISE_HETERO (0) nor RDST_NOISE_RICIAN (1)", who, model);
  if (clip_lo != clip_lo || clip_hi != clip_hi) return rdst_fail(RDST_EINVAL, "%s: clip_lo / clip_hi must not be NaN", who);
  if (clip_lo > clip_hi) return rdst_fail(RDST_EINVAL, "%s: clip_lo=%g is above clip_hi=%g", who, (double)clip_lo, (double)clip_hi);
  return 0;
}

}  // namespace
