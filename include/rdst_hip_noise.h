/* rdst_hip_noise.h: the C ABI of the noise term of the device data path (rdst_amd/data.py: Noise, add_noise, noise_words,
 * DevicePatchSampler(noise=)), LR = A(HR) + n.  Conventions, return values and rdst_last_error() are those of rdst_hip.h;
 * rdst_abi_version() does not count these entry points (a library without them is found by the missing symbol).
 *
 * The generator is counter-based Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85)
 * and has no state: the four words of a pixel are a pure function of (seed, plane, y, x) with key = (seed & 0xffffffff,
 * seed >> 32) and counter = (x, y, plane, 0).  plane = n * C + c is the image-and-channel index of the array being written,
 * (y, x) the position inside that plane (for the sampler: inside the LR patch); the fourth counter word is a stream tag, 0 here
 * and reserved.  One Philox call per output pixel, never shared among pixels; words 0 and 1 are used, 2 and 3 are not.
 * `seed` is one 64-bit value in DEVICE memory, like the dropout seed of rdst_wattn_fwd_drop.
 *
 * Normals: u1 = ((w0 >> 8) + 1) * 2^-24 in (0, 1], u2 = (w1 >> 8) * 2^-24 in [0, 1), both exact in fp32; r = sqrtf(-2 *
 * logf(u1)); (s, c) = sincospif(2 * u2); z0 = r * c, z1 = r * s.  |z| <= sqrt(48 ln 2), about 5.77: no inf, no nan.
 *
 * Models, on a value v with the two levels p0, p1 of its image (read from device memory, each passed through fmaxf(., 0)),
 * every step one explicit fp32 operation (fmaf, or a product rounded once):
 *   RDST_NOISE_HETERO  gain a = p0, floor b = p1:  sd = sqrtf(fmaf(a, fmaxf(v, 0), b * b)),  y = fmaf(sd, z0, v).
 *                      a = 0 is additive Gaussian noise of sigma b; otherwise the Gaussian approximation of Poisson-Gaussian
 *                      noise in the parametrisation of Foi et al. (variance a v + b^2).  Not exact Poisson sampling.
 *   RDST_NOISE_RICIAN  sigma = p0:  re = fmaf(sigma, z0, v),  im = sigma * z1,  y = sqrtf(fmaf(re, re, im * im)).
 * then y = fminf(fmaxf(y, clip_lo), clip_hi); -inf / +inf mean no clip.
 *
 * DEFINING PROPERTY: `lr` of rdst_sample_patches_noise equals rdst_add_noise applied to rdst_resample_sep (rdst_hip_data.h) of
 * its `hr`, under the same table, levels, seed and clip, bit for bit. */
#ifndef RDST_HIP_NOISE_H
#define RDST_HIP_NOISE_H

#include <stddef.h>
#include <stdint.h>

#define RDST_NOISE_HETERO 0
#define RDST_NOISE_RICIAN 1

#ifdef __cplusplus
extern "C" {
#endif

/* The four Philox words of every pixel as bit patterns: out int32 (planes, H, W, 4), 16-byte aligned.  The pinned contract of
 * the generator.  One launch.  RDST_EINVAL for a non-positive size, a null or misaligned `out`, a null `seed`, more values than
 * one launch takes. */
int rdst_noise_words(int32_t* out, int planes, int H, int W, const unsigned long long* seed, void* stream);
/* Whole images: x fp32 (N, C, H, W) -> y of the same shape, contiguous; y == x is allowed (no other overlap is).  `levels` is
 * (N, 2) fp32 on the device: (p0, p1) of image n.  One launch.  RDST_EINVAL for a non-positive size, a null x, y, levels or
 * seed, a model that is neither RDST_NOISE_HETERO nor RDST_NOISE_RICIAN, a NaN clip or clip_lo > clip_hi, more values than
 * one launch takes. */
int rdst_add_noise(const float* x, float* y, int N, int C, int H, int W, int model, const float* levels,
                   const unsigned long long* seed, float clip_lo, float clip_hi, void* stream);
/* rdst_sample_patches_op (rdst_hip_data.h: every argument up to tap_weight is its argument) with the noise applied to each LR
 * value in the final store of the band's LR columns: the same ONE launch, the same kernel with a compile-time switch.  `levels`
 * is (B, 2) fp32 on the device: (p0, p1) of patch b.  hr and label_out are untouched by the noise.  A K = 4 table of the plain
 * cubic resize gives the noisy form of rdst_sample_patches / rdst_sample_patches_d8.  The refusals of rdst_sample_patches_op,
 * and RDST_EINVAL for a null levels or seed, a model outside the two, a NaN clip or clip_lo > clip_hi. */
int rdst_sample_patches_noise(const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant, float* hr,
                              float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp, int K,
                              const int32_t* tap_index, const float* tap_weight, int model, const float* levels,
                              const unsigned long long* seed, float clip_lo, float clip_hi, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDST_HIP_NOISE_H */
