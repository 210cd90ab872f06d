/* rdst_hip_msssim.h: the C ABI of the multi-scale SSIM loss and score (rdst_amd/loss/msssim.py, rdst_amd.metrics.device_msssim),
 * the fourth header of librdst_hip.so.  Conventions, return values and rdst_last_error() are those of rdst_hip.h;
 * rdst_abi_version() does not count these entry points (a library without them is found by the missing symbol).
 *
 * Definition (the tests' float64 reference computes exactly this).  target X and pred Y are fp32 NCHW, contiguous.  The taps w,
 * cov_norm cn, data_range, C1, C2 and the maps ux .. B2, S at the valid window positions are those of the comment on
 * rdst_ssim_loss in rdst_hip.h.  levels M in [1, 5], weights beta_1 .. beta_M finite and > 0.
 *   Level 1 is the input.  Level j+1 is level j pooled 2x2 with floor sizes (H_{j+1} = H_j / 2, a trailing odd row or column is
 *   dropped); a pooled pixel is ((a + b) + (c + d)) * 0.25f in fp32, in that order, a, b the upper pair and c, d the lower pair.
 *   The pooled fp32 image IS the level: the rounding is part of the definition.  Required: min(H, W) >> (M - 1) >= win.
 *   Per plane p = (n, c):  m_{p,j} = the mean over the valid positions of level j of cs = A2 / B2 for j < M, of S for j = M;
 *   MS_p = prod_j m_{p,j}^beta_j if every m_{p,j} > 0, else exactly 0;   msssim[n] = mean_c MS_p;   loss = 1 - mean_n msssim[n].
 * The gradient, with respect to pred only:  grad = sum_j k_{p,j} d m_{p,j} / d Y,  k_{p,j} = -MS_p beta_j / (m_{p,j} N C).  The
 * pooling is differentiated as the exact average (0.25 to each of its four sources, nothing to a dropped row or column: straight
 * through the fp32 rounding).  A plane with some m_{p,j} <= 0 has k = 0 at every level: its gradient is exactly 0.0.  For a cs
 * level the adjoint inputs are a' = 2 cn (cs uy - ux) / B2, b' = -cn cs / B2, c' = 2 cn / B2 and
 *   d mean(cs) / d Y[p] = (sum_q w(p - q) a'_q + 2 Y[p] sum_q w(p - q) b'_q + X[p] sum_q w(p - q) c'_q) / (Ho Wo);
 * for the S level a, b, c are those of rdst_ssim_loss.  Window arithmetic is fp64; the running sum over the levels is rounded to
 * fp32 once per level, coarse to fine:  acc_j = (float)(k_{p,j} g_j + 0.25 acc_{j+1}[r / 2][c / 2]),  grad = acc_1.
 *
 * Launches: one value tile kernel per level (it also writes the next level's pooled images), one finish workgroup (means, MS_p,
 * msssim, loss and the table k in double), and with `grad` one gradient tile kernel per level: 2 M + 1, or M + 1 value only.
 * No atomics, every sum in a fixed order, nothing syncs with the host; msssim, means and loss have the same bits with and
 * without `grad`.
 *   taps       HOST array of win doubles, or NULL for the uniform window;   weights   HOST array of `levels` doubles
 *   msssim     device, N doubles;   means   device, N*C*levels doubles ([plane][level]), may be NULL
 *   loss       device, 1 float = (float)(1 - mean msssim), may be NULL
 *   grad       device, N*C*H*W floats, d loss / d pred for an upstream gradient of 1; NULL = value only
 *   workspace  device memory of at least rdst_msssim_loss_workspace(...) bytes (0 for bad arguments; with_grad != 0 adds the
 *              per-level running sums of the gradient; a workspace sized with_grad also serves a value-only call).
 * RDST_EINVAL before any launch: everything rdst_ssim_loss refuses, levels outside [1, 5], a non-finite or non-positive weight,
 * an image too small for its levels, a null msssim / weights, a short workspace. */
#ifndef RDST_HIP_MSSSIM_H
#define RDST_HIP_MSSSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t rdst_msssim_loss_workspace(int N, int C, int H, int W, int win, int levels, int with_grad);
int rdst_msssim_loss(const float* target, const float* pred, int N, int C, int H, int W, int win, const double* taps,
                     double cov_norm, double data_range, int levels, const double* weights, double* msssim, double* means,
                     float* loss, float* grad, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDST_HIP_MSSSIM_H */
