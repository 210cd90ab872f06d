/* rdst_hip_consistency.h: the C ABI of the LR-consistency kernels (rdst_amd/loss/consistency.py, SRTester's
 * back-projection), the third header of librdst_hip.so.  Conventions, return values and rdst_last_error() are those of
 * rdst_hip.h; rdst_abi_version() does not count these entry points (a library without them is found by the missing symbol).
 *
 * The operators are the K-tap tables of rdst_hip_data.h (rdst_amd.data.operator_table) and their transposes
 * (rdst_amd.data.adjoint_table), in the same format: K a positive multiple of 4, 16-byte aligned, taps ascending, padding of
 * weight 0.  Every sum is the tap chain of rdst_resample_sep (the horizontal sums first, then the vertical chain), so
 * D below has the bits of rdst_resample_sep(pred) and `a` the bits of rdst_resample_sep(g) under the transposed tables.
 * No atomics: results are bit-identical from run to run. */
#ifndef RDST_HIP_CONSISTENCY_H
#define RDST_HIP_CONSISTENCY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of rdst_lrc_residual's workspace when `loss` is asked for (one fp64 partial per workgroup, for the narrowest band
 * the entry point may choose); 0 for a non-positive size. */
size_t rdst_lrc_workspace(int N, int C, int oh, int ow);
/* The residual of the degraded prediction: pred fp32 (N, C, H, W), lr fp32 (N, C, oh, ow), contiguous; the table of the rows
 * is (oh, Ky) over [0, H), that of the columns (ow, Kx) over [0, W).  D = A_y . pred . A_x^T, R = D - lr (one rounding).
 * Outputs, each optional (NULL skips it):
 *   resid (N, C, oh, ow) = R;
 *   g     (N, C, oh, ow) = d loss / d D:  norm 1 (L1): copysignf(inv_n, R), exactly 0 where R == 0;  norm 2 (L2):
 *         scale * R rounded once;  inv_n = (float)(1.0 / n), scale = (float)(2.0 / n), n = N C oh ow, formed in double;
 *   loss  one float: mean |R| (norm 1) or mean R^2 (norm 2): fp64 partial sums, one per workgroup in `workspace`, added by a
 *         finish kernel in a fixed order, divided by n and rounded once.
 * norm 0 forms R alone: g and loss must be NULL.  One tile launch (a workgroup per plane and band of LR columns, the rows
 * staged through LDS in chunks) plus the finish launch when `loss` is given.  RDST_EINVAL for a bad size, norm, table or
 * pointer or a short workspace; RDST_ENOTSUP when the sums of one LR column and one staged row do not fit the LDS. */
int rdst_lrc_residual(const float* pred, const float* lr, int N, int C, int H, int W, int oh, int ow, int Ky,
                      const int32_t* index_y, const float* weight_y, int Kx, const int32_t* index_x, const float* weight_x,
                      int norm, float* resid, float* g, float* loss, void* workspace, size_t workspace_bytes, void* stream);
/* The adjoint: g fp32 (N, C, oh, ow) -> a = A_y^T . g . A_x (N, C, H, W) under the TRANSPOSED tables, (H, KyT) over [0, oh)
 * and (W, KxT) over [0, ow); then s = scale_dev ? scale_host * *scale_dev (one rounding) : scale_host and
 *   out = base ? fmaf(s, a, base) : s * a (one rounding).
 * out == base is allowed: every element is read once and written once by the same thread.  One launch: a workgroup per plane,
 * band of HR rows and band of HR columns stages the g rows its taps read through LDS.  RDST_EINVAL as above; RDST_ENOTSUP
 * when one column of sums and one staged row do not fit the LDS. */
int rdst_lrc_adjoint(const float* g, int N, int C, int oh, int ow, int H, int W, int KyT, const int32_t* index_yT,
                     const float* weight_yT, int KxT, const int32_t* index_xT, const float* weight_xT,
                     const float* scale_dev, float scale_host, const float* base, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDST_HIP_CONSISTENCY_H */
