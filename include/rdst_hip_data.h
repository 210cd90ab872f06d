/* rdst_hip_data.h: the C ABI of the K-tap degradations of the device data path (rdst_amd/data.py), the second header of
 * librdst_hip.so.  Conventions, return values and rdst_last_error() are those of rdst_hip.h; rdst_abi_version() does not
 * count these entry points (a library without them is found by the missing symbol).
 *
 * A degradation is a separable linear operator LR = A_y . patch . A_x^T.  An axis operator is a K-tap table in device
 * memory, 16-byte aligned: `out` rows of K int32 source indices and `out` rows of K fp32 weights, K positive and a
 * multiple of 4, taps in ascending source order, short rows padded at the end with weight 0 and the row's last index,
 * computed by the host in float64 and rounded once (rdst_amd.data.operator_table).  The kernels clamp every index they read
 * before it becomes an address.  Every output is formed by the generalisation of the 4-tap chain of rdst_resize_bicubic:
 * acc = w[0] * v[0] rounded, then acc = fmaf(w[k], v[k], acc) for k = 1 .. K-1 ascending; the HORIZONTAL sums of the tap
 * rows first, then the vertical chain over them.  The same pixels under the same table give the same bits in both entry
 * points, and a K = 4 table gives the bits of rdst_resize_bicubic / rdst_sample_patches / rdst_sample_patches_d8. */
#ifndef RDST_HIP_DATA_H
#define RDST_HIP_DATA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Resample whole images: x fp32 (N, C, H, W) -> y fp32 (N, C, oh, ow), contiguous; the table of the rows is (oh, Ky) over
 * [0, H), that of the columns (ow, Kx) over [0, W).  `tmp` is a caller workspace of N * C * H * ow floats for the horizontal
 * sums.  Two launches: the horizontal sums of every source row, then the vertical chains.  RDST_EINVAL for a non-positive
 * size, a null pointer, Ky or Kx not a positive multiple of 4, a table that is not 16-byte aligned. */
int rdst_resample_sep(const float* x, float* y, float* tmp, int N, int C, int H, int W, int oh, int ow, int Ky,
                      const int32_t* index_y, const float* weight_y, int Kx, const int32_t* index_x, const float* weight_x,
                      void* stream);
/* The batch of rdst_sample_patches / rdst_sample_patches_d8 (rdst_hip.h: stack, labels, index, variant, hr, lr, label_out
 * and the sizes are theirs) under the K-tap table (lp, K) of the (hp -> lp) axis, used for both axes: patch b is cut,
 * turned by T_k with k = variant[b] & 7 (a NULL `variant` means no turn), then degraded, so lr equals rdst_resample_sep of
 * hr under the same table bit for bit.  ONE launch, no atomics: a workgroup per (patch, channel, band of LR columns) walks
 * the rows of the turned patch in chunks through LDS, keeps the horizontal sums of its columns there and forms its LR
 * columns from them; the HR and label rows are written by the band that owns the chunk.  The refusals of
 * rdst_sample_patches, and RDST_EINVAL for K not a positive multiple of 4, a null or misaligned table; RDST_ENOTSUP if
 * the horizontal sums of one LR column and one staged row do not fit the 64 KB of LDS (hp beyond about 5400). */
int rdst_sample_patches_op(const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant, float* hr,
                           float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp, int K,
                           const int32_t* tap_index, const float* tap_weight, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RDST_HIP_DATA_H */
