// LR consistency (rdst_amd/loss/consistency.py, SRTester's back-projection; include/rdst_hip_consistency.h): the residual
// R = A(pred) - lr of a prediction under a K-tap degradation with the value and the unit gradient of its L1 / L2 mean
// (rdst_lrc_residual), and the adjoint A^T(g) with a scaled-add epilogue (rdst_lrc_adjoint).
//
// Every value is formed by tapk() (tapk.h), the chain of resample.hip: the horizontal sums of the tap rows first, then the
// vertical chain over them, reading the same samples in the same order, so D = A(pred) has the bits of rdst_resample_sep(pred)
// and a = A^T(g) the bits of rdst_resample_sep(g) under the transposed tables (a padding tap reads the element it reads
// there: the staged ranges below are taken from the first and the last tap of every row, padding included).
//
// rdst_lrc_residual is resample.hip's sample_op_kernel without the turn and without the HR / label copy: a workgroup is one
// (plane, band of BC = 8 LR columns); it walks the rows of the plane in chunks of RC = 32 through raw[RC][W | 1], keeps the
// horizontal sums of its columns in hs[H][BC + 1] and forms its LR columns from them.  42 KB of LDS at 256 x 256 (three
// workgroups per CU of the 160 KB); shorter chunks first, then narrower bands, as rdst_sample_patches_op shrinks.  The fp64
// sum of |R| or R^2 goes to one workspace slot per workgroup (threads ascending over their elements, lanes by xor-shuffle,
// waves in order); one workgroup of the finish kernel adds the slots the same way: a fixed order, no atomics.
//
// rdst_lrc_adjoint: a workgroup is one (plane, band of BR HR rows, band of BC HR columns).  It reads the first and last tap
// of its rows in the transposed y-table to find the g rows [r_lo, r_hi] it needs (and of its columns for [c_lo, c_hi]),
// stages them in chunks of RC = 32 rows through raw[RC][ow | 1], keeps their horizontal sums for its columns in
// hs[oh][BC + 1] and forms the vertical chains from them.  Sparse tables (KyT < oh): BR = 32, BC = 32 (8.4 + 8.3 KB at the
// training shape 64 x 64 -> 256 x 256, eleven g rows per band under the x4 cubic).  A dense table ('fourier') makes every
// band need all oh rows, so the row band grows to BR = min(H, 256) and the column band narrows to BC = 8: the horizontal
// sums are formed once per column band instead of once per 32 rows.  The host cannot see the table, so the choice is a
// heuristic on the y-table alone, KyT >= oh: a sparse operator on a very low LR image (cubic with oh <= 4) gets the
// dense cut too, which changes the cut and not the result.  Both pitches (BC + 1, ow | 1) are odd:
// lanes along a row or down a column of either image meet every bank once (ds_read_b32 / ds_write_b32: 32 banks per half).
//
// No MFMA, no atomics, no scratch; every index read from device memory is clamped before it becomes an address.
#include "tap_host.h"
#include "tapk.h"
#include "../../include/rdst_hip_consistency.h"

namespace {

constexpr int NW = NT / 64;
constexpr int LRC_BUDGET = LDS_BUDGET - 256;   // less the static reduction slots
constexpr int ABR = 32, ABC = 32;       // adjoint, sparse tables: HR rows / columns per band (the residual's are BC_MAX, RC_MAX)
constexpr int ABR_DENSE = 256, ABC_DENSE = 8;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the sum of `v` over the workgroup in a fixed order, in thread 0
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < NW; ++w) s += red[w];
  return s;
}

// [lo, hi] of the clamped first and last taps of table rows [o0, o0 + n): taps ascend, so a row's first is its lowest and
// its last its highest
__device__ __forceinline__ void tap_range(const int4* __restrict__ it, int K4, int o0, int n, int top, int* red, int& lo, int& hi) {
  int a = top, b = 0;
  for (int o = o0 + (int)threadIdx.x; o < o0 + n; o += NT) {
    a = min(a, clampi(it[(int64_t)o * K4].x, 0, top));
    b = max(b, clampi(it[(int64_t)o * K4 + K4 - 1].w, 0, top));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a = min(a, __shfl_xor(a, o, 64)), b = max(b, __shfl_xor(b, o, 64));
  __syncthreads();   // red may still be read from the call before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a, red[NW + (threadIdx.x >> 6)] = b;
  __syncthreads();
  lo = top, hi = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) lo = min(lo, red[w]), hi = max(hi, red[NW + w]);
  hi = max(hi, lo);
}

// rows [0, rcn) x columns [0, ncols) of `src` (row stride ld) into raw[r * pitch + j]; SG loads of a thread are in flight together
__device__ __forceinline__ void stage(const float* __restrict__ src, int64_t ld, int rcn, int ncols, float* raw, int pitch) {
  const int n = rcn * ncols;
  for (int e0 = threadIdx.x; e0 < n; e0 += SG * NT) {
    float v[SG];
    int to[SG];
#pragma unroll
    for (int u = 0; u < SG; ++u) {
      const int e = e0 + u * NT;
      const int r = e / ncols, j = e - r * ncols;
      if (e < n) v[u] = src[(int64_t)r * ld + j];
      to[u] = r * pitch + j;
    }
#pragma unroll
    for (int u = 0; u < SG; ++u)
      if (e0 + u * NT < n) raw[to[u]] = v[u];
  }
}

// ---- rdst_lrc_residual: one workgroup per (plane, band of BC LR columns) ---------------------------------------------------
__global__ void __launch_bounds__(NT) lrc_tile_kernel(const float* __restrict__ pred, const float* __restrict__ lr, int H, int W,
                                                      int oh, int ow, int Ky4, const int4* __restrict__ iy,
                                                      const f4* __restrict__ wy, int Kx4, const int4* __restrict__ ix,
                                                      const f4* __restrict__ wx, int norm, float gs, float* __restrict__ resid,
                                                      float* __restrict__ g, double* __restrict__ part, int BC, int nb, int RC,
                                                      int pitch) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // hs [H][BC + 1], then raw [RC][pitch]
  __shared__ int ired[2 * NW];
  __shared__ double dred[NW];
  const int hsp = BC + 1;
  float* hs = lds;
  float* raw = lds + (int64_t)H * hsp;
  const int band = (int)(blockIdx.x % (unsigned)nb);
  const int64_t plane = blockIdx.x / (unsigned)nb;
  const int c0 = band * BC, bcn = min(BC, ow - c0);
  int x_lo, x_hi;
  tap_range(ix, Kx4, c0, bcn, W - 1, ired, x_lo, x_hi);
  const int nx = x_hi + 1 - x_lo;
  const float* src = pred + plane * H * W + x_lo;
  for (int r0 = 0; r0 < H; r0 += RC) {
    const int rcn = min(RC, H - r0);
    stage(src + (int64_t)r0 * W, W, rcn, nx, raw, pitch);
    __syncthreads();
    for (int e = threadIdx.x; e < rcn * bcn; e += NT) {
      const int r = e / bcn, oxl = e - r * bcn;
      const float* row = raw + r * pitch;
      const int64_t t = (int64_t)(c0 + oxl) * Kx4;
      hs[(r0 + r) * hsp + oxl] = tapk(ix + t, wx + t, Kx4, [&](int j) { return row[clampi(clampi(j, 0, W - 1) - x_lo, 0, nx - 1)]; });
    }
    __syncthreads();   // hs of the chunk is whole; the next chunk overwrites raw
  }
  const int64_t at = plane * oh * ow + c0;
  double sum = 0.0;
  for (int e = threadIdx.x; e < oh * bcn; e += NT) {
    const int oy = e / bcn, oxl = e - oy * bcn;
    const int64_t t = (int64_t)oy * Ky4;
    const float D = tapk(iy + t, wy + t, Ky4, [&](int j) { return hs[clampi(j, 0, H - 1) * hsp + oxl]; });
    const int64_t i = at + (int64_t)oy * ow + oxl;
    const float R = __fsub_rn(D, lr[i]);
    if (resid != nullptr) resid[i] = R;
    if (norm == 1) {
      if (g != nullptr) g[i] = R == 0.f ? 0.f : copysignf(gs, R);
      sum += fabs((double)R);
    } else if (norm == 2) {
      if (g != nullptr) g[i] = __fmul_rn(gs, R);
      sum += (double)R * (double)R;
    }
  }
  if (part != nullptr) {
    const double s = block_sum_f64(sum, dred);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
  }
}

// one workgroup: the slots in a fixed order, divided by n, rounded once
__global__ void __launch_bounds__(NT) lrc_finish_kernel(const double* __restrict__ part, int64_t slots, double n,
                                                        float* __restrict__ loss) {
  __shared__ double dred[NW];
  double s = 0.0;
  for (int64_t t = threadIdx.x; t < slots; t += NT) s += part[t];
  s = block_sum_f64(s, dred);
  if (threadIdx.x == 0) *loss = (float)(s / n);
}

// ---- rdst_lrc_adjoint: one workgroup per (plane, band of BR HR rows, band of BC HR columns) -------------------------------
__global__ void __launch_bounds__(NT) lrc_adjoint_kernel(const float* __restrict__ g, int oh, int ow, int H, int W, int Ky4,
                                                         const int4* __restrict__ iy, const f4* __restrict__ wy, int Kx4,
                                                         const int4* __restrict__ ix, const f4* __restrict__ wx,
                                                         const float* __restrict__ scale_dev, float scale_host,
                                                         const float* base, float* out, int BR, int nbr, int BC, int nbc,
                                                         int RC, int pitch) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // hs [oh][BC + 1], then raw [RC][pitch]
  __shared__ int ired[2 * NW];
  const int hsp = BC + 1;
  float* hs = lds;
  float* raw = lds + (int64_t)oh * hsp;
  const int cb = (int)(blockIdx.x % (unsigned)nbc);
  const unsigned up = blockIdx.x / (unsigned)nbc;
  const int rb = (int)(up % (unsigned)nbr);
  const int64_t plane = up / (unsigned)nbr;
  const int y0 = rb * BR, brn = min(BR, H - y0);
  const int x0 = cb * BC, bcn = min(BC, W - x0);
  int r_lo, r_hi, c_lo, c_hi;
  tap_range(iy, Ky4, y0, brn, oh - 1, ired, r_lo, r_hi);
  tap_range(ix, Kx4, x0, bcn, ow - 1, ired, c_lo, c_hi);
  const int nr = r_hi + 1 - r_lo, nc = c_hi + 1 - c_lo;
  const float* src = g + plane * oh * ow + (int64_t)r_lo * ow + c_lo;
  for (int r0 = 0; r0 < nr; r0 += RC) {
    const int rcn = min(RC, nr - r0);
    stage(src + (int64_t)r0 * ow, ow, rcn, nc, raw, pitch);
    __syncthreads();
    for (int e = threadIdx.x; e < rcn * bcn; e += NT) {
      const int r = e / bcn, xl = e - r * bcn;
      const float* row = raw + r * pitch;
      const int64_t t = (int64_t)(x0 + xl) * Kx4;
      hs[(r0 + r) * hsp + xl] = tapk(ix + t, wx + t, Kx4, [&](int j) { return row[clampi(clampi(j, 0, ow - 1) - c_lo, 0, nc - 1)]; });
    }
    __syncthreads();   // hs of the chunk is whole; the next chunk overwrites raw
  }
  const float s = scale_dev != nullptr ? __fmul_rn(scale_host, *scale_dev) : scale_host;
  const int64_t at = plane * H * W + (int64_t)y0 * W + x0;
  for (int e = threadIdx.x; e < brn * bcn; e += NT) {
    const int yl = e / bcn, xl = e - yl * bcn;
    const int64_t t = (int64_t)(y0 + yl) * Ky4;
    const float a = tapk(iy + t, wy + t, Ky4, [&](int j) { return hs[clampi(clampi(j, 0, oh - 1) - r_lo, 0, nr - 1) * hsp + xl]; });
    const int64_t i = at + (int64_t)yl * W + xl;
    out[i] = base != nullptr ? fmaf(s, a, base[i]) : __fmul_rn(s, a);
  }
}

int shape_refusal(const char* who, int N, int C, int H, int W, int oh, int ow) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d HR %d x %d LR %d x %d", who, N, C, H, W, oh, ow);
  if ((int64_t)N * C > (1 << 20) || (int64_t)N * C * H * W > ((int64_t)1 << 40) || (int64_t)N * C * oh * ow > ((int64_t)1 << 40))
    return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d HR %d x %d LR %d x %d is too large for one launch", who, N, C, H, W, oh, ow);
  return 0;
}

}  // namespace

extern "C" size_t rdst_lrc_workspace(int N, int C, int oh, int ow) {
  if (N <= 0 || C <= 0 || oh <= 0 || ow <= 0) {
    rdst_fail(RDST_EINVAL, "rdst_lrc_workspace: bad shape N=%d C=%d LR %d x %d", N, C, oh, ow);
    return 0;
  }
  return (size_t)N * (size_t)C * (size_t)ow * sizeof(double);   // bands of one column: the most workgroups there can be
}

extern "C" int rdst_lrc_residual(const float* pred, const float* lr, int N, int C, int H, int W, int oh, int ow, int Ky,
                                 const int32_t* index_y, const float* weight_y, int Kx, const int32_t* index_x,
                                 const float* weight_x, int norm, float* resid, float* g, float* loss, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const char* who = "rdst_lrc_residual";
  if (int rc = shape_refusal(who, N, C, H, W, oh, ow)) return rc;
  if (!pred || !lr) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if (norm < 0 || norm > 2) return rdst_fail(RDST_EINVAL, "%s: norm=%d must be 0 (residual only), 1 (L1) or 2 (L2)", who, norm);
  if (norm == 0 && (g || loss)) return rdst_fail(RDST_EINVAL, "%s: norm=0 forms the residual alone: g and loss must be null", who);
  if (!resid && !g && !loss) return rdst_fail(RDST_EINVAL, "%s: nothing to write (resid, g and loss are all null)", who);
  if (int rc = table_refusal(who, " y", Ky, index_y, weight_y)) return rc;
  if (int rc = table_refusal(who, " x", Kx, index_x, weight_x)) return rc;
  const int pitch = W | 1;
  int BC = min(BC_MAX, ow), RC = min(RC_MAX, H);
  int64_t bytes;
  if (!fit_lds(H, BC, RC, pitch, LRC_BUDGET, bytes))
    return rdst_fail(RDST_ENOTSUP, "%s: H=%d W=%d is larger than the LDS holds (one column of sums and one row need %lld bytes)",
                     who, H, W, (long long)bytes);
  const int nb = (ow + BC - 1) / BC;
  const int64_t blocks = (int64_t)N * C * nb;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d ow=%d is too large for one launch", who, N, C, ow);
  if (loss) {
    const size_t need = (size_t)blocks * sizeof(double);
    if (!workspace || workspace_bytes < need)
      return rdst_fail(RDST_EINVAL, "%s: workspace of %zu bytes, %zu needed (rdst_lrc_workspace)", who,
                       workspace ? workspace_bytes : (size_t)0, need);
  }
  const double n = (double)N * C * oh * ow;
  const float gs = norm == 1 ? (float)(1.0 / n) : (float)(2.0 / n);
  double* part = loss ? (double*)workspace : nullptr;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(lrc_tile_kernel, dim3((unsigned)blocks), dim3(NT), (size_t)bytes, st, pred, lr, H, W, oh, ow, Ky / 4,
                     (const int4*)index_y, (const f4*)weight_y, Kx / 4, (const int4*)index_x, (const f4*)weight_x, norm, gs, resid,
                     g, part, BC, nb, RC, pitch);
  if (int rc = rdst_launch_status(who)) return rc;
  if (!loss) return 0;
  hipLaunchKernelGGL(lrc_finish_kernel, dim3(1), dim3(NT), 0, st, (const double*)part, blocks, n, loss);
  return rdst_launch_status(who);
}

extern "C" int rdst_lrc_adjoint(const float* g, int N, int C, int oh, int ow, int H, int W, int KyT, const int32_t* index_yT,
                                const float* weight_yT, int KxT, const int32_t* index_xT, const float* weight_xT,
                                const float* scale_dev, float scale_host, const float* base, float* out, void* stream) {
  const char* who = "rdst_lrc_adjoint";
  if (int rc = shape_refusal(who, N, C, H, W, oh, ow)) return rc;
  if (!g || !out) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if (int rc = table_refusal(who, " yT", KyT, index_yT, weight_yT)) return rc;
  if (int rc = table_refusal(who, " xT", KxT, index_xT, weight_xT)) return rc;
  const bool dense = KyT >= oh;
  const int BR = min(dense ? ABR_DENSE : ABR, H);
  const int pitch = ow | 1;
  int BC = min(dense ? ABC_DENSE : ABC, W), RC = min(RC_MAX, oh);
  int64_t bytes;
  if (!fit_lds(oh, BC, RC, pitch, LRC_BUDGET, bytes))
    return rdst_fail(RDST_ENOTSUP, "%s: LR %d x %d is larger than the LDS holds (one column of sums and one row need %lld bytes)",
                     who, oh, ow, (long long)bytes);
  const int nbr = (H + BR - 1) / BR, nbc = (W + BC - 1) / BC;
  const int64_t blocks = (int64_t)N * C * nbr * nbc;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d HR %d x %d is too large for one launch", who, N, C, H, W);
  hipLaunchKernelGGL(lrc_adjoint_kernel, dim3((unsigned)blocks), dim3(NT), (size_t)bytes, (hipStream_t)stream, g, oh, ow, H, W,
                     KyT / 4, (const int4*)index_yT, (const f4*)weight_yT, KxT / 4, (const int4*)index_xT, (const f4*)weight_xT,
                     scale_dev, scale_host, base, out, BR, nbr, BC, nbc, RC, pitch);
  return rdst_launch_status(who);
}
