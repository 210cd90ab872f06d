// Training batches cut and degraded on the device (rdst_amd/data.py): the bicubic resize of the reference's datasets
// (datasets/basic_dataset.py:65-123, cv2.resize(INTER_CUBIC) on float images) and the batch of
// BasicMultiSRTrain.__getitem__ (datasets/basic_dataset.py:190-217: one random HR crop per slice, SingleImageRandomCrop
// :482-499, and the resize of every crop down to the LR patch), which the reference builds on the CPU in DataLoader
// workers and copies to the device (models/trans_sr_trainer.py:116-121, :143).
//
// The resize is separable with four taps per axis (Keys kernel, a = -0.75, half-pixel mapping, tap indices clamped to
// the image, no antialiasing, no clamping of the values).  Tap indices and weights of an axis come from a table the host
// computed in float64 and rounded once to fp32 (rdst_amd.data.tap_table); at hp = 4 lp the taps of an LR pixel are its
// own 4 x 4 group of HR pixels with the weights -3/32, 19/32, 19/32, -3/32, which the fast path of the sampler uses
// without a table.  Every output of both entry points is formed by tap4() below: horizontal sums of the four tap rows
// first, then the vertical sum, taps in ascending order, one explicit fmaf per tap.  So a patch resized by the sampler
// equals the same patch resized by rdst_resize_bicubic bit for bit, on either path.
//
// Bandwidth kernels: no MFMA, no atomics, no scratch.  Crop origins are arbitrary, so source rows are only 4-byte
// aligned: they are read as four dwords at alignment 4 (one global_load_dwordx4 where the compiler can, which the
// hardware accepts at dword alignment); the HR and LR outputs are written with aligned 16-byte stores where
// hp % 4 == 0.
#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int LDS_BUDGET = 64 * 1024;   // the table path's tile of HR rows (the default dynamic-LDS limit)

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at dword alignment
struct __attribute__((packed, aligned(1))) u8x4 { uint32_t v; };     // four label bytes at any address

// one output value from four taps, in ascending order with one rounding per tap
__device__ __forceinline__ float tap4(float v0, float v1, float v2, float v3, float w0, float w1, float w2, float w3) {
  return fmaf(w3, v3, fmaf(w2, v2, fmaf(w1, v1, __fmul_rn(w0, v0))));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- rdst_resize_bicubic: one thread per output pixel ----------------------------------------------------------------
__global__ void __launch_bounds__(NT) resize_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int oh,
                                                    int ow, const int4* __restrict__ iy, const f4* __restrict__ wy,
                                                    const int4* __restrict__ ix, const f4* __restrict__ wx, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % ow);
  const int64_t t = i / ow;
  const int oy = (int)(t % oh);
  const int64_t plane = t / oh;
  int4 jx = ix[ox], jy = iy[oy];
  const f4 fx = wx[ox], fy = wy[oy];
  // the tables are the caller's: an index outside the image must not become an address
  jx.x = clampi(jx.x, 0, W - 1), jx.y = clampi(jx.y, 0, W - 1), jx.z = clampi(jx.z, 0, W - 1), jx.w = clampi(jx.w, 0, W - 1);
  jy.x = clampi(jy.x, 0, H - 1), jy.y = clampi(jy.y, 0, H - 1), jy.z = clampi(jy.z, 0, H - 1), jy.w = clampi(jy.w, 0, H - 1);
  const float* p = x + plane * H * W;
  const float* r0 = p + (int64_t)jy.x * W;
  const float* r1 = p + (int64_t)jy.y * W;
  const float* r2 = p + (int64_t)jy.z * W;
  const float* r3 = p + (int64_t)jy.w * W;
  const float h0 = tap4(r0[jx.x], r0[jx.y], r0[jx.z], r0[jx.w], fx.x, fx.y, fx.z, fx.w);
  const float h1 = tap4(r1[jx.x], r1[jx.y], r1[jx.z], r1[jx.w], fx.x, fx.y, fx.z, fx.w);
  const float h2 = tap4(r2[jx.x], r2[jx.y], r2[jx.z], r2[jx.w], fx.x, fx.y, fx.z, fx.w);
  const float h3 = tap4(r3[jx.x], r3[jx.y], r3[jx.z], r3[jx.w], fx.x, fx.y, fx.z, fx.w);
  y[i] = tap4(h0, h1, h2, h3, fy.x, fy.y, fy.z, fy.w);
}

// the window of patch b, clamped into the stack (the index table is device memory nobody checked)
struct Window {
  int64_t slice;
  int top, left;
};
__device__ __forceinline__ Window window_of(const int* __restrict__ index, int b, int S, int H, int W, int hp) {
  Window w;
  w.slice = clampi(index[3 * b], 0, S - 1);
  w.top = clampi(index[3 * b + 1], 0, H - hp);
  w.left = clampi(index[3 * b + 2], 0, W - hp);
  return w;
}

// ---- rdst_sample_patches, hp = 4 lp: one thread per LR pixel = per 4 x 4 group of HR pixels --------------------------
__global__ void __launch_bounds__(NT) sample4_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ labels,
                                                     const int* __restrict__ index, float* __restrict__ hr,
                                                     float* __restrict__ lr, uint8_t* __restrict__ lab, int S, int C, int H,
                                                     int W, int lp, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int hp = 4 * lp;
  const int ox = (int)(i % lp);
  int64_t t = i / lp;
  const int oy = (int)(t % lp);
  t /= lp;
  const int c = (int)(t % C);
  const int b = (int)(t / C);
  const Window w = window_of(index, b, S, H, W, hp);
  const float* src = stack + ((w.slice * C + c) * H + w.top + 4 * oy) * W + w.left + 4 * ox;
  float* dst = hr + (((int64_t)b * C + c) * hp + 4 * oy) * hp + 4 * ox;
  constexpr float K0 = -3.f / 32.f, K1 = 19.f / 32.f;
  float h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f4 v = *reinterpret_cast<const f4u*>(src + (int64_t)j * W);
    *reinterpret_cast<f4*>(dst + (int64_t)j * hp) = v;
    h[j] = tap4(v.x, v.y, v.z, v.w, K0, K1, K1, K0);
  }
  lr[i] = tap4(h[0], h[1], h[2], h[3], K0, K1, K1, K0);
  if (labels != nullptr && c == 0) {
    const uint8_t* ls = labels + (w.slice * H + w.top + 4 * oy) * W + w.left + 4 * ox;
    uint8_t* ld = lab + ((int64_t)b * hp + 4 * oy) * hp + 4 * ox;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<uint32_t*>(ld + (int64_t)j * hp) = reinterpret_cast<const u8x4*>(ls + (int64_t)j * W)->v;
  }
}

// ---- rdst_sample_patches, any ratio: one workgroup per (patch, channel, band of LB rows of the LR patch) --------------
// The bands partition the rows of the HR patch: band k owns the rows from the first tap row of its first LR row up to the
// first tap row of the next band (band 0 from row 0, the last band to row hp - 1).  A workgroup walks the rows it owns and
// the tap rows of its LR rows once: an owned row goes to the HR output, a tap row into the LDS tile, most rows both, from one
// load.  The tap rows a band shares with the next one (three at most when shrinking) are read by both, from the L2.  Then
// the LR rows are formed from the tile.  V4: hp % 4 == 0 and 16-byte aligned outputs, four pixels per lane and access.
template <bool V4>
__global__ void __launch_bounds__(NT) sample_tab_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ labels,
                                                        const int* __restrict__ index, float* __restrict__ hr,
                                                        float* __restrict__ lr, uint8_t* __restrict__ lab, int S, int C,
                                                        int H, int W, int hp, int lp, const int4* __restrict__ it,
                                                        const f4* __restrict__ wt, int LB, int nb, int max_rows) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [max_rows][hp]
  const int band = (int)(blockIdx.x % (unsigned)nb);
  const int plane = (int)(blockIdx.x / (unsigned)nb);
  const int c = plane % C, b = plane / C;
  const int o0 = band * LB, o1 = min(o0 + LB, lp);
  const Window w = window_of(index, b, S, H, W, hp);
  const int tap_lo = clampi(it[o0].x, 0, hp - 1);
  const int tap_hi = min(max(clampi(it[o1 - 1].w, 0, hp - 1) + 1, tap_lo + 1), tap_lo + max_rows);   // staged: [tap_lo, tap_hi)
  const int own_lo = band == 0 ? 0 : tap_lo;
  const int own_hi = band == nb - 1 ? hp : max(clampi(it[o1].x, 0, hp - 1), own_lo);
  const int row_lo = min(own_lo, tap_lo), row_hi = max(own_hi, tap_hi);
  const float* src = stack + ((w.slice * C + c) * H + w.top) * W + w.left;
  float* dst = hr + ((int64_t)b * C + c) * hp * hp;
  const uint8_t* ls = labels != nullptr && c == 0 ? labels + (w.slice * H + w.top) * W + w.left : nullptr;
  uint8_t* ld = lab + (int64_t)b * hp * hp;
  constexpr int V = V4 ? 4 : 1;
  const int per_row = hp / V;
  for (int e = threadIdx.x; e < (row_hi - row_lo) * per_row; e += NT) {
    const int r = row_lo + e / per_row, col = (e % per_row) * V;
    const bool own = r >= own_lo && r < own_hi, tap = r >= tap_lo && r < tap_hi;
    if (!own && !tap) continue;
    if (V4) {
      const f4 v = *reinterpret_cast<const f4u*>(src + (int64_t)r * W + col);
      if (own) *reinterpret_cast<f4*>(dst + (int64_t)r * hp + col) = v;
      if (tap) *reinterpret_cast<f4*>(tile + (r - tap_lo) * hp + col) = v;
      if (own && ls != nullptr)
        *reinterpret_cast<uint32_t*>(ld + (int64_t)r * hp + col) = reinterpret_cast<const u8x4*>(ls + (int64_t)r * W + col)->v;
    } else {
      const float v = src[(int64_t)r * W + col];
      if (own) dst[(int64_t)r * hp + col] = v;
      if (tap) tile[(r - tap_lo) * hp + col] = v;
      if (own && ls != nullptr) ld[(int64_t)r * hp + col] = ls[(int64_t)r * W + col];
    }
  }
  __syncthreads();
  const int staged = tap_hi - tap_lo;
  float* out = lr + ((int64_t)b * C + c) * lp * lp;
  for (int e = threadIdx.x; e < (o1 - o0) * lp; e += NT) {
    const int oy = o0 + e / lp, ox = e % lp;
    const int4 jx = it[ox], jy = it[oy];
    const f4 fx = wt[ox], fy = wt[oy];
    const int x0 = clampi(jx.x, 0, hp - 1), x1 = clampi(jx.y, 0, hp - 1), x2 = clampi(jx.z, 0, hp - 1), x3 = clampi(jx.w, 0, hp - 1);
    // (a well-formed table keeps every tap row inside the staged rows; the clamp is for the other kind)
    const float* r0 = tile + clampi(clampi(jy.x, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float* r1 = tile + clampi(clampi(jy.y, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float* r2 = tile + clampi(clampi(jy.z, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float* r3 = tile + clampi(clampi(jy.w, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float h0 = tap4(r0[x0], r0[x1], r0[x2], r0[x3], fx.x, fx.y, fx.z, fx.w);
    const float h1 = tap4(r1[x0], r1[x1], r1[x2], r1[x3], fx.x, fx.y, fx.z, fx.w);
    const float h2 = tap4(r2[x0], r2[x1], r2[x2], r2[x3], fx.x, fx.y, fx.z, fx.w);
    const float h3 = tap4(r3[x0], r3[x1], r3[x2], r3[x3], fx.x, fx.y, fx.z, fx.w);
    out[(int64_t)oy * lp + ox] = tap4(h0, h1, h2, h3, fy.x, fy.y, fy.z, fy.w);
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int rdst_resize_bicubic(const float* x, float* y, int N, int C, int H, int W, int oh, int ow,
                                   const int32_t* tap_index_y, const float* tap_weight_y, const int32_t* tap_index_x,
                                   const float* tap_weight_x, void* stream) {
  const char* who = "rdst_resize_bicubic";
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d -> %d x %d", who, N, C, H, W, oh, ow);
  if (!x || !y || !tap_index_y || !tap_weight_y || !tap_index_x || !tap_weight_x)
    return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if (!aligned16(tap_index_y) || !aligned16(tap_weight_y) || !aligned16(tap_index_x) || !aligned16(tap_weight_x))
    return rdst_fail(RDST_EINVAL, "%s: the tap tables must be 16-byte aligned", who);
  const int64_t total = (int64_t)N * C * oh * ow;
  const int64_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: %lld output pixels are too many for one launch", who, (long long)total);
  hipLaunchKernelGGL(resize_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, y, H, W, oh, ow,
                     (const int4*)tap_index_y, (const f4*)tap_weight_y, (const int4*)tap_index_x, (const f4*)tap_weight_x,
                     total);
  return rdst_launch_status(who);
}

extern "C" int rdst_sample_patches(const float* stack, const uint8_t* labels, const int32_t* index, float* hr, float* lr,
                                   uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp,
                                   const int32_t* tap_index, const float* tap_weight, void* stream) {
  const char* who = "rdst_sample_patches";
  if (S <= 0 || C <= 0 || H <= 0 || W <= 0 || B <= 0 || hp <= 0 || lp <= 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape S=%d C=%d H=%d W=%d B=%d hp=%d lp=%d", who, S, C, H, W, B, hp, lp);
  if (hp > H || hp > W) return rdst_fail(RDST_EINVAL, "%s: a %d x %d patch does not fit a %d x %d slice", who, hp, hp, H, W);
  if (!stack || !index || !hr || !lr) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if ((labels != nullptr) != (label_out != nullptr))
    return rdst_fail(RDST_EINVAL, "%s: labels and label_out go together", who);
  if ((int64_t)B * C * hp * hp > ((int64_t)1 << 40) || (int64_t)B * C > (1 << 20))
    return rdst_fail(RDST_EINVAL, "%s: B=%d C=%d hp=%d is too large for one launch", who, B, C, hp);
  hipStream_t st = (hipStream_t)stream;
  const bool wide = hp % 4 == 0 && aligned16(hr) && (label_out == nullptr || ((uintptr_t)label_out & 3) == 0);
  if (hp == 4 * lp && wide) {
    const int64_t total = (int64_t)B * C * lp * lp;
    hipLaunchKernelGGL(sample4_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, stack, labels, index, hr, lr,
                       label_out, S, C, H, W, lp, total);
    return rdst_launch_status(who);
  }
  if (!tap_index || !tap_weight) return rdst_fail(RDST_EINVAL, "%s: hp=%d lp=%d needs the tap table", who, hp, lp);
  if (!aligned16(tap_index) || !aligned16(tap_weight)) return rdst_fail(RDST_EINVAL, "%s: the tap table must be 16-byte aligned", who);
  // LB LR rows per band: the largest power of two whose tap rows, (LB - 1) hp / lp + 5 at most, fit the tile
  int LB = 32, max_rows = 0;
  for (; LB >= 1; LB >>= 1) {
    max_rows = (int)(((int64_t)(LB - 1) * hp + lp - 1) / lp) + 5;
    if (max_rows > hp) max_rows = hp;
    if ((int64_t)max_rows * hp * (int64_t)sizeof(float) <= LDS_BUDGET) break;
  }
  if (LB < 1) return rdst_fail(RDST_ENOTSUP, "%s: hp=%d is wider than the table path's tile holds", who, hp);
  const int nb = (lp + LB - 1) / LB;
  const int smem = max_rows * hp * (int)sizeof(float);
  const unsigned grid = (unsigned)((int64_t)B * C * nb);
  if (wide)
    hipLaunchKernelGGL(sample_tab_kernel<true>, dim3(grid), dim3(NT), smem, st, stack, labels, index, hr, lr, label_out, S, C, H,
                       W, hp, lp, (const int4*)tap_index, (const f4*)tap_weight, LB, nb, max_rows);
  else
    hipLaunchKernelGGL(sample_tab_kernel<false>, dim3(grid), dim3(NT), smem, st, stack, labels, index, hr, lr, label_out, S, C,
                       H, W, hp, lp, (const int4*)tap_index, (const f4*)tap_weight, LB, nb, max_rows);
  return rdst_launch_status(who);
}
