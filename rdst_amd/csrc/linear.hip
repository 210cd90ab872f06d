// K3: (LayerNorm | activation ->) Linear (-> *scale + residual), forward and backward.
// Reference sequences replaced: see include/rdst_hip.h (rdst_ln_linear_fwd / _bwd).
// This file holds the shape-generic fp32-math implementation built on gemm_valu.h plus the row-wise
// LayerNorm kernels; the MFMA fast paths for the shapes of the shipped configs live in
// linear_mfma.hip and are dispatched from here.
#include "common.h"
#include "gemm_valu.h"
#include "linear.h"
#include "pack.h"

// out[i] = sum_s slab[s*n + i]: 16 outputs x 16 slab-groups per block (short dependent chains: these
// reductions are latency-bound), fixed summation order => reproducible
__global__ void __launch_bounds__(256) slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ out,
                                                          int S, int64_t n) {
  __shared__ float part[16][17];
  const int o = threadIdx.x & 15, sg = threadIdx.x >> 4;
  const int64_t i = (int64_t)blockIdx.x * 16 + o;
  float a = 0.f;
  if (i < n)
    for (int s = sg; s < S; s += 16) a += slab[(int64_t)s * n + i];
  part[sg][o] = a;
  __syncthreads();
  if (sg == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][o];
    out[i] = t;
  }
}

int slab_reduce(const float* slab, float* out, int S, int64_t n, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, slab, out, S, n);
  return rdst_launch_status("slab_reduce");
}

// slab [S][2][K] -> out_a[K] (first half), out_b[K] (second half); either may be NULL.
// One wave per output (4 outputs per block): lanes stride over the S slab rows with independent loads and
// combine with a fixed shuffle tree, so the result is reproducible and the kernel is not a serial chain.
__global__ void __launch_bounds__(256) slab_reduce2_kernel(const float* __restrict__ slab, float* __restrict__ out_a,
                                                           float* __restrict__ out_b, int S, int K) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= 2 * K) return;
  float a = 0.f;
  for (int s = lane; s < S; s += 64) a += slab[(int64_t)s * 2 * K + i];
  a = wave_sum(a);
  if (lane == 0) {
    if (i < K) { if (out_a) out_a[i] = a; }
    else if (out_b) out_b[i - K] = a;
  }
}

int slab_reduce2(const float* slab, float* out_a, float* out_b, int S, int K, hipStream_t st) {
  if (K <= 0 || (!out_a && !out_b)) return 0;
  hipLaunchKernelGGL(slab_reduce2_kernel, dim3((unsigned)((2 * K + 3) / 4)), dim3(256), 0, st, slab, out_a, out_b, S, K);
  return rdst_launch_status("slab_reduce2");
}

namespace {

constexpr float kLnEps = 1e-5f;  // nn.LayerNorm default

// ---- LayerNorm row statistics: one wave per row ------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) row_stats_kernel(const T* __restrict__ X, int64_t ldx, float* __restrict__ stats,
                                                        int64_t M, int K) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const T* x = X + row * ldx;
  float s = 0.f;
  for (int k = lane; k < K; k += 64) s += to_f32<T>(x[k]);
  const float mean = wave_sum(s) / (float)K;
  float v = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float d = to_f32<T>(x[k]) - mean;
    v = fmaf(d, d, v);
  }
  const float var = wave_sum(v) / (float)K;
  if (lane == 0) {
    stats[row * 2] = mean;
    stats[row * 2 + 1] = 1.0f / sqrtf(var + kLnEps);
  }
}

// ---- LayerNorm only: Y = LN(X)*s + R -------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) ln_apply_kernel(const T* __restrict__ X, int64_t ldx, const float* __restrict__ stats,
                                                       const float* __restrict__ g, const float* __restrict__ b,
                                                       const T* R, int64_t ldr, T* Y, int64_t ldy, int64_t M, int K,
                                                       float s) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * K) return;
  const int64_t m = i / K;
  const int k = (int)(i - m * K);
  float v = (to_f32<T>(X[m * ldx + k]) - stats[2 * m]) * stats[2 * m + 1] * g[k] + b[k];
  v *= s;
  if (R) v += to_f32<T>(R[m * ldr + k]);
  Y[m * ldy + k] = from_f32<T>(v);
}

// ---- LayerNorm-only rows, bf16, 8 <= K <= 64 (the patch norm and the final norm of RDSTSR: K = 60): 8 lanes per row ------
// A row's K channels are 8 chunks of 16 B (lane = chunk, the last chunk of a row that is not a multiple of 8 overlaps its
// neighbour and counts only its own channels), a wave works on 8 rows at once, row sums over the 8 lanes on the DPP path.
// Forward: statistics + apply in one pass (was row_stats_kernel + ln_apply_kernel: one wave per row, 2-byte loads);
// backward: dY read as it lies (was scale_to_f32_kernel into an fp32 copy + ln_bwd_rows_kernel: one wave per row).
typedef uint32_t ln8_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
__device__ __forceinline__ float ln8_sum8(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xf, 0xf, true));   // row_half_mirror
  return v;
}
__device__ __forceinline__ void ln8_unpack(const ln8_u32x4& v, float (&f)[8]) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u); f[2] = __uint_as_float(v.y << 16);
  f[3] = __uint_as_float(v.y & 0xffff0000u); f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ uint32_t ln8_pack2(float a, float b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, __float2bfloat16(a)) | ((uint32_t)__builtin_bit_cast(uint16_t, __float2bfloat16(b)) << 16);
}
// a lane's 8 channels of a row: one 16-byte load (bf16) or two (fp32 rows: round 6 — the fp32 modes still ran row_stats + ln_apply and
// scale_to_f32 + ln_bwd_rows, one wave per row: 0.24 ms of the fp32x3 step for the two LayerNorm-only layers)
template <typename T>
__device__ __forceinline__ void ln8_load(const T* p, float (&f)[8]) {
  if constexpr (sizeof(T) == 2) {
    ln8_unpack(*reinterpret_cast<const ln8_u32x4*>(p), f);
  } else {
    const ln8_u32x4 a = *reinterpret_cast<const ln8_u32x4*>(p), b = *reinterpret_cast<const ln8_u32x4*>(p + 4);
    f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y); f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
    f[4] = __uint_as_float(b.x); f[5] = __uint_as_float(b.y); f[6] = __uint_as_float(b.z); f[7] = __uint_as_float(b.w);
  }
}
struct Ln8Lane { int c0, lo; bool on; };
__device__ __forceinline__ Ln8Lane ln8_lane(int grp, int K) {
  Ln8Lane l;
  l.on = 8 * grp < K;
  l.c0 = 8 * grp + 8 <= K ? 8 * grp : K - 8;
  l.lo = 8 * grp - l.c0;
  if (!l.on) { l.c0 = 0; l.lo = 8; }
  return l;
}
__device__ __forceinline__ void ln8_store(float* dst, const float (&o)[8], const Ln8Lane& l) {
  if (!l.on) return;
  if (l.lo == 0) {
    ln8_u32x4 u, v;
    u.x = __float_as_uint(o[0]); u.y = __float_as_uint(o[1]); u.z = __float_as_uint(o[2]); u.w = __float_as_uint(o[3]);
    v.x = __float_as_uint(o[4]); v.y = __float_as_uint(o[5]); v.z = __float_as_uint(o[6]); v.w = __float_as_uint(o[7]);
    *reinterpret_cast<ln8_u32x4*>(dst + l.c0) = u;
    *reinterpret_cast<ln8_u32x4*>(dst + l.c0 + 4) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e >= l.lo) dst[l.c0 + e] = o[e];
  }
}
__device__ __forceinline__ void ln8_store(bf16* dst, const float (&o)[8], const Ln8Lane& l) {
  if (!l.on) return;
  if (l.lo == 0) {
    ln8_u32x4 u;
    u.x = ln8_pack2(o[0], o[1]); u.y = ln8_pack2(o[2], o[3]); u.z = ln8_pack2(o[4], o[5]); u.w = ln8_pack2(o[6], o[7]);
    *reinterpret_cast<ln8_u32x4*>(dst + l.c0) = u;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e >= l.lo) dst[l.c0 + e] = __float2bfloat16(o[e]);
  }
}

template <typename T>
__global__ void __launch_bounds__(256) ln8_fwd_kernel(const T* __restrict__ X, int64_t ldx, const float* __restrict__ g,
                                                      const float* __restrict__ b, const T* R, int64_t ldr, T* Y, int64_t ldy,
                                                      float* __restrict__ stats, int64_t M, int K, float s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ps = lane >> 3, grp = lane & 7;
  const Ln8Lane l = ln8_lane(grp, K);
  float gm[8], bt[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { gm[e] = g[l.c0 + e]; bt[e] = b[l.c0 + e]; }
  const float invK = 1.0f / (float)K;
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 8; r0 < M; r0 += (int64_t)gridDim.x * 32) {
    const int64_t row = r0 + ps < M ? r0 + ps : M - 1;
    const bool valid = r0 + ps < M;
    float f[8];
    ln8_load<T>(X + row * ldx + l.c0, f);
    float sum = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) sum += (l.on && e >= l.lo) ? f[e] : 0.f;
    const float mean = ln8_sum8(sum) * invK;
    float sq = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] -= mean;
      sq = (l.on && e >= l.lo) ? fmaf(f[e], f[e], sq) : sq;
    }
    const float rstd = 1.0f / sqrtf(ln8_sum8(sq) * invK + kLnEps);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (f[e] * rstd * gm[e] + bt[e]) * s;
    if (R) {
      float rr[8];
      ln8_load<T>(R + row * ldr + l.c0, rr);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] += rr[e];
    }
    if (valid) {
      ln8_store(Y + row * ldy, o, l);
      if (grp == 0) *reinterpret_cast<float2*>(stats + 2 * row) = make_float2(mean, rstd);
    }
  }
}

// dX = rstd (g - mean(g) - xhat mean(g xhat)) + acc, g = dY s gamma; per-block partial d(gamma) / d(beta) -> slab [block][2][K]
template <typename T>
__global__ void __launch_bounds__(256) ln8_bwd_kernel(const T* __restrict__ dY, int64_t lddy, const T* __restrict__ X, int64_t ldx,
                                                      const float* __restrict__ stats, const float* __restrict__ gamma, T* dX,
                                                      int64_t lddx, const T* acc, int64_t ldacc, float* __restrict__ slab, int64_t M,
                                                      int K, float s) {
  __shared__ float red[4][2][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, ps = lane >> 3, grp = lane & 7;
  const Ln8Lane l = ln8_lane(grp, K);
  float gm[8], dg[8], db[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { gm[e] = gamma[l.c0 + e]; dg[e] = 0.f; db[e] = 0.f; }
  const float invK = 1.0f / (float)K;
  for (int64_t r0 = ((int64_t)blockIdx.x * 4 + wave) * 8; r0 < M; r0 += (int64_t)gridDim.x * 32) {
    const int64_t row = r0 + ps < M ? r0 + ps : M - 1;
    const bool valid = r0 + ps < M;
    const float2 st = *reinterpret_cast<const float2*>(stats + 2 * row);
    float da[8], xh[8], gg[8];
    ln8_load<T>(dY + row * lddy + l.c0, da);
    ln8_load<T>(X + row * ldx + l.c0, xh);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool mine = l.on && e >= l.lo && valid;
      da[e] = mine ? da[e] * s : 0.f;
      xh[e] = (xh[e] - st.x) * st.y;
      gg[e] = da[e] * gm[e];
      s1 += gg[e];
      s2 = fmaf(gg[e], xh[e], s2);
      dg[e] = fmaf(da[e], xh[e], dg[e]);
      db[e] += da[e];
    }
    s1 = ln8_sum8(s1) * invK;
    s2 = ln8_sum8(s2) * invK;
    if (dX && valid) {
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = st.y * (gg[e] - s1 - xh[e] * s2);
      if (acc) {
        float a[8];
        ln8_load<T>(acc + row * ldacc + l.c0, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += a[e];
      }
      ln8_store(dX + row * lddx, o, l);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {   // the 8 row slots of the wave (lane bits 3..5), fixed butterfly
    dg[e] += __shfl_xor(dg[e], 8, 64); dg[e] += __shfl_xor(dg[e], 16, 64); dg[e] += __shfl_xor(dg[e], 32, 64);
    db[e] += __shfl_xor(db[e], 8, 64); db[e] += __shfl_xor(db[e], 16, 64); db[e] += __shfl_xor(db[e], 32, 64);
  }
  if (ps == 0 && l.on)
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e >= l.lo) { red[wave][0][l.c0 + e] = dg[e]; red[wave][1][l.c0 + e] = db[e]; }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * K; i += 256) {
    const int which = i / K, k = i - which * K;
    slab[(int64_t)blockIdx.x * 2 * K + i] = red[0][which][k] + red[1][which][k] + red[2][which][k] + red[3][which][k];
  }
}
static inline bool ln8_ok(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc, int K, int elt = 2) {
  auto al = [elt](const void* q, int64_t l) { return ((uintptr_t)q & 3) == 0 && (elt == 4 || (l & 1) == 0); };
  return K >= 8 && K <= 64 && (K & 1) == 0 && al(a, lda) && al(b, ldb) && al(c, ldc);
}

// ---- functors -------------------------------------------------------------------------------------
template <typename T>
struct LinIn {  // f(X)[m][k]
  static constexpr bool kFast = true;
  const T* X; int64_t ldx; const float* stats; const float* g; const float* b; int act;
  __device__ __forceinline__ float operator()(int64_t m, int64_t k) const {
    float v = to_f32<T>(X[m * ldx + k]);
    if (g) return (v - stats[2 * m]) * stats[2 * m + 1] * g[k] + b[k];
    return apply_act(v, act);
  }
};
template <typename T>
struct LinInT {  // same matrix as B operand of the wgrad GEMM: B(k = m_row, n = k_col)
  static constexpr bool kFast = false;
  LinIn<T> f;
  __device__ __forceinline__ float operator()(int64_t m, int k) const { return f(m, k); }
};
struct WtB {  // B(k, n) = Wt[n][k]
  static constexpr bool kFast = true;
  const float* Wt; int K;
  __device__ __forceinline__ float operator()(int64_t k, int n) const { return Wt[(int64_t)n * K + k]; }
};
struct WtBT {  // B(n_idx as k, k_idx as n) = Wt[n_idx][k_idx]
  static constexpr bool kFast = false;
  const float* Wt; int K;
  __device__ __forceinline__ float operator()(int64_t n_idx, int k_idx) const { return Wt[n_idx * K + k_idx]; }
};
template <typename T>
struct DyA {  // A(m, n) = dY[m][n] * s
  static constexpr bool kFast = true;
  const T* dY; int64_t ld; float s;
  __device__ __forceinline__ float operator()(int64_t m, int64_t n) const { return to_f32<T>(dY[m * ld + n]) * s; }
};
template <typename T>
struct DyAT {  // A(n, m) = dY[m][n] * s   (wgrad: rows of the output are n)
  static constexpr bool kFast = false;
  const T* dY; int64_t ld; float s;
  __device__ __forceinline__ float operator()(int64_t n, int64_t m) const { return to_f32<T>(dY[m * ld + n]) * s; }
};
template <typename T>
struct DyCol {  // colsum functor
  const T* dY; int64_t ld; float s;
  __device__ __forceinline__ float operator()(int64_t m, int n) const { return to_f32<T>(dY[m * ld + n]) * s; }
};

template <typename T>
struct FwdEp {
  const float* bias; const T* R; int64_t ldr; T* Y; int64_t ldy; float s;
  __device__ __forceinline__ void operator()(int64_t m, int n, float acc, int) const {
    float v = acc + (bias ? bias[n] : 0.f);
    v *= s;
    if (R) v += to_f32<T>(R[m * ldr + n]);
    Y[m * ldy + n] = from_f32<T>(v);
  }
};
struct SlabEp {  // split-K partials of an (rows x cols) matrix
  float* slab; int64_t n_total; int cols;
  __device__ __forceinline__ void operator()(int64_t r, int c, float acc, int z) const {
    slab[(int64_t)z * n_total + r * cols + c] = acc;
  }
};
struct DaEp {  // LN case: keep d(LN output) in fp32 for the row-wise LN backward
  float* dA; int K;
  __device__ __forceinline__ void operator()(int64_t m, int k, float acc, int) const { dA[m * K + k] = acc; }
};
template <typename T>
struct DxEp {  // no LN: dX = dA * act'(X) (+ existing dX)
  const T* X; int64_t ldx; T* dX; int64_t lddx; int act; const T* addp; int64_t ldacc;
  __device__ __forceinline__ void operator()(int64_t m, int k, float acc, int) const {
    float v = acc;
    if (act) v *= act_grad(to_f32<T>(X[m * ldx + k]), act);
    if (addp) v += to_f32<T>(addp[m * ldacc + k]);
    dX[m * lddx + k] = from_f32<T>(v);
  }
};

// ---- LayerNorm backward, one wave per row, K <= 64*KC --------------------------------------------
// dX = rstd * (g - mean(g) - xhat * mean(g*xhat)),  g = dA * gamma;  partial dgamma/dbeta per block.
template <typename T, int KC>
__global__ void __launch_bounds__(256)
ln_bwd_rows_kernel(const float* __restrict__ dA, const T* __restrict__ X, int64_t ldx, const float* __restrict__ stats,
                   const float* __restrict__ gamma, T* dX, int64_t lddx, const T* acc, int64_t ldacc,
                   float* __restrict__ slab,
                   int64_t M, int K) {
  __shared__ float red[4][2][64 * KC];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float dg[KC], db[KC], gm[KC];
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    dg[c] = 0.f;
    db[c] = 0.f;
    const int k = lane + 64 * c;
    gm[c] = k < K ? gamma[k] : 0.f;
  }
  const float invK = 1.0f / (float)K;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < M; row += (int64_t)gridDim.x * 4) {
    const float mean = stats[2 * row], rstd = stats[2 * row + 1];
    float xh[KC], g[KC];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int k = lane + 64 * c;
      if (k < K) {
        const float da = dA[row * K + k];
        xh[c] = (to_f32<T>(X[row * ldx + k]) - mean) * rstd;
        g[c] = da * gm[c];
        s1 += g[c];
        s2 = fmaf(g[c], xh[c], s2);
        dg[c] = fmaf(da, xh[c], dg[c]);
        db[c] += da;
      } else {
        xh[c] = 0.f;
        g[c] = 0.f;
      }
    }
    s1 = wave_sum(s1) * invK;
    s2 = wave_sum(s2) * invK;
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int k = lane + 64 * c;
      if (k < K) {
        float v = rstd * (g[c] - s1 - xh[c] * s2);
        if (dX) {
          if (acc) v += to_f32<T>(acc[row * ldacc + k]);
          dX[row * lddx + k] = from_f32<T>(v);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < KC; ++c) {
    red[wave][0][lane + 64 * c] = dg[c];
    red[wave][1][lane + 64 * c] = db[c];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * K; i += 256) {
    const int which = i / K, k = i - which * K;
    const float a = red[0][which][k] + red[1][which][k] + red[2][which][k] + red[3][which][k];
    slab[(int64_t)blockIdx.x * 2 * K + i] = a;  // [block][2][K]
  }
}

template <typename T>
int fwd_t(const T* X, int64_t ldx, const float* ln_w, const float* ln_b, int in_act, const float* Wt, const float* bias,
          const T* R, int64_t ldr, T* Y, int64_t ldy, float* stats, int64_t M, int K, int N, float s, bool split, hipStream_t st) {
  auto run_stats = [&]() -> int {
    hipLaunchKernelGGL((row_stats_kernel<T>), dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, X, ldx, stats, M, K);
    return rdst_launch_status("row_stats");
  };
  if (!Wt) {
    if (ln8_ok(X, ldx, Y, ldy, R, ldr, K, (int)sizeof(T))) {
      const int64_t nb = (M + 31) / 32;
      hipLaunchKernelGGL((ln8_fwd_kernel<T>), dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, st, X, ldx, ln_w, ln_b, R, ldr, Y, ldy,
                         stats, M, K, s);
      return rdst_launch_status("ln8_fwd");
    }
    if (int rc = run_stats()) return rc;
    const int64_t n = M * K;
    hipLaunchKernelGGL((ln_apply_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, X, ldx, stats, ln_w,
                       ln_b, R, ldr, Y, ldy, M, K, s);
    return rdst_launch_status("ln_apply");
  }
  // the MFMA path computes (and stores) the LayerNorm statistics itself
  if (int rc = linear_fwd_mfma<T>(X, ldx, ln_w, ln_b, in_act, Wt, bias, R, ldr, Y, ldy, stats, M, K, N, s, split, st);
      rc != RDST_ENOTSUP)
    return rc;
  if (ln_w)
    if (int rc = run_stats()) return rc;
  LinIn<T> la{X, ldx, stats, ln_w, ln_b, in_act};
  WtB lb{Wt, K};
  FwdEp<T> ep{bias, R, ldr, Y, ldy, s};
  return gemm_valu_launch(la, lb, ep, M, N, K, 1, st, "linear_fwd");
}

template <typename T>
int bwd_t(const T* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* stats, int in_act, const float* Wt,
          const T* dY, int64_t lddy, T* dX, int64_t lddx, const T* acc, int64_t ldacc, float* dW, float* dbias,
          float* dln_w,
          float* dln_b, float* wsp, int64_t M, int K, int N, float s, bool split, hipStream_t st, const T* acc2, int64_t ldacc2) {
  const LinBwdWs w = lin_bwd_layout(wsp, M, K, N, ln_w != nullptr, true);
  float* const dA = w.dA;
  const WsSlab& slabW = w.slabW;
  const WsSlab& small = w.small;
  if constexpr (sizeof(T) == 4) {   // RDST_F32X3: the one-pass kernel of the E1 shapes (every gradient requested), else the paths below
    if (split && Wt && dX && dW && dbias && (!ln_w || (dln_w && dln_b && w.G)) && !rdst_dbg_getenv("RDST_LBX_OFF")) {
      const int rc = lnlin3x_bwd_f32(X, ldx, ln_w, ln_b, stats, in_act, Wt, dY, lddy, dX, lddx, acc, ldacc, acc2, ldacc2, dW, dbias, dln_w,
                                     dln_b, slabW, w.G, M, K, N, s, st);
      if (rc != RDST_ENOTSUP) return rc;
    }
  }
  if (acc2) {   // a second addend of dX: only the one-pass LayerNorm-Linear backward of the E1 shapes takes it (nothing is launched otherwise)
    if constexpr (sizeof(T) == 2) {
      if (Wt && ln_w && ln_b && dW && dbias && dln_w && dln_b && dX && K <= 128 && w.G)
        return linear_ln_bwd_fused_bf16(X, ldx, ln_w, ln_b, stats, Wt, dY, lddy, dX, lddx, acc, ldacc, dW, dbias, dln_w, dln_b, slabW,
                                        w.G, M, K, N, s, st, acc2, ldacc2);
    }
    return RDST_ENOTSUP;
  }
  LinIn<T> fin{X, ldx, stats, ln_w, ln_b, in_act};
  if (Wt) {
    // LayerNorm-fused Linear with everything requested in one call: the weight-gradient pass runs on x-hat and
    // its reduction also yields d(gamma)/d(beta); the data-gradient kernel then only produces dX.
    if (ln_w && ln_b && dW && dbias && dln_w && dln_b && dX && K <= 128 && !rdst_dbg_getenv("RDST_LN_BWD_V1")) {
      if (float* G = w.G) {   // the fp32 dA buffer of the generic path is unused here: N*(K+1) floats of scratch where they fit
        if constexpr (sizeof(T) == 2) {   // one pass over (x, dY) for everything, where the shape is covered
          const int rcf = linear_ln_bwd_fused_bf16(X, ldx, ln_w, ln_b, stats, Wt, dY, lddy, dX, lddx, acc, ldacc, dW, dbias, dln_w,
                                                   dln_b, slabW, G, M, K, N, s, st);
          if (rcf != RDST_ENOTSUP) return rcf;
        }
        int rc = linear_wgrad_ln_mfma<T>(X, ldx, ln_w, ln_b, stats, Wt, dY, lddy, dW, dbias, dln_w, dln_b, slabW, G, M, K, N,
                                         s, split, st);
        if (rc == 0) {
          rc = linear_dgrad_ln2_mfma<T>(X, ldx, stats, ln_w, Wt, dY, lddy, dX, lddx, acc, ldacc, M, K, N, s, split, st);
          if (rc == 0) return 0;
          if (rc != RDST_ENOTSUP) return rc;
          if (N >= 64) {
            // N too wide for the kernel's resident weights (fp32 qkv at C = 90 / 120: 3C x C floats > LDS): the data gradient is
            // LINEAR in dY — dX = LN'(dY[:, :N1] W[:N1]) + LN'(dY[:, N1:] W[N1:]) — so two launches over halves of the
            // output features, the second accumulating onto the first (in place), replace the scalar GEMM + LayerNorm-backward
            // pair this shape used to fall back to
            const int N1 = (N / 2 + 3) / 4 * 4;
            rc = linear_dgrad_ln2_mfma<T>(X, ldx, stats, ln_w, Wt, dY, lddy, dX, lddx, acc, ldacc, M, K, N1, s, split, st);
            if (rc == 0) {
              rc = linear_dgrad_ln2_mfma<T>(X, ldx, stats, ln_w, Wt + (int64_t)N1 * K, dY + N1, lddy, dX, lddx, dX, lddx, M, K, N - N1, s, split, st);
              if (rc != RDST_ENOTSUP) return rc;   // (a refused SECOND half leaves dX half done: rebuilt from scratch below)
            } else if (rc != RDST_ENOTSUP) {
              return rc;
            }
          }
          // dX not covered: finish it below; dW / dbias / d(gamma) / d(beta) are done
          dW = nullptr; dbias = nullptr; dln_w = nullptr; dln_b = nullptr;
        } else if (rc != RDST_ENOTSUP) {
          return rc;
        }
      }
    }
    if constexpr (sizeof(T) == 2) {   // plain Linear (proj): dX, dW, dbias in one pass over (x, dY)
      if (!ln_w && !in_act && dW && dbias && dX) {
        const int rcf = linear_ln_bwd_fused_bf16(X, ldx, nullptr, nullptr, nullptr, Wt, dY, lddy, dX, lddx, acc, ldacc, dW, dbias,
                                                 nullptr, nullptr, slabW, nullptr, M, K, N, s, st);
        if (rcf != RDST_ENOTSUP) return rcf;
      }
    }
    bool wgrad_done = false;
    if (dW || dbias) {
      const int rc = linear_wgrad_mfma<T>(X, ldx, ln_w, ln_b, stats, in_act, dY, lddy, dW, dbias, slabW, M, K, N, s, split, st);
      if (rc == 0) wgrad_done = true;
      else if (rc != RDST_ENOTSUP) return rc;
    }
    if (!wgrad_done && dbias) {
      DyCol<T> f{dY, lddy, s};
      if (int rc = colsum_launch(f, M, N, small, dbias, st, "linear_dbias")) return rc;
    }
    if (!wgrad_done && dW) {
      DyAT<T> la{dY, lddy, s};
      LinInT<T> lb{fin};
      SlabEp ep{slabW.p, (int64_t)N * K, K};
      const int z = gemm_valu_splits(M, kLinWgradSplits);
      if (int rc2 = rdst_slab_fits(slabW, z, (int64_t)N * K, "linear_wgrad")) return rc2;
      if (int rc2 = gemm_valu_launch(la, lb, ep, N, K, M, kLinWgradSplits, st, "linear_wgrad")) return rc2;
      if (int rc2 = slab_reduce(slabW.p, dW, z, (int64_t)N * K, st)) return rc2;
    }
    if (dX && ln_w) {  // fused dgrad + LayerNorm backward
      int nslab = 0;
      const int rc = linear_dgrad_ln_mfma<T>(X, ldx, stats, ln_w, Wt, dY, lddy, dX, lddx, acc, ldacc, small, &nslab, M, K,
                                             N, s, st);
      if (rc == 0) {
        return slab_reduce2(small.p, dln_w, dln_b, nslab, K, st);
      }
      if (rc != RDST_ENOTSUP) return rc;
    }
    // behind a LayerNorm, d(gamma) / d(beta) need dA = s dY W as much as dX does (a frozen input in front of a trainable norm):
    // the row kernel below reads it whether or not dX is wanted
    if (dX || (ln_w && (dln_w || dln_b))) {
      int rc = linear_dgrad_mfma<T>(X, ldx, ln_w != nullptr, in_act, Wt, dY, lddy, dX, lddx, acc, ldacc, dA, M, K, N, s, split, st);
      if (rc == RDST_ENOTSUP) {
        DyA<T> la{dY, lddy, s};
        WtBT lb{Wt, K};
        if (ln_w) {
          DaEp ep{dA, K};
          rc = gemm_valu_launch(la, lb, ep, M, K, N, 1, st, "linear_dgrad");
        } else {
          DxEp<T> ep{X, ldx, dX, lddx, in_act, acc, ldacc};
          rc = gemm_valu_launch(la, lb, ep, M, K, N, 1, st, "linear_dgrad");
        }
      }
      if (rc) return rc;
    }
  }
  if (ln_w) {
    const float* dAsrc = dA;
    if (!dX && !dln_w && !dln_b) return 0;
    if (K > 512) return rdst_fail(RDST_ENOTSUP, "rdst_ln_linear_bwd: LayerNorm width %d > 512", K);
    const int blocks = (int)small.cap((M + 3) / 4 < kSmallBlocks ? (M + 3) / 4 : kSmallBlocks, 2 * K);
    if (int rc = rdst_slab_fits(small, blocks, 2 * K, "ln_bwd_rows")) return rc;
    const int kc = (K + 63) / 64;
#define RDST_LNB(KC)                                                                                              \
  hipLaunchKernelGGL((ln_bwd_rows_kernel<T, KC>), dim3(blocks), dim3(256), 0, st, dAsrc, X, ldx, stats, ln_w, dX, \
                     lddx, acc, ldacc, small.p, M, K)
    if (kc <= 1) RDST_LNB(1); else if (kc <= 2) RDST_LNB(2); else if (kc <= 4) RDST_LNB(4); else RDST_LNB(8);
#undef RDST_LNB
    if (int rc = rdst_launch_status("ln_bwd_rows")) return rc;
    // slab is [blocks][2][K] -> reduce to a [2][K] scratch then copy out
    if (int rc = slab_reduce2(small.p, dln_w, dln_b, blocks, K, st)) return rc;
  }
  return 0;
}

// LN-only (Wt == NULL) backward: dA = dY*s in fp32, then the row kernel.
template <typename T>
__global__ void __launch_bounds__(256) scale_to_f32_kernel(const T* __restrict__ dY, int64_t ld, float* __restrict__ dA,
                                                           int64_t M, int K, float s) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * K) return;
  const int64_t m = i / K;
  dA[i] = to_f32<T>(dY[m * ld + (i - m * K)]) * s;
}

template <typename T>
int ln_only_bwd(const T* X, int64_t ldx, const float* ln_w, const float* stats, const T* dY, int64_t lddy, T* dX,
                int64_t lddx, const T* acc, int64_t ldacc, float* dln_w, float* dln_b, float* wsp, int64_t M, int K, float s,
                hipStream_t st) {
  const LinBwdWs w = lin_bwd_layout(wsp, M, K, K, true, false);
  float* const dA = w.dA;
  const WsSlab& small = w.small;
  const int64_t n = M * K;
  if (K <= 64 && ln8_ok(X, ldx, dY, lddy, dX, lddx, K, (int)sizeof(T)) && ln8_ok(acc, ldacc, nullptr, 0, nullptr, 0, K, (int)sizeof(T))) {
    const int64_t nb = (M + 31) / 32;
    const int blocks = (int)small.cap(nb < kSmallBlocks ? nb : kSmallBlocks, 2 * K);
    if (int rc = rdst_slab_fits(small, blocks, 2 * K, "ln8_bwd")) return rc;
    hipLaunchKernelGGL((ln8_bwd_kernel<T>), dim3(blocks), dim3(256), 0, st, dY, lddy, X, ldx, stats, ln_w, dX, lddx, acc, ldacc, small.p, M, K, s);
    if (int rc = rdst_launch_status("ln8_bwd")) return rc;
    return slab_reduce2(small.p, dln_w, dln_b, blocks, K, st);
  }
  hipLaunchKernelGGL((scale_to_f32_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dY, lddy, dA, M, K, s);
  if (int rc = rdst_launch_status("scale_to_f32")) return rc;
  if (K > 512) return rdst_fail(RDST_ENOTSUP, "rdst_ln_linear_bwd: LayerNorm width %d > 512", K);
  const int blocks = (int)small.cap((M + 3) / 4 < kSmallBlocks ? (M + 3) / 4 : kSmallBlocks, 2 * K);
  if (int rc = rdst_slab_fits(small, blocks, 2 * K, "ln_bwd_rows")) return rc;
  const int kc = (K + 63) / 64;
#define RDST_LNB(KC)                                                                                           \
  hipLaunchKernelGGL((ln_bwd_rows_kernel<T, KC>), dim3(blocks), dim3(256), 0, st, dA, X, ldx, stats, ln_w, dX, \
                     lddx, acc, ldacc, small.p, M, K)
  if (kc <= 1) RDST_LNB(1); else if (kc <= 2) RDST_LNB(2); else if (kc <= 4) RDST_LNB(4); else RDST_LNB(8);
#undef RDST_LNB
  if (int rc = rdst_launch_status("ln_bwd_rows")) return rc;
  return slab_reduce2(small.p, dln_w, dln_b, blocks, K, st);
}

}  // namespace

extern "C" int rdst_ln_linear_fwd_packable(int K, int N, int has_ln, int has_residual, int in_act, int dtype) {
  bool split;
  if (rdst_dtype(dtype, split, "rdst_ln_linear_fwd_packable")) return 0;
  if (split) return lin3x_kind(K, N, has_ln != 0, has_residual != 0, in_act) != 0;   // lin3x_mfma.hip
  return dtype == RDST_BF16 && lin3_kind(K, N, has_ln != 0, has_residual != 0, in_act) != 0;   // lin3_mfma.hip
}

extern "C" size_t rdst_ln_linear_fwd_workspace(int K, int N) {
  if (K <= 0 || N <= 0) return 16;
  return lin3_pack_bytes(K, N);
}

// the same per compute mode: RDST_F32X3 reads hi / lo fragment pairs + b' (lin3x_mfma.hip), twice the bf16 image
extern "C" size_t rdst_ln_linear_fwd_workspace2(int K, int N, int dtype) {
  if (K <= 0 || N <= 0) return 16;
  return dtype == RDST_F32X3 ? lin3x_pack_bytes(K, N) : lin3_pack_bytes(K, N);
}

extern "C" int rdst_ln_linear_fwd(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, int in_act,
                                  const float* Wt, const float* bias, const void* R, int64_t ld_r, void* Y, int64_t ld_y,
                                  float* stats, void* workspace, size_t workspace_bytes, int64_t M, int K, int N,
                                  float out_scale, int dtype, void* stream) {
  bool split;
  if (int rc = rdst_dtype(dtype, split, "rdst_ln_linear_fwd")) return rc;
  if (!X || !Y) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: null pointer");
  if (M < 0 || K <= 0 || N <= 0) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: bad dimensions");
  if ((ln_w == nullptr) != (ln_b == nullptr)) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: ln_w/ln_b must come together");
  if (ln_w && !stats) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: LayerNorm needs a stats buffer");
  if (ln_w && in_act) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: LayerNorm and in_act are exclusive");
  if (!Wt && (!ln_w || N != K)) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: Wt == NULL means LayerNorm only (N == K)");
  if (ld_x < K || ld_y < N || (R && ld_r < N)) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_fwd: leading dimension too small");
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == RDST_BF16 && workspace && workspace_bytes >= rdst_ln_linear_fwd_workspace(K, N)) {
    const int rc = lin3_fwd_bf16((const bf16*)X, ld_x, ln_w, ln_b, in_act, Wt, bias, (const bf16*)R, ld_r, (bf16*)Y, ld_y, stats, M,
                                 K, N, out_scale, workspace, workspace_bytes == RDST_PREPACKED, st);
    if (rc != RDST_ENOTSUP) return rc;   // (a prepacked image the call cannot use is simply ignored)
  }
  if (split && workspace && workspace_bytes >= lin3x_pack_bytes(K, N)) {
    const int rc = lin3x_fwd_f32((const float*)X, ld_x, ln_w, ln_b, in_act, Wt, bias, (const float*)R, ld_r, (float*)Y, ld_y, stats, M,
                                 K, N, out_scale, workspace, workspace_bytes == RDST_PREPACKED, st);
    if (rc != RDST_ENOTSUP) return rc;
  }
  if (dtype == RDST_F32)
    return fwd_t<float>((const float*)X, ld_x, ln_w, ln_b, in_act, Wt, bias, (const float*)R, ld_r, (float*)Y, ld_y, stats, M, K, N, out_scale, split, st);
  return fwd_t<bf16>((const bf16*)X, ld_x, ln_w, ln_b, in_act, Wt, bias, (const bf16*)R, ld_r, (bf16*)Y, ld_y, stats, M, K, N, out_scale, false, st);
}

extern "C" size_t rdst_ln_linear_bwd_workspace(int64_t M, int K, int N) {
  if (M <= 0 || K <= 0 || N <= 0) return 0;
  return lin_bwd_layout(nullptr, M, K, N, true, true).bytes;
}

namespace {
// rdst_ln_linear_bwd / rdst_ln_linear_bwd2 after the dtype is decoded
int ln_linear_bwd(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, const float* stats, int in_act, const float* Wt,
                  const void* dY, int64_t ld_dy, void* dX, int64_t ld_dx, const void* dX_add, int64_t ld_dx_add, float* dW, float* dbias,
                  float* dln_w, float* dln_b, void* workspace, size_t workspace_bytes, int64_t M, int K, int N, float out_scale,
                  int dtype, bool split, hipStream_t st, const void* dX_add2, int64_t ld_dx_add2) {
  if (!X || !dY || !workspace) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_bwd: null pointer");
  if (M < 0 || K <= 0 || N <= 0) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_bwd: bad dimensions");
  if (ln_w && !stats) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_bwd: LayerNorm needs the forward's stats");
  if (!Wt && (!ln_w || N != K)) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_bwd: Wt == NULL means LayerNorm only (N == K)");
  if (ld_x < K || ld_dy < N || (dX && ld_dx < K)) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_bwd: leading dimension too small");
  if (workspace_bytes < rdst_ln_linear_bwd_workspace(M, K, N)) return rdst_fail(RDST_EINVAL, "rdst_ln_linear_bwd: workspace too small");
  if (M == 0) return 0;
  float* wsp = (float*)workspace;
  if (dX_add2 && (!Wt || (dtype != RDST_BF16 && !(split && lnlin3x_bwd_kind(K, N, ln_w != nullptr, in_act))))) return RDST_ENOTSUP;
  if (!Wt) {
    if (dtype == RDST_F32)
      return ln_only_bwd<float>((const float*)X, ld_x, ln_w, stats, (const float*)dY, ld_dy, (float*)dX, ld_dx, (const float*)dX_add, ld_dx_add, dln_w, dln_b, wsp, M, K, out_scale, st);
    return ln_only_bwd<bf16>((const bf16*)X, ld_x, ln_w, stats, (const bf16*)dY, ld_dy, (bf16*)dX, ld_dx, (const bf16*)dX_add, ld_dx_add, dln_w, dln_b, wsp, M, K, out_scale, st);
  }
  if (dtype == RDST_F32)
    return bwd_t<float>((const float*)X, ld_x, ln_w, ln_b, stats, in_act, Wt, (const float*)dY, ld_dy, (float*)dX, ld_dx, (const float*)dX_add, ld_dx_add, dW, dbias, dln_w, dln_b, wsp, M, K, N, out_scale, split, st,
                      (const float*)dX_add2, ld_dx_add2);
  return bwd_t<bf16>((const bf16*)X, ld_x, ln_w, ln_b, stats, in_act, Wt, (const bf16*)dY, ld_dy, (bf16*)dX, ld_dx, (const bf16*)dX_add, ld_dx_add, dW, dbias, dln_w, dln_b, wsp, M, K, N, out_scale, false, st,
                     (const bf16*)dX_add2, ld_dx_add2);
}
}  // namespace

extern "C" int rdst_ln_linear_bwd2(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, const float* stats,
                                  int in_act, const float* Wt, const void* dY, int64_t ld_dy, void* dX, int64_t ld_dx,
                                  const void* dX_add, int64_t ld_dx_add, float* dW, float* dbias, float* dln_w, float* dln_b,
                                  void* workspace,
                                  size_t workspace_bytes, int64_t M, int K, int N, float out_scale, int dtype,
                                  void* stream, const void* dX_add2, int64_t ld_dx_add2) {
  bool split;
  if (int rc = rdst_dtype(dtype, split, "rdst_ln_linear_bwd")) return rc;
  return ln_linear_bwd(X, ld_x, ln_w, ln_b, stats, in_act, Wt, dY, ld_dy, dX, ld_dx, dX_add, ld_dx_add, dW, dbias, dln_w, dln_b, workspace,
                       workspace_bytes, M, K, N, out_scale, dtype, split, (hipStream_t)stream, dX_add2, ld_dx_add2);
}

extern "C" int rdst_ln_linear_bwd(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, const float* stats,
                                  int in_act, const float* Wt, const void* dY, int64_t ld_dy, void* dX, int64_t ld_dx,
                                  const void* dX_add, int64_t ld_dx_add, float* dW, float* dbias, float* dln_w, float* dln_b,
                                  void* workspace, size_t workspace_bytes, int64_t M, int K, int N, float out_scale, int dtype,
                                  void* stream) {
  bool split;
  if (int rc = rdst_dtype(dtype, split, "rdst_ln_linear_bwd")) return rc;
  return ln_linear_bwd(X, ld_x, ln_w, ln_b, stats, in_act, Wt, dY, ld_dy, dX, ld_dx, dX_add, ld_dx_add, dW, dbias, dln_w, dln_b, workspace,
                       workspace_bytes, M, K, N, out_scale, dtype, split, (hipStream_t)stream, nullptr, 0);
}
