// Weight EMA inside the fused Adam launches, and the in-place exchange that puts the averaged weights under the network
// for evaluation.  Rules: include/rdst_hip.h.
//   adam_ema      : adam_kernel of adam.hip plus one more flat buffer: e = fmaf(p_new - e, omd, e) while p_new is in registers
//   adam_dev_ema  : adam_dev_kernel of step_guard.hip likewise; thread 0 of every block derives omd = 1 - d_t from state->kept
//   swap_f32      : exchanges two flat fp32 buffers; no address changes, so packed-weight plans and captured graphs stay valid
// The parameter and moment expressions are those of the two existing kernels, operation for operation: p, m and v carry the
// same bits whether the EMA is on or off (an edit to adam_kernel or adam_one there must be mirrored here; tests/test_ema_gpu.py
// compares the two with torch.equal).  Five fp32 streams read (p, g, m, v, ema: 20 B) and four written (p, m, v, ema: 16 B) per
// element, 36 B against the plain kernels' 28 B; 16-byte accesses, no atomics, no LDS traffic beyond the three broadcast
// scalars of adam_dev_ema.
#include "common.h"

namespace {

constexpr int kThreads = 256;

// d_t of the header: ema_decay, or with warmup min(ema_decay, (1 + t) / (10 + t)); 1 - d_t is rounded to fp32 ONCE
__host__ __device__ inline float one_minus_decay(double decay, int warmup, int64_t t) {
  double d = decay;
  if (warmup) {
    const double w = (1.0 + (double)t) / (10.0 + (double)t);
    if (w < d) d = w;
  }
  return (float)(1.0 - d);
}

__host__ inline int64_t stream_blocks(int64_t n) {
  int64_t blocks = ((n >> 2) + kThreads - 1) / kThreads;
  if (blocks > 256 * 8) blocks = 256 * 8;
  return blocks < 1 ? 1 : blocks;
}

__global__ void __launch_bounds__(kThreads) adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ ema, int64_t n, float lr_bc1, float beta1,
                                                            float beta2, float eps, float wd, float sqrt_bc2, float omd) {
  const int64_t n4 = n >> 2;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee = reinterpret_cast<float4*>(ema)[i];
    float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x; float* ea = &ee.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gr = wd != 0.f ? fmaf(wd, pa[e], ga[e]) : ga[e];
      ma[e] = fmaf(gr - ma[e], omb1, ma[e]);
      va[e] = fmaf(omb2 * gr, gr, va[e] * beta2);
      const float denom = sqrtf(va[e]) / sqrt_bc2 + eps;
      pa[e] = pa[e] - lr_bc1 * (ma[e] / denom);
      ea[e] = fmaf(pa[e] - ea[e], omd, ea[e]);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(ema)[i] = ee;
  }
  // tail (n % 4 elements)
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float gr = wd != 0.f ? fmaf(wd, p[t], g[t]) : g[t];
    const float mt = fmaf(gr - m[t], omb1, m[t]);
    const float vt = fmaf(omb2 * gr, gr, v[t] * beta2);
    m[t] = mt;
    v[t] = vt;
    const float pt = p[t] - lr_bc1 * (mt / (sqrtf(vt) / sqrt_bc2 + eps));
    p[t] = pt;
    ema[t] = fmaf(pt - ema[t], omd, ema[t]);
  }
}

// step_guard.hip's adam_one, operation for operation
__device__ __forceinline__ float adam_one(float& p, float g, float& m, float& v, float clip, float wd, float omb1,
                                          float omb2, float beta2, float eps, float lr_bc1, float sqrt_bc2) {
  const float gc = g * clip;      // clip == 1 leaves the bits of g as they are
  const float gr = wd != 0.f ? fmaf(wd, p, gc) : gc;
  m = fmaf(gr - m, omb1, m);
  v = fmaf(omb2 * gr, gr, v * beta2);
  const float denom = sqrtf(v) / sqrt_bc2 + eps;
  p = p - lr_bc1 * (m / denom);
  return p;
}

__global__ void __launch_bounds__(kThreads) adam_dev_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                float* __restrict__ m, float* __restrict__ v,
                                                                float* __restrict__ ema, int64_t n, rdst_lr_schedule sched,
                                                                float beta1, float beta2, float eps, float wd,
                                                                double ema_decay, int ema_warmup, rdst_step_state* st) {
  // written by the guard launch before this one; nothing in this launch writes these three fields
  const int64_t t = st->kept;
  if (st->last_keep == 0 || t < 1) return;     // a skipped step: param, both moments and the EMA stay bit for bit
  const float clip = st->last_clip;
  __shared__ float sh[3];
  if (threadIdx.x == 0) {     // every block derives the same three values from the same inputs
    int k = 0;
    for (int i = 0; i < sched.count; ++i) k += sched.milestones[i] <= t - 1;
    const float lr = sched.lr[k];
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    sh[0] = (float)((double)lr / bc1);
    sh[1] = (float)sqrt(bc2);
    sh[2] = one_minus_decay(ema_decay, ema_warmup, t);
    if (blockIdx.x == 0) st->last_lr = lr;
  }
  __syncthreads();
  const float lr_bc1 = sh[0], sqrt_bc2 = sh[1], omd = sh[2];
  const int64_t n4 = n >> 2;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2, b2 = beta2;   // as adam_kernel forms them: the same bits per element
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee = reinterpret_cast<float4*>(ema)[i];
    float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x; float* ea = &ee.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float pn = adam_one(pa[e], ga[e], ma[e], va[e], clip, wd, omb1, omb2, b2, eps, lr_bc1, sqrt_bc2);
      ea[e] = fmaf(pn - ea[e], omd, ea[e]);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(ema)[i] = ee;
  }
  // tail (n % 4 elements)
  const int64_t e = (n4 << 2) + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x == 0 && e < n) {
    float pt = p[e], mt = m[e], vt = v[e];
    adam_one(pt, g[e], mt, vt, clip, wd, omb1, omb2, b2, eps, lr_bc1, sqrt_bc2);
    m[e] = mt;
    v[e] = vt;
    p[e] = pt;
    ema[e] = fmaf(pt - ema[e], omd, ema[e]);
  }
}

__global__ void __launch_bounds__(kThreads) swap_f32_kernel(float* __restrict__ a, float* __restrict__ b, int64_t n) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
    const float4 x = reinterpret_cast<float4*>(a)[i];
    const float4 y = reinterpret_cast<float4*>(b)[i];
    reinterpret_cast<float4*>(a)[i] = y;
    reinterpret_cast<float4*>(b)[i] = x;
  }
  // tail (n % 4 elements)
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const float x = a[t], y = b[t];
    a[t] = y;
    b[t] = x;
  }
}

}  // namespace

extern "C" int rdst_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                  double ema_decay, int ema_warmup, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || n < 0 || step < 1)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_ema: null buffer, n < 0 or step < 1");
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_ema: buffers must be 16-byte aligned");
  if (!(ema_decay >= 0.0 && ema_decay < 1.0))     // a NaN decay is refused too
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_ema: ema_decay %g is not in [0, 1)", ema_decay);
  if (n == 0) return 0;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float lr_bc1 = (float)((double)lr / bc1), sqrt_bc2 = (float)sqrt(bc2);
  const float omd = one_minus_decay(ema_decay, ema_warmup, step);
  hipLaunchKernelGGL(adam_ema_kernel, dim3((unsigned)stream_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, ema, n, lr_bc1, beta1, beta2, eps, weight_decay, sqrt_bc2, omd);
  return rdst_launch_status("rdst_adam_step_ema");
}

extern "C" int rdst_adam_step_dev_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                      int64_t n, rdst_lr_schedule sched, float beta1, float beta2, float eps,
                                      float weight_decay, double ema_decay, int ema_warmup, rdst_step_state* state,
                                      void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !ema || !state || n < 0)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev_ema: null buffer or n < 0");
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema | (uintptr_t)state) & 15)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev_ema: buffers and state must be 16-byte aligned");
  if (!(ema_decay >= 0.0 && ema_decay < 1.0))
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev_ema: ema_decay %g is not in [0, 1)", ema_decay);
  if (sched.count < 0 || sched.count > 16)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev_ema: %d milestones (0..16)", sched.count);
  for (int i = 1; i < sched.count; ++i)
    if (sched.milestones[i] < sched.milestones[i - 1])
      return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev_ema: milestones must ascend");
  if (n == 0) return 0;
  hipLaunchKernelGGL(adam_dev_ema_kernel, dim3((unsigned)stream_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, param,
                     grad, exp_avg, exp_avg_sq, ema, n, sched, beta1, beta2, eps, weight_decay, ema_decay, ema_warmup, state);
  return rdst_launch_status("rdst_adam_step_dev_ema");
}

extern "C" int rdst_swap_f32(float* a, float* b, int64_t n, void* stream) {
  if (!a || !b || n < 0) return rdst_fail(RDST_EINVAL, "rdst_swap_f32: null buffer or n < 0");
  if (((uintptr_t)a | (uintptr_t)b) & 15) return rdst_fail(RDST_EINVAL, "rdst_swap_f32: buffers must be 16-byte aligned");
  if (n == 0) return 0;
  const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b;
  const uintptr_t hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
  if ((hi - lo) / sizeof(float) < (uint64_t)n)
    return rdst_fail(RDST_EINVAL, "rdst_swap_f32: the two ranges of %lld floats overlap", (long long)n);
  hipLaunchKernelGGL(swap_f32_kernel, dim3((unsigned)stream_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, a, b, n);
  return rdst_launch_status("rdst_swap_f32");
}
