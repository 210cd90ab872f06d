// Fused Adam over the flat parameter / gradient / moment buffers of the data-parallel training step
// (SURVEY.md §8f row N1).  Same update rule and operation order as torch.optim.Adam (amsgrad=False,
// maximize=False), which the reference builds in utils/optim.py:30-53 with the ini's hyper-parameters
// (betas 0.9/0.99, eps 1e-8, lr 1e-4, weight_decay 0):
//   g = grad + wd * p;  m = m + (g - m) * (1 - b1);  v = v * b2 + (1 - b2) * g * g
//   p = p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// One launch for all 4.46 M parameters (stock foreach Adam: ~15 multi-tensor launches plus ~1500
// scalar kernels per step in its capturable form).  Pure streaming: 16 B read + 12 B written per
// element, 16-byte vector accesses, grid-stride.
//
// The rule stands here ONCE (adam_one, adam_stream<CLIP, EMA>) under two thin kernels and four entry points:
//   adam_kernel<EMA>     : step count and rate are launch arguments        (rdst_adam_step, rdst_adam_step_ema)
//   adam_dev_kernel<EMA> : they are read from the rdst_step_state the guard of step_guard.hip wrote: thread 0 of every
//                          block derives (lr / bc1, sqrt(bc2), 1 - d_t) into LDS, the gradient is multiplied by last_clip as it
//                          is read and a skipped step returns at once, so the launch arguments never change and the step is
//                          graph-capturable                                (rdst_adam_step_dev, rdst_adam_step_dev_ema)
//   EMA                  : one more flat buffer, e = fmaf(p_new - e, omd, e) while p_new is in registers: 20 B read + 16 B
//                          written per element.  p, m and v carry the same bits whether the EMA is on or off.
//   swap_f32_kernel      : exchanges two flat fp32 buffers (the live and the averaged weights); no address changes, so
//                          packed-weight plans and captured graphs stay valid.
// Layout of the state and the rules of decay and schedule: include/rdst_hip.h.
#include "common.h"

namespace {

constexpr int kThreads = 256;

// what one launch holds fixed; clip is read only under CLIP and omd only under EMA
struct AdamCoef {
  float lr_bc1, sqrt_bc2, omd, clip, wd, omb1, omb2, beta2, eps;
};

// the hyper-parameters as every kernel forms them: the same bits per element
__device__ __forceinline__ AdamCoef adam_coef(float lr_bc1, float sqrt_bc2, float omd, float clip, float beta1, float beta2,
                                              float eps, float wd) {
  return {lr_bc1, sqrt_bc2, omd, clip, wd, 1.f - beta1, 1.f - beta2, beta2, eps};
}

// d_t of the header: ema_decay, or with warmup min(ema_decay, (1 + t) / (10 + t)); 1 - d_t is rounded to fp32 ONCE
__host__ __device__ inline float one_minus_decay(double decay, int warmup, int64_t t) {
  double d = decay;
  if (warmup) {
    const double w = (1.0 + (double)t) / (10.0 + (double)t);
    if (w < d) d = w;
  }
  return (float)(1.0 - d);
}

// grid of a streaming kernel over n floats, a float4 per thread and trip
__host__ inline int64_t stream_blocks(int64_t n) {
  int64_t blocks = ((n >> 2) + kThreads - 1) / kThreads;
  if (blocks > 256 * 8) blocks = 256 * 8;
  return blocks < 1 ? 1 : blocks;
}

template <bool CLIP>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamCoef& c) {
  const float gc = CLIP ? g * c.clip : g;      // clip == 1 leaves the bits of g as they are
  const float gr = c.wd != 0.f ? fmaf(c.wd, p, gc) : gc;
  m = fmaf(gr - m, c.omb1, m);
  v = fmaf(c.omb2 * gr, gr, v * c.beta2);
  const float denom = sqrtf(v) / c.sqrt_bc2 + c.eps;
  p = p - c.lr_bc1 * (m / denom);
}

template <bool CLIP, bool EMA>
__device__ __forceinline__ void adam_stream(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, float* __restrict__ ema, int64_t n, const AdamCoef c) {
  const int64_t n4 = n >> 2;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float4 ee;
    if constexpr (EMA) ee = reinterpret_cast<float4*>(ema)[i];
    float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x; float* ea = &ee.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      adam_one<CLIP>(pa[e], ga[e], ma[e], va[e], c);
      if constexpr (EMA) ea[e] = fmaf(pa[e] - ea[e], c.omd, ea[e]);
    }
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    if constexpr (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
  }
  // tail (n % 4 elements)
  const int64_t t = (n4 << 2) + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    float pt = p[t], mt = m[t], vt = v[t];
    adam_one<CLIP>(pt, g[t], mt, vt, c);
    m[t] = mt;
    v[t] = vt;
    p[t] = pt;
    if constexpr (EMA) ema[t] = fmaf(pt - ema[t], c.omd, ema[t]);
  }
}

// host count: the coefficients are launch arguments (ema and omd are not read without EMA)
template <bool EMA>
__global__ void __launch_bounds__(kThreads) adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, int64_t n, float lr_bc1, float beta1,
                                                        float beta2, float eps, float wd, float sqrt_bc2, float omd) {
  adam_stream<false, EMA>(p, g, m, v, ema, n, adam_coef(lr_bc1, sqrt_bc2, omd, 1.f, beta1, beta2, eps, wd));
}

// device count (ema, ema_decay and ema_warmup are not read without EMA)
template <bool EMA>
__global__ void __launch_bounds__(kThreads) adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v,
                                                            float* __restrict__ ema, int64_t n, rdst_lr_schedule sched,
                                                            float beta1, float beta2, float eps, float wd, double ema_decay,
                                                            int ema_warmup, rdst_step_state* st) {
  // written by the guard launch before this one; nothing in this launch writes these three fields
  const int64_t t = st->kept;
  if (st->last_keep == 0 || t < 1) return;     // a skipped step: param, both moments and the EMA stay bit for bit
  const float clip = st->last_clip;
  __shared__ float sh[EMA ? 3 : 2];
  if (threadIdx.x == 0) {     // every block derives the same values from the same inputs
    int k = 0;
    for (int i = 0; i < sched.count; ++i) k += sched.milestones[i] <= t - 1;
    const float lr = sched.lr[k];
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    sh[0] = (float)((double)lr / bc1);
    sh[1] = (float)sqrt(bc2);
    if constexpr (EMA) sh[2] = one_minus_decay(ema_decay, ema_warmup, t);
    if (blockIdx.x == 0) st->last_lr = lr;
  }
  __syncthreads();
  float omd = 0.f;
  if constexpr (EMA) omd = sh[2];
  adam_stream<true, EMA>(p, g, m, v, ema, n, adam_coef(sh[0], sh[1], omd, clip, beta1, beta2, eps, wd));
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

// The refusals of the five entry points, in one order: a null buffer (`bufs` ends with the state where there is one) or a bad
// count, alignment, the decay, the schedule.  `step`, `decay` and `sched` are null where the entry point has none; `sched`
// marks the device-count pair.
int check_args(const char* who, std::initializer_list<const void*> bufs, int64_t n, const int64_t* step, const double* decay,
               const rdst_lr_schedule* sched) {
  uintptr_t bits = 0;
  bool null = false;
  for (const void* b : bufs) {
    null |= !b;
    bits |= (uintptr_t)b;
  }
  if (null || n < 0 || (step && *step < 1))
    return rdst_fail(RDST_EINVAL, step ? "%s: null buffer, n < 0 or step < 1" : "%s: null buffer or n < 0", who);
  if (bits & 15)
    return rdst_fail(RDST_EINVAL, sched ? "%s: buffers and state must be 16-byte aligned" : "%s: buffers must be 16-byte aligned",
                     who);
  if (decay && !(*decay >= 0.0 && *decay < 1.0))     // a NaN decay is refused too
    return rdst_fail(RDST_EINVAL, "%s: ema_decay %g is not in [0, 1)", who, *decay);
  if (sched) {
    if (sched->count < 0 || sched->count > 16) return rdst_fail(RDST_EINVAL, "%s: %d milestones (0..16)", who, sched->count);
    for (int i = 1; i < sched->count; ++i)
      if (sched->milestones[i] < sched->milestones[i - 1]) return rdst_fail(RDST_EINVAL, "%s: milestones must ascend", who);
  }
  return 0;
}

template <bool EMA>
int adam_step(const char* who, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
              float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, double ema_decay,
              int ema_warmup, void* stream) {
  const int rc = EMA ? check_args(who, {param, grad, exp_avg, exp_avg_sq, ema}, n, &step, &ema_decay, nullptr)
                     : check_args(who, {param, grad, exp_avg, exp_avg_sq}, n, &step, nullptr, nullptr);
  if (rc || n == 0) return rc;
  const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
  const float lr_bc1 = (float)((double)lr / bc1), sqrt_bc2 = (float)sqrt(bc2);
  const float omd = EMA ? one_minus_decay(ema_decay, ema_warmup, step) : 0.f;
  hipLaunchKernelGGL(adam_kernel<EMA>, dim3((unsigned)stream_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, param, grad,
                     exp_avg, exp_avg_sq, ema, n, lr_bc1, beta1, beta2, eps, weight_decay, sqrt_bc2, omd);
  return rdst_launch_status(who);
}

template <bool EMA>
int adam_step_dev(const char* who, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                  const rdst_lr_schedule& sched, float beta1, float beta2, float eps, float weight_decay, double ema_decay,
                  int ema_warmup, rdst_step_state* state, void* stream) {
  const int rc = EMA ? check_args(who, {param, grad, exp_avg, exp_avg_sq, ema, state}, n, nullptr, &ema_decay, &sched)
                     : check_args(who, {param, grad, exp_avg, exp_avg_sq, state}, n, nullptr, nullptr, &sched);
  if (rc || n == 0) return rc;
  hipLaunchKernelGGL(adam_dev_kernel<EMA>, dim3((unsigned)stream_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, param,
                     grad, exp_avg, exp_avg_sq, ema, n, sched, beta1, beta2, eps, weight_decay, ema_decay, ema_warmup, state);
  return rdst_launch_status(who);
}

}  // namespace

extern "C" int rdst_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  return adam_step<false>("rdst_adam_step", param, grad, exp_avg, exp_avg_sq, nullptr, n, lr, beta1, beta2, eps, weight_decay,
                          step, 0.0, 0, stream);
}

extern "C" int rdst_adam_step_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                  double ema_decay, int ema_warmup, void* stream) {
  return adam_step<true>("rdst_adam_step_ema", param, grad, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, weight_decay,
                         step, ema_decay, ema_warmup, stream);
}

extern "C" int rdst_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  rdst_lr_schedule sched, float beta1, float beta2, float eps, float weight_decay,
                                  rdst_step_state* state, void* stream) {
  return adam_step_dev<false>("rdst_adam_step_dev", param, grad, exp_avg, exp_avg_sq, nullptr, n, sched, beta1, beta2, eps,
                              weight_decay, 0.0, 0, state, stream);
}

extern "C" int rdst_adam_step_dev_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                      int64_t n, rdst_lr_schedule sched, float beta1, float beta2, float eps,
                                      float weight_decay, double ema_decay, int ema_warmup, rdst_step_state* state,
                                      void* stream) {
  return adam_step_dev<true>("rdst_adam_step_dev_ema", param, grad, exp_avg, exp_avg_sq, ema, n, sched, beta1, beta2, eps,
                             weight_decay, ema_decay, ema_warmup, state, stream);
}

extern "C" int rdst_swap_f32(float* a, float* b, int64_t n, void* stream) {
  const int rc = check_args("rdst_swap_f32", {a, b}, n, nullptr, nullptr, nullptr);
  if (rc || n == 0) return rc;
  const uintptr_t lo = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)a : (uintptr_t)b;
  const uintptr_t hi = (uintptr_t)a < (uintptr_t)b ? (uintptr_t)b : (uintptr_t)a;
  if ((hi - lo) / sizeof(float) < (uint64_t)n)
    return rdst_fail(RDST_EINVAL, "rdst_swap_f32: the two ranges of %lld floats overlap", (long long)n);
  hipLaunchKernelGGL(swap_f32_kernel, dim3((unsigned)stream_blocks(n)), dim3(kThreads), 0, (hipStream_t)stream, a, b, n);
  return rdst_launch_status("rdst_swap_f32");
}
