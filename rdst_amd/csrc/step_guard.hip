// Device-side step guard: the `if loss.item() < self.loss_threshold:` of the reference's inner loop
// (models/trans_sr_trainer.py:162-174) decided in device memory, plus a non-finite-gradient skip and global-norm clipping
// from one fp64 sum-of-squares pass over the flat gradient bucket, and the fused Adam of adam.hip driven by that decision:
// step count, learning-rate schedule and clip coefficient are read from the step state, so the launch arguments never
// change and the whole step is graph-capturable.  Layout and rules: include/rdst_hip.h.
//   sumsq_partial : grid-stride float4 loads, fp64 accumulation per thread, fixed-order LDS tree, one partial per block
//   decide        : one block sums the partials in a fixed order; thread 0 writes the state
//   adam_dev      : adam_kernel's streaming loop; thread 0 of every block derives (lr / bc1, sqrt(bc2)) from the state
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPartials = 1024;

__host__ __device__ inline int64_t sumsq_blocks(int64_t n) {
  int64_t b = ((n >> 2) + kThreads - 1) / kThreads;
  return b < 1 ? 1 : (b > kMaxPartials ? kMaxPartials : b);
}

// fixed-order tree over the block's 256 accumulators: the same bits on every run
__device__ __forceinline__ double block_sum(double acc, double* s) {
  s[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  return s[0];
}

__global__ void __launch_bounds__(kThreads) sumsq_partial_kernel(const float* __restrict__ g, int64_t n,
                                                                 double* __restrict__ partial) {
  __shared__ double s[kThreads];
  const int64_t n4 = n >> 2;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
    const float4 v = reinterpret_cast<const float4*>(g)[i];
    const double a = v.x, b = v.y, c = v.z, d = v.w;
    acc = fma(a, a, acc);
    acc = fma(b, b, acc);
    acc = fma(c, c, acc);
    acc = fma(d, d, acc);
  }
  // tail (n % 4 elements)
  const int64_t t = (n4 << 2) + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const double a = g[t];
    acc = fma(a, a, acc);
  }
  const double tot = block_sum(acc, s);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(kThreads) decide_kernel(const float* __restrict__ loss, double threshold,
                                                          const int32_t* __restrict__ peer_skip,
                                                          const double* __restrict__ partial, int nparts,
                                                          double max_grad_norm, int check_finite, rdst_step_state* st) {
  __shared__ double s[kThreads];
  double sumsq = -1.0;
  if (nparts > 0) {   // uniform over the block
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += kThreads) acc += partial[i];
    sumsq = block_sum(acc, s);
  }
  if (threadIdx.x != 0) return;
  int reason = 0;
  if (loss && !((double)loss[0] < threshold)) reason |= RDST_SKIP_LOSS;     // a NaN loss is "not below"
  if (nparts > 0 && check_finite && !isfinite(sumsq)) reason |= RDST_SKIP_NONFINITE;
  if (peer_skip && peer_skip[0] != 0) reason |= RDST_SKIP_PEER;
  float clip = 1.f;
  if (nparts > 0 && max_grad_norm > 0.0) {   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1)
    double c = max_grad_norm / (sqrt(sumsq) + 1e-6);
    if (c > 1.0) c = 1.0;
    clip = (float)c;
  }
  const int keep = reason == 0;
  st->kept += keep;
  st->skipped += !keep;
  st->last_keep = keep;
  st->last_reason = reason;
  st->last_clip = clip;
  st->last_sumsq = sumsq;
}

// (ema.hip restates adam_one and adam_dev_kernel's loop with the EMA stream added: mirror an edit there)
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

__global__ void __launch_bounds__(kThreads) adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                            rdst_lr_schedule sched, float beta1, float beta2, float eps,
                                                            float wd, rdst_step_state* st) {
  // written by the guard launch before this one; nothing in this launch writes these three fields
  const int64_t t = st->kept;
  if (st->last_keep == 0 || t < 1) return;     // a skipped step: param and both moments stay bit for bit
  const float clip = st->last_clip;
  __shared__ float sh[2];
  if (threadIdx.x == 0) {     // every block derives the same two values from the same inputs
    int k = 0;
    for (int i = 0; i < sched.count; ++i) k += sched.milestones[i] <= t - 1;
    const float lr = sched.lr[k];
    const double bc1 = 1.0 - pow((double)beta1, (double)t), bc2 = 1.0 - pow((double)beta2, (double)t);
    sh[0] = (float)((double)lr / bc1);
    sh[1] = (float)sqrt(bc2);
    if (blockIdx.x == 0) st->last_lr = lr;
  }
  __syncthreads();
  const float lr_bc1 = sh[0], sqrt_bc2 = sh[1];
  const int64_t n4 = n >> 2;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2, b2 = beta2;   // as adam_kernel forms them: the same bits per element
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kThreads) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 mm = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
    for (int e = 0; e < 4; ++e) adam_one(pa[e], ga[e], ma[e], va[e], clip, wd, omb1, omb2, b2, eps, lr_bc1, sqrt_bc2);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
  // tail (n % 4 elements)
  const int64_t e = (n4 << 2) + (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (blockIdx.x == 0 && e < n) {
    float pt = p[e], mt = m[e], vt = v[e];
    adam_one(pt, g[e], mt, vt, clip, wd, omb1, omb2, b2, eps, lr_bc1, sqrt_bc2);
    m[e] = mt;
    v[e] = vt;
    p[e] = pt;
  }
}

}  // namespace

extern "C" size_t rdst_step_guard_workspace(int64_t n) { return n > 0 ? (size_t)sumsq_blocks(n) * sizeof(double) : 0; }

extern "C" int rdst_step_guard(const float* loss, double threshold, const int32_t* peer_skip, const float* grad, int64_t n,
                               double max_grad_norm, int check_finite, void* workspace, size_t workspace_bytes,
                               rdst_step_state* state, void* stream) {
  if (!state || ((uintptr_t)state & 15)) return rdst_fail(RDST_EINVAL, "rdst_step_guard: state is null or not 16-byte aligned");
  if (n < 0) return rdst_fail(RDST_EINVAL, "rdst_step_guard: n < 0");
  int nparts = 0;
  if ((max_grad_norm > 0.0 || check_finite) && n > 0) {
    if (!grad || ((uintptr_t)grad & 15)) return rdst_fail(RDST_EINVAL, "rdst_step_guard: grad is null or not 16-byte aligned");
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < rdst_step_guard_workspace(n))
      return rdst_fail(RDST_EINVAL, "rdst_step_guard: workspace is null, misaligned or smaller than %zu bytes",
                       rdst_step_guard_workspace(n));
    nparts = (int)sumsq_blocks(n);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3((unsigned)nparts), dim3(kThreads), 0, (hipStream_t)stream, grad, n,
                       (double*)workspace);
  }
  hipLaunchKernelGGL(decide_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, loss, threshold, peer_skip,
                     (const double*)workspace, nparts, max_grad_norm, check_finite, state);
  return rdst_launch_status("rdst_step_guard");
}

extern "C" int rdst_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                                  rdst_lr_schedule sched, float beta1, float beta2, float eps, float weight_decay,
                                  rdst_step_state* state, void* stream) {
  if (!param || !grad || !exp_avg || !exp_avg_sq || !state || n < 0)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev: null buffer or n < 0");
  if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)state) & 15)
    return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev: buffers and state must be 16-byte aligned");
  if (sched.count < 0 || sched.count > 16) return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev: %d milestones (0..16)", sched.count);
  for (int i = 1; i < sched.count; ++i)
    if (sched.milestones[i] < sched.milestones[i - 1]) return rdst_fail(RDST_EINVAL, "rdst_adam_step_dev: milestones must ascend");
  if (n == 0) return 0;
  int64_t blocks = ((n >> 2) + kThreads - 1) / kThreads;
  if (blocks > 256 * 8) blocks = 256 * 8;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(adam_dev_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, param, grad, exp_avg,
                     exp_avg_sq, n, sched, beta1, beta2, eps, weight_decay, state);
  return rdst_launch_status("rdst_adam_step_dev");
}
