// Device-side step guard: the `if loss.item() < self.loss_threshold:` of the reference's inner loop
// (models/trans_sr_trainer.py:162-174) decided in device memory, plus a non-finite-gradient skip and global-norm clipping
// from one fp64 sum-of-squares pass over the flat gradient bucket.  The decision lands in the rdst_step_state that the
// device-count Adam of adam.hip (adam_dev_kernel) reads: step count, learning-rate schedule and clip coefficient come from
// the state, so the launch arguments never change and the whole step is graph-capturable.  Layout and rules: include/rdst_hip.h.
//   sumsq_partial : grid-stride float4 loads, fp64 accumulation per thread, fixed-order LDS tree, one partial per block
//   decide        : one block sums the partials in a fixed order; thread 0 writes the state
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
