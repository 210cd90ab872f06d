// The whole-image entry points of the noise term (include/rdst_hip_noise.h): rdst_noise_words, the generator's words as they
// are, and rdst_add_noise, LR = A(HR) + n on images that are already degraded.  One thread per pixel, one Philox call per
// pixel keyed by its own (plane, y, x): nothing is shared among threads, so the workgroup shape does not enter the result and
// rdst_sample_patches_noise (resample.hip), which calls the same noise_apply() in its final store, gives the same bits.
// No MFMA, no LDS, no atomics, no scratch; every store is a vector store.
#include "common.h"
#include "noise.h"

namespace {

constexpr int NT = 256;

__global__ void __launch_bounds__(NT) noise_words_kernel(int4* __restrict__ out, int H, int W,
                                                         const unsigned long long* __restrict__ seedp, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i / W;
  const PhiloxWords w = philox_pixel(*seedp, (uint32_t)(t / H), (uint32_t)(t % H), (uint32_t)(i % W));
  out[i] = make_int4((int)w.w0, (int)w.w1, (int)w.w2, (int)w.w3);
}

// x and y may be one array: a thread reads its own value and nothing else before it writes it
__global__ void __launch_bounds__(NT) add_noise_kernel(const float* x, float* y, int C, int H, int W, NoiseArgs nz, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int64_t t = i / W;
  const int64_t plane = t / H;
  const float* lv = nz.levels + 2 * (plane / C);
  y[i] = noise_apply(x[i], *nz.seed, (uint32_t)plane, (uint32_t)(t % H), (uint32_t)(i % W), nz.model, lv[0], lv[1], nz.clip_lo,
                     nz.clip_hi);
}

// rows * W values, one thread each: the total and the grid, or the refusal (rows is at most 2^62, so nothing here overflows)
int one_launch(const char* who, int64_t rows, int W, int64_t* total, int64_t* blocks) {
  if (rows > (int64_t)0x7fffffff * NT / W)
    return rdst_fail(RDST_EINVAL, "%s: %lld rows of %d values are too many for one launch", who, (long long)rows, W);
  *total = rows * W;
  *blocks = (*total + NT - 1) / NT;
  return 0;
}

}  // namespace

extern "C" int rdst_noise_words(int32_t* out, int planes, int H, int W, const unsigned long long* seed, void* stream) {
  const char* who = "rdst_noise_words";
  if (planes <= 0 || H <= 0 || W <= 0) return rdst_fail(RDST_EINVAL, "%s: bad shape planes=%d H=%d W=%d", who, planes, H, W);
  if (!out) return rdst_fail(RDST_EINVAL, "%s: null out", who);
  if ((uintptr_t)out & 15) return rdst_fail(RDST_EINVAL, "%s: out must be 16-byte aligned", who);
  if (!seed) return rdst_fail(RDST_EINVAL, "%s: null seed", who);
  int64_t total, blocks;
  if (int rc = one_launch(who, (int64_t)planes * H, W, &total, &blocks)) return rc;
  hipLaunchKernelGGL(noise_words_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, (int4*)out, H, W, seed, total);
  return rdst_launch_status(who);
}

extern "C" int rdst_add_noise(const float* x, float* y, int N, int C, int H, int W, int model, const float* levels,
                              const unsigned long long* seed, float clip_lo, float clip_hi, void* stream) {
  const char* who = "rdst_add_noise";
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
  if (!x || !y) return rdst_fail(RDST_EINVAL, "%s: null %s", who, !x ? "x" : "y");
  if (int rc = noise_refusal(who, model, levels, seed, clip_lo, clip_hi)) return rc;
  if ((int64_t)N * C > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d is too many planes for one launch", who, N, C);
  int64_t total, blocks;
  if (int rc = one_launch(who, (int64_t)N * C * H, W, &total, &blocks)) return rc;
  const NoiseArgs nz = {model, levels, seed, clip_lo, clip_hi};
  hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, y, C, H, W, nz, total);
  return rdst_launch_status(who);
}
