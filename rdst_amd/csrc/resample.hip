// K-tap degradations of the device data path (rdst_amd/data.py, include/rdst_hip_data.h): any separable linear operator
// LR = A_y . patch . A_x^T given as a table of K taps per output (rdst_amd.data.operator_table: plain and antialiased
// bicubic, bicubic followed by cv2's Gaussian blur, Fourier-domain truncation, ...), applied to whole images
// (rdst_resample_sep) and inside the sampler's one launch (rdst_sample_patches_op).  sampler.hip has the 4-tap kernels; the
// argument checks and the LDS fit both files make are tap_host.h's.
// rdst_sample_patches_noise (include/rdst_hip_noise.h) is that launch with the noise term applied in its final store: the
// same kernel under a compile-time switch, whose off instantiation is the kernel as it was.
//
// Every output is formed by tapk() (tapk.h), the generalisation of sampler.hip's tap4(): acc = w[0] * v[0] rounded, then one
// explicit fmaf per tap in ascending order; the horizontal sums of the tap rows first, then the vertical chain over them.
// A horizontal sum depends on its source row, its output column and the table only, so forming it once and sharing it
// among the output rows gives the bits of forming it per output pixel: a K = 4 table gives the bits of tap4(), and the
// sampler's LR patch equals rdst_resample_sep of its HR patch.  A padding tap (weight 0) leaves the sum as it is.
//
// No MFMA, no atomics, no scratch.  Tables are read as int4 / float4 (K % 4 == 0, 16-byte aligned), pixels as dwords with
// lanes along a source row; every index read from device memory is clamped before it becomes an address.
#include "tap_host.h"
#include "tapk.h"
#include "noise.h"
#include "../../include/rdst_hip_data.h"

namespace {

// ---- rdst_resample_sep: the horizontal sums of every source row, then the vertical chains; one thread per value -------
__global__ void __launch_bounds__(NT) hsum_kernel(const float* __restrict__ x, float* __restrict__ tmp, int W, int ow, int Kx4,
                                                  const int4* __restrict__ ix, const f4* __restrict__ wx, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % ow);
  const float* p = x + (i / ow) * W;   // the source row: (plane * H + r) * W
  tmp[i] = tapk(ix + (int64_t)ox * Kx4, wx + (int64_t)ox * Kx4, Kx4, [&](int j) { return p[clampi(j, 0, W - 1)]; });
}

__global__ void __launch_bounds__(NT) vsum_kernel(const float* __restrict__ tmp, float* __restrict__ y, int H, int oh, int ow,
                                                  int Ky4, const int4* __restrict__ iy, const f4* __restrict__ wy,
                                                  int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % ow);
  const int64_t t = i / ow;
  const int oy = (int)(t % oh);
  const float* p = tmp + (t / oh) * H * ow + ox;
  y[i] = tapk(iy + (int64_t)oy * Ky4, wy + (int64_t)oy * Ky4, Ky4, [&](int j) { return p[(int64_t)clampi(j, 0, H - 1) * ow]; });
}

// ---- rdst_sample_patches_op: one workgroup per (patch, channel, band of BC columns of the LR patch) -------------------
// T_k(x)[i][j] = x[a][b] with (a, b) = (j, i) if k & 4 else (i, j), then a = hp - 1 - a if k & 2, b = hp - 1 - b if k & 1.
// The workgroup walks the rows of the TURNED patch in chunks of RC: it stages the columns its taps read, [x_lo, x_hi), into
// raw[RC][pitch] (lanes along the source rows: along a turned row, or down a turned column for the transposed variants; pitch
// is odd, so neither walk meets a bank twice), forms the horizontal sums of those rows for its BC columns into hs[hp][BC + 1]
// and, after the last chunk, the vertical chains of its LR columns from hs.  Chunk number ch belongs to band ch % nb: that
// band stages the whole rows, writes them to the HR output from LDS with lanes along them, and moves the label bytes.
// NOISE: every LR value goes through noise_apply() (noise.h) on its way out, keyed by its own place in the LR array (plane =
// b * C + c, row, column) and under the levels of patch b; nothing else changes, and `nz` is not read without it.
template <bool NOISE>
__global__ void __launch_bounds__(NT) sample_op_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ labels,
                                                       const int* __restrict__ index, const int* __restrict__ variant,
                                                       float* __restrict__ hr, float* __restrict__ lr, uint8_t* __restrict__ lab,
                                                       int S, int C, int H, int W, int hp, int lp, int K4,
                                                       const int4* __restrict__ it, const f4* __restrict__ wt, int BC, int nb,
                                                       int RC, int pitch, NoiseArgs nz) {
  extern __shared__ __attribute__((aligned(16))) float lds[];   // hs [hp][BC + 1], then raw [RC][pitch]
  const int hsp = BC + 1;
  float* hs = lds;
  float* raw = lds + hp * hsp;
  const int band = (int)(blockIdx.x % (unsigned)nb);
  const int plane = (int)(blockIdx.x / (unsigned)nb);
  const int c = plane % C, b = plane / C;
  const int c0 = band * BC, bcn = min(BC, lp - c0);
  // the window and the turn: device memory nobody checked
  const int64_t slice = clampi(index[3 * b], 0, S - 1);
  const int top = clampi(index[3 * b + 1], 0, H - hp), left = clampi(index[3 * b + 2], 0, W - hp);
  const int k = variant != nullptr ? variant[b] & 7 : 0;
  const bool tr = k & 4, fa = k & 2, fb = k & 1;
  int x_lo = hp - 1, x_hi = 0;   // taps ascend: a row's first is its lowest, its last its highest
  for (int o = c0; o < c0 + bcn; ++o) {
    x_lo = min(x_lo, clampi(it[(int64_t)o * K4].x, 0, hp - 1));
    x_hi = max(x_hi, clampi(it[(int64_t)o * K4 + K4 - 1].w, 0, hp - 1));
  }
  const int nx = max(x_hi + 1 - x_lo, 1);
  const float* src = stack + ((slice * C + c) * H + top) * W + left;
  float* dst = hr + ((int64_t)b * C + c) * hp * hp;
  const uint8_t* ls = labels != nullptr && c == 0 ? labels + (slice * H + top) * W + left : nullptr;
  uint8_t* ld = lab + (int64_t)b * hp * hp;
  for (int r0 = 0, ch = 0; r0 < hp; r0 += RC, ++ch) {
    const int rcn = min(RC, hp - r0);
    const bool own = ch % nb == band;
    const int col0 = own ? 0 : x_lo, ncols = own ? hp : nx;
    // element e of the chunk: its place in raw (r, jj) and in the slice; SG loads of a thread are in flight together
    auto place = [&](int e, int& r, int& jj) -> int64_t {
      if (!tr) r = e / ncols, jj = e - r * ncols;
      else jj = e / rcn, r = e - jj * rcn;
      const int i = r0 + r, j = col0 + jj;
      int a = tr ? j : i, bb = tr ? i : j;
      if (fa) a = hp - 1 - a;
      if (fb) bb = hp - 1 - bb;
      return (int64_t)a * W + bb;
    };
    const int n = rcn * ncols;
    for (int e0 = threadIdx.x; e0 < n; e0 += SG * NT) {
      float v[SG];
      int to[SG];
#pragma unroll
      for (int u = 0; u < SG; ++u) {
        const int e = e0 + u * NT;
        int r = 0, jj = 0;
        if (e < n) v[u] = src[place(e, r, jj)];
        to[u] = r * pitch + jj;
      }
#pragma unroll
      for (int u = 0; u < SG; ++u)
        if (e0 + u * NT < n) raw[to[u]] = v[u];
    }
    if (own && ls != nullptr)
      for (int e = threadIdx.x; e < n; e += NT) {
        int r, jj;
        const int64_t at = place(e, r, jj);
        ld[(int64_t)(r0 + r) * hp + col0 + jj] = ls[at];
      }
    __syncthreads();
    if (own)
      for (int e = threadIdx.x; e < rcn * hp; e += NT) {
        const int r = e / hp, j = e - r * hp;
        dst[(int64_t)(r0 + r) * hp + j] = raw[r * pitch + j];
      }
    for (int e = threadIdx.x; e < rcn * bcn; e += NT) {
      const int r = e / bcn, oxl = e - r * bcn;
      const float* row = raw + r * pitch;
      const int64_t t = (int64_t)(c0 + oxl) * K4;
      hs[(r0 + r) * hsp + oxl] = tapk(it + t, wt + t, K4, [&](int j) { return row[clampi(clampi(j, 0, hp - 1) - col0, 0, ncols - 1)]; });
    }
    __syncthreads();   // hs of the chunk is whole; the next chunk overwrites raw
  }
  float* out = lr + ((int64_t)b * C + c) * lp * lp + c0;
  unsigned long long seed = 0ull;
  float p0 = 0.f, p1 = 0.f;
  if constexpr (NOISE) seed = *nz.seed, p0 = nz.levels[2 * b], p1 = nz.levels[2 * b + 1];
  for (int e = threadIdx.x; e < lp * bcn; e += NT) {
    const int oy = e / bcn, oxl = e - oy * bcn;
    const int64_t t = (int64_t)oy * K4;
    float v = tapk(it + t, wt + t, K4, [&](int j) { return hs[clampi(j, 0, hp - 1) * hsp + oxl]; });
    if constexpr (NOISE)
      v = noise_apply(v, seed, (uint32_t)plane, (uint32_t)oy, (uint32_t)(c0 + oxl), nz.model, p0, p1, nz.clip_lo, nz.clip_hi);
    out[(int64_t)oy * lp + oxl] = v;
  }
}

}  // namespace

extern "C" int rdst_resample_sep(const float* x, float* y, float* tmp, int N, int C, int H, int W, int oh, int ow, int Ky,
                                 const int32_t* index_y, const float* weight_y, int Kx, const int32_t* index_x,
                                 const float* weight_x, void* stream) {
  const char* who = "rdst_resample_sep";
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d -> %d x %d", who, N, C, H, W, oh, ow);
  if (!x || !y || !tmp) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if (int rc = table_refusal(who, " y", Ky, index_y, weight_y)) return rc;
  if (int rc = table_refusal(who, " x", Kx, index_x, weight_x)) return rc;
  const int64_t htotal = (int64_t)N * C * H * ow, vtotal = (int64_t)N * C * oh * ow;
  const int64_t hblocks = (htotal + NT - 1) / NT, vblocks = (vtotal + NT - 1) / NT;
  if (hblocks > 0x7fffffff || vblocks > 0x7fffffff)
    return rdst_fail(RDST_EINVAL, "%s: %lld values are too many for one launch", who, (long long)max(htotal, vtotal));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(hsum_kernel, dim3((unsigned)hblocks), dim3(NT), 0, st, x, tmp, W, ow, Kx / 4, (const int4*)index_x,
                     (const f4*)weight_x, htotal);
  if (int rc = rdst_launch_status(who)) return rc;
  hipLaunchKernelGGL(vsum_kernel, dim3((unsigned)vblocks), dim3(NT), 0, st, (const float*)tmp, y, H, oh, ow, Ky / 4,
                     (const int4*)index_y, (const f4*)weight_y, vtotal);
  return rdst_launch_status(who);
}

namespace {

// rdst_sample_patches_op (nz == nullptr) and rdst_sample_patches_noise: one set of refusals, one plan, one launch
int sample_op(const char* who, const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant, float* hr,
              float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp, int K, const int32_t* tap_index,
              const float* tap_weight, const NoiseArgs* nz, void* stream) {
  if (int rc = sample_refusal(who, stack, labels, index, hr, lr, label_out, S, C, H, W, B, hp, lp)) return rc;
  if (int rc = table_refusal(who, "", K, tap_index, tap_weight)) return rc;
  if (nz != nullptr)
    if (int rc = noise_refusal(who, nz->model, nz->levels, nz->seed, nz->clip_lo, nz->clip_hi)) return rc;
  const int pitch = hp | 1;   // hs [hp][BC + 1] and raw [RC][pitch]
  int BC = min(BC_MAX, lp), RC = min(RC_MAX, hp);
  int64_t bytes;
  if (!fit_lds(hp, BC, RC, pitch, LDS_BUDGET, bytes))
    return rdst_fail(RDST_ENOTSUP, "%s: hp=%d is wider than the LDS holds (one column of sums and one row need %lld bytes)", who,
                     hp, (long long)bytes);
  const int nb = (lp + BC - 1) / BC;
  const int64_t blocks = (int64_t)B * C * nb;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: B=%d C=%d lp=%d is too large for one launch", who, B, C, lp);
  auto launch = [&](auto kern, const NoiseArgs& a) {
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(NT), (size_t)bytes, (hipStream_t)stream, stack, labels, index, variant,
                       hr, lr, label_out, S, C, H, W, hp, lp, K / 4, (const int4*)tap_index, (const f4*)tap_weight, BC, nb, RC,
                       pitch, a);
  };
  if (nz != nullptr) launch(sample_op_kernel<true>, *nz);
  else launch(sample_op_kernel<false>, NoiseArgs{});
  return rdst_launch_status(who);
}

}  // namespace

extern "C" int rdst_sample_patches_op(const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant,
                                      float* hr, float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp,
                                      int K, const int32_t* tap_index, const float* tap_weight, void* stream) {
  return sample_op("rdst_sample_patches_op", stack, labels, index, variant, hr, lr, label_out, S, C, H, W, B, hp, lp, K, tap_index,
                   tap_weight, nullptr, stream);
}

extern "C" int rdst_sample_patches_noise(const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant,
                                         float* hr, float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp,
                                         int lp, int K, const int32_t* tap_index, const float* tap_weight, int model,
                                         const float* levels, const unsigned long long* seed, float clip_lo, float clip_hi,
                                         void* stream) {
  const NoiseArgs nz = {model, levels, seed, clip_lo, clip_hi};
  return sample_op("rdst_sample_patches_noise", stack, labels, index, variant, hr, lr, label_out, S, C, H, W, B, hp, lp, K,
                   tap_index, tap_weight, &nz, stream);
}
