// The SSIM training loss: loss = 1 - mean_n ssim[n] and d loss / d pred in ONE tile kernel plus a small finish kernel; the
// definition is the comment on rdst_ssim_loss in include/rdst_hip.h.  Window arithmetic is fp64 as in srmetrics.hip
// (products of two fp32 values are exact there), sums run in a fixed order, nothing is atomic: results are bit-identical
// run to run.
//
// The tile, its LDS carve and the phases 1 - 6 are ssim_tile.h's (shared with msssim_loss.hip).  What is this kernel's own:
//   4  beside a, b, c: S of the positions the tile owns (position (i,j) belongs to the tile holding pixel (i,j))   sown [TR][TC]
//   6  one rounding to fp32 per gradient element, one 16-byte store where aligned
// and the sum of sown in an order that does not depend on whether the gradient was asked for: the value-only
// instantiation (HL = 0, abc and phases 5-6 dropped) returns the same bits.
#include "ssim_tile.h"
#include <math.h>

namespace {

using namespace ssim_tile;

// one workgroup per (plane = image * C + channel, tile row, tile column); part[block] = sum of S over the owned positions
template <int WIN, bool GRAD>
__global__ void __launch_bounds__(NT) ssl_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                                      int tiles_y, int tiles_x, SsimTaps taps, double cn, double C1, double C2,
                                                      double inv_cnt, double* __restrict__ part, float* __restrict__ grad) {
  using G = Geo<WIN, GRAD>;
  constexpr int HL = G::HL, PR = G::PR, PC = G::PC, SC = G::SC;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* red = smem;
  double* hs = red + G::RED_D;
  float* xs = reinterpret_cast<float*>(hs + G::HS_D);
  float* ys = xs + G::XS_F;
  const int tid = threadIdx.x;
  const int Ho = H - WIN + 1, Wo = W - WIN + 1;
  unsigned b = blockIdx.x;
  const int tx = (int)(b % (unsigned)tiles_x);
  b /= (unsigned)tiles_x;
  const int ty = (int)(b % (unsigned)tiles_y);
  const int64_t plane = b / (unsigned)tiles_y;
  const int r0 = ty * TR, c0 = tx * TC;         // first gradient pixel = first owned position
  const int sr0 = r0 - HL, sc0 = c0 - HL;       // first staged pixel = first evaluated position
  const int64_t origin = plane * H * W;

  ssim_stage<G>(X, Y, origin, H, W, sr0, sc0, xs, ys, tid);
  __syncthreads();
  ssim_row_sums<WIN, G>(xs, ys, hs, taps, tid);
  __syncthreads();

  double rs[G::NPOS], ra[G::NPOS], rb[G::NPOS], rc[G::NPOS];
#pragma unroll
  for (int n = 0; n < G::NPOS; ++n) {
    const int idx = tid + n * NT;
    rs[n] = ra[n] = rb[n] = rc[n] = 0.0;
    if (idx >= PR * PC) continue;
    const int pi = idx / PC, pj = idx - pi * PC;
    const int i = sr0 + pi, j = sc0 + pj;
    if (i >= 0 && i < Ho && j >= 0 && j < Wo)
      ssim_s_terms<GRAD>(ssim_window_stats<WIN, G>(hs + pi * PC + pj, taps, cn, C2), cn, C1, rs[n], ra[n], rb[n], rc[n]);
  }
  __syncthreads();

  // hs is dead behind this barrier: the registers go over it
  double* abc = hs;                      // [3][PR][PC]
  double* vs = hs + 3 * PR * PC;         // [3][TR][PC]
  double* sown = hs + G::SOWN_AT;        // [TR][TC]
#pragma unroll
  for (int n = 0; n < G::NPOS; ++n) {
    const int idx = tid + n * NT;
    if (idx < PR * PC) {
      const int pi = idx / PC, pj = idx - pi * PC;
      if (pi >= HL && pj >= HL) sown[(pi - HL) * TC + (pj - HL)] = rs[n];
    }
  }
  if (GRAD) ssim_store_abc<G>(abc, ra, rb, rc, tid);
  __syncthreads();

  // the sum of the owned S: the same order with and without the gradient
  {
    double s = 0.0;
    for (int i = tid; i < TR * TC; i += NT) s += sown[i];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
  }

  if (GRAD) {
    ssim_adjoint_rows<WIN, G>(abc, vs, taps, tid);
    __syncthreads();

    if (tid < TR * TC / 4) {
      const int pr = tid / (TC / 4), pc = 4 * (tid - pr * (TC / 4));
      const int R = r0 + pr, Cc = c0 + pc;
      if (R < H && Cc < W) {
        double ga[4] = {0.0, 0.0, 0.0, 0.0}, gb[4] = {0.0, 0.0, 0.0, 0.0}, gc[4] = {0.0, 0.0, 0.0, 0.0};
        ssim_adjoint_quad<WIN, G>(vs + pr * PC + pc, taps, ga, gb, gc);
        const float* xp = xs + (pr + HL) * SC + pc + HL;
        const float* yp = ys + (pr + HL) * SC + pc + HL;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)(-(ga[e] + 2.0 * (double)yp[e] * gb[e] + (double)xp[e] * gc[e]) * inv_cnt);
        ssim_store_quad(grad + origin + (int64_t)R * W + Cc, o, Cc, W);
      }
    }
  }

  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    part[blockIdx.x] = s;
  }
}

// One workgroup: wave w sums the `tiles` workspace entries of images w, w + 4, ... in a fixed order, then wave 0 the images.
__global__ void __launch_bounds__(NT) ssl_finish_kernel(const double* __restrict__ part, int N, int64_t tiles, double n_pos,
                                                        double* __restrict__ ssim, float* __restrict__ loss) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int n = wave; n < N; n += NT / 64) {
    const double* pp = part + (int64_t)n * tiles;
    double s = 0.0;
    for (int64_t t = lane; t < tiles; t += 64) s += pp[t];
    s = wave_sum_f64(s);
    if (lane == 0) ssim[n] = s / n_pos;
  }
  if (!loss) return;
  __syncthreads();
  if (wave == 0) {
    double s = 0.0;
    for (int n = lane; n < N; n += 64) s += ssim[n];
    s = wave_sum_f64(s);
    if (lane == 0) *loss = (float)(1.0 - s / (double)N);
  }
}

int check_shape(const char* who, int N, int C, int H, int W, int win) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
  if (win < 3 || win > 15 || win % 2 == 0) return rdst_fail(RDST_EINVAL, "%s: win=%d must be odd and in [3, 15]", who, win);
  if (H < win || W < win) return rdst_fail(RDST_EINVAL, "%s: the image (%d x %d) is smaller than win=%d", who, H, W, win);
  if ((int64_t)N * C * H * W > ((int64_t)1 << 31))
    return rdst_fail(RDST_EINVAL, "%s: %lld pixels exceed 2^31", who, (long long)((int64_t)N * C * H * W));
  return 0;
}

// tiles per image: the tiles partition the PIXELS of every plane, with or without the gradient
int64_t tiles_per_image(int C, int H, int W, int& tiles_y, int& tiles_x) {
  tiles_y = (H + TR - 1) / TR;
  tiles_x = (W + TC - 1) / TC;
  return (int64_t)C * tiles_y * tiles_x;
}

template <int WIN>
int launch_tiles(bool with_grad, int64_t grid, hipStream_t st, const char* who, const float* X, const float* Y, int H, int W, int ty,
                 int tx, const SsimTaps& taps, double cn, double C1, double C2, double inv_cnt, double* part, float* grad) {
  if (with_grad)
    return rdst_launch(ssl_tile_kernel<WIN, true>, dim3((unsigned)grid), dim3(NT), Geo<WIN, true>::BYTES, st, who, X, Y, H, W, ty, tx,
                       taps, cn, C1, C2, inv_cnt, part, grad);
  return rdst_launch(ssl_tile_kernel<WIN, false>, dim3((unsigned)grid), dim3(NT), Geo<WIN, false>::BYTES, st, who, X, Y, H, W, ty, tx,
                     taps, cn, C1, C2, inv_cnt, part, grad);
}

}  // namespace

extern "C" size_t rdst_ssim_loss_workspace(int N, int C, int H, int W, int win) {
  if (check_shape("rdst_ssim_loss_workspace", N, C, H, W, win)) return 0;
  int ty, tx;
  return (size_t)N * (size_t)tiles_per_image(C, H, W, ty, tx) * sizeof(double);
}

extern "C" int rdst_ssim_loss(const float* target, const float* pred, int N, int C, int H, int W, int win, const double* taps,
                              double cov_norm, double data_range, double* ssim, float* loss, float* grad, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const char* who = "rdst_ssim_loss";
  if (int rc = check_shape(who, N, C, H, W, win)) return rc;
  if (!(cov_norm > 0.0) || !__builtin_isfinite(cov_norm)) return rdst_fail(RDST_EINVAL, "%s: cov_norm=%g must be positive", who, cov_norm);
  if (!(data_range > 0.0) || !__builtin_isfinite(data_range))
    return rdst_fail(RDST_EINVAL, "%s: data_range=%g must be positive", who, data_range);
  if (!target || !pred || !ssim || !workspace) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  SsimTaps tw;
  double sum = 0.0;
  for (int k = 0; k < 15; ++k) {
    tw.w[k] = k < win ? (taps ? taps[k] : 1.0 / (double)win) : 0.0;
    if (!__builtin_isfinite(tw.w[k])) return rdst_fail(RDST_EINVAL, "%s: tap %d is not finite", who, k);
    sum += tw.w[k];
  }
  if (!(fabs(sum - 1.0) <= 1e-9)) return rdst_fail(RDST_EINVAL, "%s: the taps sum to %.12g, not 1", who, sum);
  int ty, tx;
  const int64_t tiles = tiles_per_image(C, H, W, ty, tx);
  const size_t need = (size_t)N * (size_t)tiles * sizeof(double);
  if (workspace_bytes < need)
    return rdst_fail(RDST_EINVAL, "%s: workspace of %zu bytes, %zu needed (rdst_ssim_loss_workspace)", who, workspace_bytes, need);
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const double n_pos = (double)C * (H - win + 1) * (W - win + 1);
  const double inv_cnt = 1.0 / ((double)N * n_pos);
  hipStream_t st = (hipStream_t)stream;
  const int64_t grid = (int64_t)N * tiles;
  double* part = (double*)workspace;
  int rc;
#define SSL_CASE(WIN) \
  case WIN: rc = launch_tiles<WIN>(grad != nullptr, grid, st, who, target, pred, H, W, ty, tx, tw, cov_norm, C1, C2, inv_cnt, part, grad); break
  switch (win) {
    SSL_CASE(3);
    SSL_CASE(5);
    SSL_CASE(7);
    SSL_CASE(9);
    SSL_CASE(11);
    SSL_CASE(13);
    SSL_CASE(15);
    default: return rdst_fail(RDST_EINVAL, "%s: win=%d must be odd and in [3, 15]", who, win);
  }
#undef SSL_CASE
  if (rc) return rc;
  hipLaunchKernelGGL(ssl_finish_kernel, dim3(1), dim3(NT), 0, st, (const double*)part, N, tiles, n_pos, ssim, loss);
  return rdst_launch_status(who);
}
