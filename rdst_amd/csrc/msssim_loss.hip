// The multi-scale SSIM loss and score: the definition is the comment of include/rdst_hip_msssim.h.  The tile, its LDS carve
// and the phases are ssim_tile.h's, shared with the SSIM loss (ssim_loss.hip); here they run over a pyramid:
//   fine to coarse   msl_tile_kernel<WIN, false>, one launch per level: 16 x 32 owned positions, no halo; one fp64 partial per
//                    workgroup of cs = A2 / B2 (levels below the last) or S (the last), and the 8 x 16 pooled pixels of both
//                    images under the owned tile (tiles start on even coordinates, so pooling needs no launch of its own);
//   finish           msl_finish_kernel, one workgroup: per-plane, per-level sums in a fixed order, then m, MS_p, msssim[n],
//                    loss and the table k[p][j] = -MS_p beta_j / (m_{p,j} N C Ho_j Wo_j), all in double;
//   coarse to fine   msl_tile_kernel<WIN, true>, one launch per level, only when the gradient is asked for: the halo geometry
//                    of the SSIM loss; the epilogue adds a quarter of the coarser level's running sum and rounds once:
//                    acc_j = (float)(k[p][j] g64 + 0.25 acc_{j+1}[r / 2][c / 2]); level 1 writes grad.
// 2 M + 1 launches with the gradient, M + 1 without; the value launches are the same either way, so msssim, means and loss
// do not depend on whether the gradient was asked for.  No atomics, fixed-order sums, nothing syncs with the host.
//
// LDS per workgroup (ssim_tile.h): the gradient instantiation needs 51.2 KB at win 7, 73.7 KB at win 11 (two workgroups in a
// CU's 160 KB), the value instantiation 34.9 KB / 42.0 KB (four / three).  The coarse levels keep the 16 x 32 tile: a plane of level 4 or 5 fills
// part of one tile, and those launches are bound by their launch, not by the CU's LDS.
#include "ssim_tile.h"
#include "../../include/rdst_hip_msssim.h"
#include <math.h>

namespace {

using namespace ssim_tile;

constexpr int MAXL = 5;  // levels

// One workgroup per (plane = image * C + channel, tile row, tile column) of ONE level (H x W).  `last` != 0: the level's term is S,
// else cs.  GRAD = false: part[block] = the sum of the term over the owned positions; Xn, Yn (non-null below the last level)
// receive the pooled pixels.  GRAD = true: out (H x W per plane) = (float)(ktab[plane * M + lvl] g64 + 0.25 coarse[r/2][c/2]),
// coarse (Hc x Wc per plane) null at the last level.
template <int WIN, bool GRAD>
__global__ void __launch_bounds__(NT) msl_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                                      int tiles_y, int tiles_x, SsimTaps taps, double cn, double C1, double C2,
                                                      int last, double* __restrict__ part, float* __restrict__ Xn,
                                                      float* __restrict__ Yn, const double* __restrict__ ktab, int M, int lvl,
                                                      const float* __restrict__ coarse, int Hc, int Wc, float* __restrict__ out) {
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
  const int r0 = ty * TR, c0 = tx * TC;         // first owned pixel = first owned position
  const int sr0 = r0 - HL, sc0 = c0 - HL;       // first staged pixel = first evaluated position
  const int64_t origin = plane * H * W;

  ssim_stage<G>(X, Y, origin, H, W, sr0, sc0, xs, ys, tid);
  __syncthreads();
  ssim_row_sums<WIN, G>(xs, ys, hs, taps, tid);

  if (!GRAD && Xn && tid < (TR / 2) * (TC / 2)) {
    // the next level under the owned tile: ((a + b) + (c + d)) * 0.25f in fp32; a pooled pixel inside H/2 x W/2 has all four
    // sources inside the image, and r0, c0 are even
    const int H2 = H >> 1, W2 = W >> 1;
    const int i = tid / (TC / 2), j = tid - i * (TC / 2);
    const int R2 = (r0 >> 1) + i, C2 = (c0 >> 1) + j;
    if (R2 < H2 && C2 < W2) {
      const float* xa = xs + (2 * i) * SC + 2 * j;
      const float* ya = ys + (2 * i) * SC + 2 * j;
      const int64_t at = plane * H2 * W2 + (int64_t)R2 * W2 + C2;
      Xn[at] = ((xa[0] + xa[1]) + (xa[SC] + xa[SC + 1])) * 0.25f;
      Yn[at] = ((ya[0] + ya[1]) + (ya[SC] + ya[SC + 1])) * 0.25f;
    }
  }
  __syncthreads();

  double rs[G::NPOS], ra[G::NPOS], rb[G::NPOS], rc[G::NPOS];
#pragma unroll
  for (int n = 0; n < G::NPOS; ++n) {
    const int idx = tid + n * NT;
    rs[n] = ra[n] = rb[n] = rc[n] = 0.0;
    if (idx >= PR * PC) continue;
    const int pi = idx / PC, pj = idx - pi * PC;
    const int i = sr0 + pi, j = sc0 + pj;
    if (i >= 0 && i < Ho && j >= 0 && j < Wo) {
      const SsimStats t = ssim_window_stats<WIN, G>(hs + pi * PC + pj, taps, cn, C2);
      if (last) ssim_s_terms<GRAD>(t, cn, C1, rs[n], ra[n], rb[n], rc[n]);
      else ssim_cs_terms<GRAD>(t, cn, rs[n], ra[n], rb[n], rc[n]);
    }
  }

  if (!GRAD) {
    // the owned positions are all the evaluated ones: thread, wave, workgroup, in that order
    double s = 0.0;
#pragma unroll
    for (int n = 0; n < G::NPOS; ++n) s += rs[n];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
      double t = 0.0;
      for (int w = 0; w < NT / 64; ++w) t += red[w];
      part[blockIdx.x] = t;
    }
    return;
  }
  __syncthreads();

  // hs is dead behind this barrier: the registers go over it
  double* abc = hs;                      // [3][PR][PC]
  double* vs = hs + 3 * PR * PC;         // [3][TR][PC]
  ssim_store_abc<G>(abc, ra, rb, rc, tid);
  __syncthreads();
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
      const double kk = ktab[plane * M + lvl];
      // the coarser level's running sum: absent on a dropped row or column (R/2 == Hc, C/2 == Wc) and at the last level
      const float* cr = (coarse && (R >> 1) < Hc) ? coarse + (plane * Hc + (R >> 1)) * Wc : nullptr;
      float o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // k == 0 is a clamped plane: exactly zero, whatever its maps hold
        double v = kk != 0.0 ? kk * (ga[e] + 2.0 * (double)yp[e] * gb[e] + (double)xp[e] * gc[e]) : 0.0;
        const int cc = (Cc + e) >> 1;
        if (cr && cc < Wc) v += 0.25 * (double)cr[cc];
        o[e] = (float)v;
      }
      ssim_store_quad(out + origin + (int64_t)R * W + Cc, o, Cc, W);
    }
  }
}

struct MslFinish {
  int M;
  int64_t tiles[MAXL];     // workgroups per plane
  int64_t part_at[MAXL];   // the level's first partial, in doubles
  double n_pos[MAXL];      // Ho_j Wo_j
  double beta[MAXL];
};

// One workgroup of NF threads (16 waves: the sums below are a chain of dependent global reads per wave, and the whole step waits on
// this one workgroup).  Wave w sums the partials of the (plane, level) pairs w, w + 16, ... lane-strided and then across the lanes; a
// thread per plane forms MS_p and the row of k; a thread per image the channel mean; wave 0 the loss.
constexpr int NF = 1024;
__global__ void __launch_bounds__(NF) msl_finish_kernel(const double* __restrict__ part, MslFinish f, int N, int C,
                                                        double* __restrict__ mean, double* __restrict__ ms, double* __restrict__ ktab,
                                                        double* __restrict__ msssim, double* __restrict__ means_out,
                                                        float* __restrict__ loss) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int M = f.M;
  const int64_t P = (int64_t)N * C;
  for (int64_t idx = wave; idx < P * M; idx += NF / 64) {
    const int64_t p = idx / M;
    const int j = (int)(idx - p * M);
    const int64_t tiles = f.tiles[j];
    const double* pp = part + f.part_at[j] + p * tiles;
    double s = 0.0;
    for (int64_t t = lane; t < tiles; t += 64) s += pp[t];
    s = wave_sum_f64(s);
    if (lane == 0) {
      const double m = s / f.n_pos[j];
      mean[idx] = m;
      if (means_out) means_out[idx] = m;
    }
  }
  __syncthreads();
  for (int64_t p = tid; p < P; p += NF) {
    bool ok = true;
    double prod = 1.0;
    for (int j = 0; j < M; ++j) {
      const double m = mean[p * M + j];
      if (m > 0.0) prod *= pow(m, f.beta[j]);
      else ok = false;
    }
    const double MS = ok ? prod : 0.0;
    ms[p] = MS;
    for (int j = 0; j < M; ++j)
      ktab[p * M + j] = ok ? -MS * f.beta[j] / (mean[p * M + j] * (double)N * (double)C) / f.n_pos[j] : 0.0;
  }
  __syncthreads();
  for (int n = tid; n < N; n += NF) {
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += ms[(int64_t)n * C + c];
    msssim[n] = s / (double)C;
  }
  if (!loss) return;
  __syncthreads();
  if (wave == 0) {
    double s = 0.0;
    for (int n = lane; n < N; n += 64) s += msssim[n];
    s = wave_sum_f64(s);
    if (lane == 0) *loss = (float)(1.0 - s / (double)N);
  }
}

// The pyramid and the workspace, from ONE place: the sizes of every level, its tiles, and where each region starts (bytes, every
// offset a multiple of 16).  Regions: the partial sums of every level; mean [P][M], ms [P], k [P][M] (doubles); the pooled
// target and prediction of the levels 2 .. M; with_grad: the running sums of the gradient at the levels 2 .. M.
struct MslLayout {
  int M;
  int H[MAXL], W[MAXL], ty[MAXL], tx[MAXL];
  int64_t tiles[MAXL];      // per plane
  size_t part_at[MAXL], mean_at, ms_at, k_at, x_at[MAXL], y_at[MAXL], acc_at[MAXL];
  size_t bytes;
};

int msl_layout(const char* who, int N, int C, int H, int W, int win, int levels, bool with_grad, MslLayout& L) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d", who, N, C, H, W);
  if (win < 3 || win > 15 || win % 2 == 0) return rdst_fail(RDST_EINVAL, "%s: win=%d must be odd and in [3, 15]", who, win);
  if (levels < 1 || levels > MAXL) return rdst_fail(RDST_EINVAL, "%s: levels=%d must be in [1, %d]", who, levels, MAXL);
  if (((H < W ? H : W) >> (levels - 1)) < win)
    return rdst_fail(RDST_EINVAL, "%s: the image (%d x %d) is too small for %d levels of win=%d: the least side is %d", who, H, W,
                     levels, win, win << (levels - 1));
  if ((int64_t)N * C * H * W > ((int64_t)1 << 31))
    return rdst_fail(RDST_EINVAL, "%s: %lld pixels exceed 2^31", who, (long long)((int64_t)N * C * H * W));
  const size_t P = (size_t)N * C;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  L.M = levels;
  size_t at = 0;
  for (int j = 0; j < levels; ++j) {
    L.H[j] = H >> j;
    L.W[j] = W >> j;
    L.ty[j] = (L.H[j] + TR - 1) / TR;
    L.tx[j] = (L.W[j] + TC - 1) / TC;
    L.tiles[j] = (int64_t)L.ty[j] * L.tx[j];
    L.part_at[j] = at;
    at = up(at + P * (size_t)L.tiles[j] * sizeof(double));
  }
  L.mean_at = at;
  at = up(at + P * levels * sizeof(double));
  L.ms_at = at;
  at = up(at + P * sizeof(double));
  L.k_at = at;
  at = up(at + P * levels * sizeof(double));
  L.x_at[0] = L.y_at[0] = L.acc_at[0] = 0;   // level 1 is the caller's: target, pred and grad
  for (int j = 1; j < levels; ++j) {
    const size_t img = P * (size_t)L.H[j] * L.W[j] * sizeof(float);
    L.x_at[j] = at;
    at = up(at + img);
    L.y_at[j] = at;
    at = up(at + img);
    L.acc_at[j] = at;
    if (with_grad) at = up(at + img);
  }
  L.bytes = at;
  return 0;
}

template <int WIN>
int launch_value(int64_t grid, hipStream_t st, const char* who, const float* X, const float* Y, int H, int W, int ty, int tx,
                 const SsimTaps& taps, double cn, double C1, double C2, int last, double* part, float* Xn, float* Yn) {
  return rdst_launch(msl_tile_kernel<WIN, false>, dim3((unsigned)grid), dim3(NT), Geo<WIN, false>::BYTES, st, who, X, Y, H, W, ty, tx,
                     taps, cn, C1, C2, last, part, Xn, Yn, (const double*)nullptr, 0, 0, (const float*)nullptr, 0, 0, (float*)nullptr);
}

template <int WIN>
int launch_grad(int64_t grid, hipStream_t st, const char* who, const float* X, const float* Y, int H, int W, int ty, int tx,
                const SsimTaps& taps, double cn, double C1, double C2, int last, const double* ktab, int M, int lvl,
                const float* coarse, int Hc, int Wc, float* out) {
  return rdst_launch(msl_tile_kernel<WIN, true>, dim3((unsigned)grid), dim3(NT), Geo<WIN, true>::BYTES, st, who, X, Y, H, W, ty, tx,
                     taps, cn, C1, C2, last, (double*)nullptr, (float*)nullptr, (float*)nullptr, ktab, M, lvl, coarse, Hc, Wc, out);
}

}  // namespace

extern "C" size_t rdst_msssim_loss_workspace(int N, int C, int H, int W, int win, int levels, int with_grad) {
  MslLayout L;
  if (msl_layout("rdst_msssim_loss_workspace", N, C, H, W, win, levels, with_grad != 0, L)) return 0;
  return L.bytes;
}

extern "C" int rdst_msssim_loss(const float* target, const float* pred, int N, int C, int H, int W, int win, const double* taps,
                                double cov_norm, double data_range, int levels, const double* weights, double* msssim,
                                double* means, float* loss, float* grad, void* workspace, size_t workspace_bytes, void* stream) {
  const char* who = "rdst_msssim_loss";
  MslLayout L;
  if (int rc = msl_layout(who, N, C, H, W, win, levels, grad != nullptr, L)) return rc;
  if (!(cov_norm > 0.0) || !__builtin_isfinite(cov_norm)) return rdst_fail(RDST_EINVAL, "%s: cov_norm=%g must be positive", who, cov_norm);
  if (!(data_range > 0.0) || !__builtin_isfinite(data_range))
    return rdst_fail(RDST_EINVAL, "%s: data_range=%g must be positive", who, data_range);
  if (!target || !pred || !msssim || !weights || !workspace) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  SsimTaps tw;
  double sum = 0.0;
  for (int k = 0; k < 15; ++k) {
    tw.w[k] = k < win ? (taps ? taps[k] : 1.0 / (double)win) : 0.0;
    if (!__builtin_isfinite(tw.w[k])) return rdst_fail(RDST_EINVAL, "%s: tap %d is not finite", who, k);
    sum += tw.w[k];
  }
  if (!(fabs(sum - 1.0) <= 1e-9)) return rdst_fail(RDST_EINVAL, "%s: the taps sum to %.12g, not 1", who, sum);
  MslFinish f;
  f.M = levels;
  for (int j = 0; j < MAXL; ++j) {
    f.tiles[j] = f.part_at[j] = 0;
    f.n_pos[j] = f.beta[j] = 1.0;
  }
  for (int j = 0; j < levels; ++j) {
    if (!(weights[j] > 0.0) || !__builtin_isfinite(weights[j]))
      return rdst_fail(RDST_EINVAL, "%s: weight %d = %g must be finite and positive", who, j, weights[j]);
    f.tiles[j] = L.tiles[j];
    f.part_at[j] = (int64_t)(L.part_at[j] / sizeof(double));
    f.n_pos[j] = (double)(L.H[j] - win + 1) * (double)(L.W[j] - win + 1);
    f.beta[j] = weights[j];
  }
  if (workspace_bytes < L.bytes)
    return rdst_fail(RDST_EINVAL, "%s: workspace of %zu bytes, %zu needed (rdst_msssim_loss_workspace)", who, workspace_bytes, L.bytes);
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int64_t P = (int64_t)N * C;
  const float* lx[MAXL];
  const float* ly[MAXL];
  float* acc[MAXL];
  lx[0] = target;
  ly[0] = pred;
  acc[0] = grad;
  for (int j = 1; j < levels; ++j) {
    lx[j] = (const float*)(ws + L.x_at[j]);
    ly[j] = (const float*)(ws + L.y_at[j]);
    acc[j] = (float*)(ws + L.acc_at[j]);
  }
  double* part = (double*)ws;
  double* mean = (double*)(ws + L.mean_at);
  double* ms = (double*)(ws + L.ms_at);
  double* ktab = (double*)(ws + L.k_at);

#define MSL_SWITCH(CALL)                                                                        \
  switch (win) {                                                                                \
    case 3: rc = CALL(3); break;                                                                \
    case 5: rc = CALL(5); break;                                                                \
    case 7: rc = CALL(7); break;                                                                \
    case 9: rc = CALL(9); break;                                                                \
    case 11: rc = CALL(11); break;                                                              \
    case 13: rc = CALL(13); break;                                                              \
    case 15: rc = CALL(15); break;                                                              \
    default: return rdst_fail(RDST_EINVAL, "%s: win=%d must be odd and in [3, 15]", who, win);  \
  }
  int rc = 0;
  for (int j = 0; j < levels; ++j) {   // fine to coarse
    const bool last = j == levels - 1;
#define MSL_VALUE(WIN)                                                                                                        \
  launch_value<WIN>(P * L.tiles[j], st, who, lx[j], ly[j], L.H[j], L.W[j], L.ty[j], L.tx[j], tw, cov_norm, C1, C2, last ? 1 : 0, \
                    part + f.part_at[j], last ? nullptr : (float*)lx[j + 1], last ? nullptr : (float*)ly[j + 1])
    MSL_SWITCH(MSL_VALUE)
#undef MSL_VALUE
    if (rc) return rc;
  }
  hipLaunchKernelGGL(msl_finish_kernel, dim3(1), dim3(NF), 0, st, (const double*)part, f, N, C, mean, ms, ktab, msssim, means, loss);
  if (int e = rdst_launch_status(who)) return e;
  if (!grad) return 0;
  for (int j = levels - 1; j >= 0; --j) {   // coarse to fine
    const bool last = j == levels - 1;
#define MSL_GRAD(WIN)                                                                                                           \
  launch_grad<WIN>(P * L.tiles[j], st, who, lx[j], ly[j], L.H[j], L.W[j], L.ty[j], L.tx[j], tw, cov_norm, C1, C2, last ? 1 : 0,  \
                   ktab, levels, j, last ? nullptr : acc[j + 1], last ? 0 : L.H[j + 1], last ? 0 : L.W[j + 1], acc[j])
    MSL_SWITCH(MSL_GRAD)
#undef MSL_GRAD
    if (rc) return rc;
  }
#undef MSL_SWITCH
  return 0;
}
