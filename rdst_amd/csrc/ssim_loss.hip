// The SSIM training loss: loss = 1 - mean_n ssim[n] and d loss / d pred in ONE tile kernel plus a small finish kernel; the
// definition is the comment on rdst_ssim_loss in include/rdst_hip.h.  Window arithmetic is fp64 as in srmetrics.hip
// (products of two fp32 values are exact there), sums run in a fixed order, nothing is atomic: results are bit-identical
// run to run.
//
// A 256-thread workgroup takes TR x TC = 16 x 32 gradient pixels of one (image, channel) plane.  A pixel's gradient needs
// the window positions whose window holds it: HL = win-1 more rows above and columns to the left of the tile, so the
// workgroup evaluates PR x PC = (TR+HL) x (TC+HL) positions and stages the SR x SC = (PR+win-1) x (PC+win-1) pixels under
// them (zeros outside the image).  The phases, a barrier between each:
//   1  stage X (target) and Y (pred) as fp32                                              xs, ys [SR][SC]
//   2  horizontal weighted sums of X, Y, X^2, Y^2, XY in fp64                             hs [5][SR][PC]
//   3  vertical sums -> S, a, b, c per position (zero outside [0,Ho) x [0,Wo)), kept in REGISTERS
//   4  over the dead hs planes: a, b, c                                                   abc [3][PR][PC]
//      and S of the positions the tile owns (position (i,j) belongs to the tile holding pixel (i,j))   sown [TR][TC]
//   5  the adjoint's vertical sums                                                        vs [3][TR][PC]
//   6  the adjoint's horizontal sums, four pixels per thread, one rounding to fp32, one 16-byte store where aligned
// and the sum of sown in an order that does not depend on whether the gradient was asked for: the value-only
// instantiation (HL = 0, abc and phases 5-6 dropped) returns the same bits.  `win` is a template parameter: the tap loops unroll,
// the taps sit in scalar registers and the LDS geometry is constant.
//
// LDS, deliberate: holding S, a, b, c in registers over a barrier lets abc, vs and sown reuse hs, so a workgroup needs
// hs + xs + ys = 51.2 KB at win 7 (three workgroups in a CU's 160 KB), 73.7 KB at win 11 (two), 99.7 KB at win 15 (one)
// instead of 75 / 104 / 137 KB with planes of their own (two, one, one).
#include "common.h"
#include <math.h>

namespace {

constexpr int TR = 16;   // gradient rows per tile
constexpr int TC = 32;   // gradient columns per tile
constexpr int NT = 256;

struct SsimTaps {
  double w[15];
};

constexpr int imax(int a, int b) { return a > b ? a : b; }

template <int WIN, bool GRAD>
struct Geo {
  static constexpr int HL = GRAD ? WIN - 1 : 0;
  static constexpr int PR = TR + HL, PC = TC + HL;             // window positions
  static constexpr int SR = PR + WIN - 1, SC = PC + WIN - 1;   // staged pixels
  static constexpr int NPOS = (PR * PC + NT - 1) / NT;         // positions per thread
  // doubles: [0, 4) the waves' sums, then hs (abc, vs and sown reuse it); every carve offset is a multiple of 16 bytes
  static constexpr int RED_D = 4;
  static constexpr int SOWN_AT = GRAD ? 3 * PR * PC + 3 * TR * PC : 0;
  static constexpr int HS_D = (imax(5 * SR * PC, SOWN_AT + TR * TC) + 1) & ~1;
  static constexpr int XS_F = (SR * SC + 3) & ~3;
  static constexpr int BYTES = (RED_D + HS_D) * 8 + 2 * XS_F * 4;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one workgroup per (plane = image * C + channel, tile row, tile column); part[block] = sum of S over the owned positions
template <int WIN, bool GRAD>
__global__ void __launch_bounds__(NT) ssl_tile_kernel(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                                      int tiles_y, int tiles_x, SsimTaps taps, double cn, double C1, double C2,
                                                      double inv_cnt, double* __restrict__ part, float* __restrict__ grad) {
  using G = Geo<WIN, GRAD>;
  constexpr int HL = G::HL, PR = G::PR, PC = G::PC, SR = G::SR, SC = G::SC;
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

  for (int i = tid; i < SR * SC; i += NT) {
    const int r = i / SC, c = i - r * SC;
    const int R = sr0 + r, Cc = sc0 + c;
    float x = 0.f, y = 0.f;
    if (R >= 0 && R < H && Cc >= 0 && Cc < W) {
      const int64_t at = origin + (int64_t)R * W + Cc;
      x = X[at];
      y = Y[at];
    }
    xs[i] = x;
    ys[i] = y;
  }
  __syncthreads();

  constexpr int plane_sz = SR * PC;
  for (int i = tid; i < SR * PC; i += NT) {
    const int r = i / PC, c = i - r * PC;
    const float* xr = xs + r * SC + c;
    const float* yr = ys + r * SC + c;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int k = 0; k < WIN; ++k) {
      const double w = taps.w[k], x = xr[k], y = yr[k];
      sx += w * x;
      sy += w * y;
      sxx += w * (x * x);
      syy += w * (y * y);
      sxy += w * (x * y);
    }
    hs[i] = sx;
    hs[plane_sz + i] = sy;
    hs[2 * plane_sz + i] = sxx;
    hs[3 * plane_sz + i] = syy;
    hs[4 * plane_sz + i] = sxy;
  }
  __syncthreads();

  double rs[G::NPOS], ra[G::NPOS], rb[G::NPOS], rc[G::NPOS];
  {
    // no fused multiply-adds: pred == target then gives A1 == B1 and A2 == B2 bit for bit, S = 1 and a zero gradient
#pragma clang fp contract(off)
#pragma unroll
    for (int n = 0; n < G::NPOS; ++n) {
      const int idx = tid + n * NT;
      rs[n] = ra[n] = rb[n] = rc[n] = 0.0;
      if (idx >= PR * PC) continue;
      const int pi = idx / PC, pj = idx - pi * PC;
      const int i = sr0 + pi, j = sc0 + pj;
      if (i >= 0 && i < Ho && j >= 0 && j < Wo) {
        double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
        const double* h = hs + pi * PC + pj;
#pragma unroll
        for (int k = 0; k < WIN; ++k, h += PC) {
          const double w = taps.w[k];
          ux += w * h[0];
          uy += w * h[plane_sz];
          uxx += w * h[2 * plane_sz];
          uyy += w * h[3 * plane_sz];
          uxy += w * h[4 * plane_sz];
        }
        const double vx = cn * (uxx - ux * ux), vy = cn * (uyy - uy * uy), vxy = cn * (uxy - ux * uy);
        const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
        const double iB = 1.0 / (B1 * B2);
        const double S = (A1 * A2) / (B1 * B2);
        rs[n] = S;
        if (GRAD) {
          ra[n] = 2.0 * ux * A2 * iB - 2.0 * uy * S / B1 - 2.0 * cn * ux * A1 * iB + 2.0 * cn * uy * S / B2;
          rb[n] = -cn * S / B2;
          rc[n] = 2.0 * cn * A1 * iB;
        }
      }
    }
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
      if (GRAD) {
        abc[idx] = ra[n];
        abc[PR * PC + idx] = rb[n];
        abc[2 * PR * PC + idx] = rc[n];
      }
    }
  }
  __syncthreads();

  // the sum of the owned S: the same order with and without the gradient
  {
    double s = 0.0;
    for (int i = tid; i < TR * TC; i += NT) s += sown[i];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
  }

  if (GRAD) {

    // pixel row pr lies in the windows of the position rows pr .. pr + WIN-1 (local), under tap WIN-1 .. 0
    for (int i = tid; i < TR * PC; i += NT) {
      const int pr = i / PC, pj = i - pr * PC;
      const double* q = abc + pr * PC + pj;
      double va = 0.0, vb = 0.0, vc = 0.0;
#pragma unroll
      for (int k = 0; k < WIN; ++k, q += PC) {
        const double w = taps.w[WIN - 1 - k];
        va += w * q[0];
        vb += w * q[PR * PC];
        vc += w * q[2 * PR * PC];
      }
      vs[i] = va;
      vs[TR * PC + i] = vb;
      vs[2 * TR * PC + i] = vc;
    }
    __syncthreads();

    if (tid < TR * TC / 4) {
      const int pr = tid / (TC / 4), pc = 4 * (tid - pr * (TC / 4));
      const int R = r0 + pr, Cc = c0 + pc;
      if (R < H && Cc < W) {
        double ga[4] = {0.0, 0.0, 0.0, 0.0}, gb[4] = {0.0, 0.0, 0.0, 0.0}, gc[4] = {0.0, 0.0, 0.0, 0.0};
        const double* q = vs + pr * PC + pc;
#pragma unroll
        for (int m = 0; m < WIN + 3; ++m) {
          const double va = q[m], vb = q[TR * PC + m], vc = q[2 * TR * PC + m];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int l = e + WIN - 1 - m;     // pixel column pc + e under tap l of position column pc + m
            if (l >= 0 && l < WIN) {
              ga[e] += taps.w[l] * va;
              gb[e] += taps.w[l] * vb;
              gc[e] += taps.w[l] * vc;
            }
          }
        }
        const float* xp = xs + (pr + HL) * SC + pc + HL;
        const float* yp = ys + (pr + HL) * SC + pc + HL;
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (float)(-(ga[e] + 2.0 * (double)yp[e] * gb[e] + (double)xp[e] * gc[e]) * inv_cnt);
        float* out = grad + origin + (int64_t)R * W + Cc;
        if (Cc + 3 < W && ((uintptr_t)out & 15) == 0) {
          *reinterpret_cast<float4*>(out) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (Cc + e < W) out[e] = o[e];
        }
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
