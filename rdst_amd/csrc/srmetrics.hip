// PSNR / SSIM scoring of super-resolved images on the device: the per-image MSE and SSIM of rdst_amd/metrics.py (the
// reference's scikit-image calls, metrics/sr_metrics.py:8-14, after the border crop of :108-115), in fp64 throughout.
//
// The SSIM of an image is the mean of the SSIM map over its INTERIOR: the cropped image without the (win-1)/2 = p pixels at
// each edge.  The win x win window of an interior pixel lies wholly inside the cropped image, so no reflected pixel of the
// filter's border ever enters the result: the kernel computes the map on the interior only and reads nothing outside the
// crop.  Tiles are TR x TC interior pixels of one (image, channel); a workgroup stages the (TR + 2p) x (TC + 2p) cropped
// pixels they need of both images in LDS as fp32, forms the five horizontal win-sums (X, Y, X^2, Y^2, XY) of every staged
// row and output column in fp64 (products of two fp32 values are exact in fp64), then the vertical win-sums and the SSIM
// expression per pixel.  The squared error is summed over the staged pixels the tile OWNS (the interior tiles partition
// the cropped image once the border bands are given to the first and last tiles).  Every workgroup writes one (sum of
// squared errors, sum of SSIM) pair to the workspace; a second kernel sums the pairs of each image in a fixed order.
// No atomics: the results are bit-identical run to run.
#include "common.h"

namespace {

constexpr int TR = 16;    // interior rows per tile
constexpr int TC = 64;    // interior columns per tile: one wave per staged row in the horizontal pass
constexpr int NT = 256;

int smem_bytes(int win) {
  const int p = (win - 1) / 2, SR = TR + 2 * p, SW = TC + 2 * p;
  return 5 * SR * TC * (int)sizeof(double) + 2 * SR * SW * (int)sizeof(float);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// one workgroup per (plane = image * C + channel, tile row, tile column); part[block] = (sum (g - p)^2, sum SSIM)
__global__ void __launch_bounds__(NT) srm_tile_kernel(const float* __restrict__ gt, const float* __restrict__ pred, int H,
                                                      int W, int m, int win, int tiles_y, int tiles_x, double C1, double C2,
                                                      double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int p = (win - 1) / 2;
  const int Hc = H - 2 * m, Wc = W - 2 * m, Ho = Hc - 2 * p, Wo = Wc - 2 * p;
  const int SR = TR + 2 * p, SW = TC + 2 * p;
  unsigned b = blockIdx.x;
  const int tx = (int)(b % (unsigned)tiles_x);
  b /= (unsigned)tiles_x;
  const int ty = (int)(b % (unsigned)tiles_y);
  const int64_t plane = b / (unsigned)tiles_y;
  const int r0 = ty * TR, c0 = tx * TC;        // first interior row / column = first staged cropped row / column
  double* hs = smem;                           // [5][SR][TC] horizontal sums
  float* xs = reinterpret_cast<float*>(smem + 5 * SR * TC);   // [SR][SW] staged gt, then pred
  float* ys = xs + SR * SW;
  const int64_t origin = plane * H * W + (int64_t)m * W + m;
  const float* g = gt + origin;
  const float* q = pred + origin;

  // the cropped pixels whose squared error this tile adds: its interior rows / columns shifted by p, plus the border
  // bands [0, p) and [Hc - p, Hc) for the first and the last tile
  const int rlo = ty == 0 ? 0 : r0 + p, rhi = ty == tiles_y - 1 ? Hc : r0 + TR + p;
  const int clo = tx == 0 ? 0 : c0 + p, chi = tx == tiles_x - 1 ? Wc : c0 + TC + p;
  double sq = 0.0;
  for (int i = threadIdx.x; i < SR * SW; i += NT) {
    const int r = i / SW, c = i - r * SW;
    const int R = r0 + r, Cc = c0 + c;
    float a = 0.f, e = 0.f;                    // (staged entries past the crop feed masked pixels only)
    if (R < Hc && Cc < Wc) {
      a = g[(int64_t)R * W + Cc];
      e = q[(int64_t)R * W + Cc];
      if (R >= rlo && R < rhi && Cc >= clo && Cc < chi) {
        const double d = (double)a - (double)e;
        sq += d * d;
      }
    }
    xs[i] = a;
    ys[i] = e;
  }
  __syncthreads();

  const int plane_sz = SR * TC;
  for (int i = threadIdx.x; i < SR * TC; i += NT) {
    const int r = i / TC, c = i - r * TC;
    const float* xr = xs + r * SW + c;
    const float* yr = ys + r * SW + c;
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sxy = 0.0;
    for (int k = 0; k < win; ++k) {
      const double x = xr[k], y = yr[k];
      sx += x;
      sy += y;
      sxx += x * x;
      syy += y * y;
      sxy += x * y;
    }
    hs[i] = sx;
    hs[plane_sz + i] = sy;
    hs[2 * plane_sz + i] = sxx;
    hs[3 * plane_sz + i] = syy;
    hs[4 * plane_sz + i] = sxy;
  }
  __syncthreads();

  double ssum = 0.0;
  {
    // rounded as numpy rounds it (no fused multiply-adds): gt == pred then gives exactly 1 per pixel
#pragma clang fp contract(off)
    const double NP = (double)win * (double)win;
    const double cov_norm = NP / (NP - 1.0);
    for (int i = threadIdx.x; i < TR * TC; i += NT) {
      const int r = i / TC, c = i - r * TC;
      if (r0 + r >= Ho || c0 + c >= Wo) continue;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
      const double* h = hs + r * TC + c;
      for (int k = 0; k < win; ++k, h += TC) {
        s0 += h[0];
        s1 += h[plane_sz];
        s2 += h[2 * plane_sz];
        s3 += h[3 * plane_sz];
        s4 += h[4 * plane_sz];
      }
      const double ux = s0 / NP, uy = s1 / NP, uxx = s2 / NP, uyy = s3 / NP, uxy = s4 / NP;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      ssum += ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
  }

  __shared__ double red[NT / 64][2];
  sq = wave_sum_f64(sq);
  ssum = wave_sum_f64(ssum);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6][0] = sq;
    red[threadIdx.x >> 6][1] = ssum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, s = 0.0;
    for (int w = 0; w < NT / 64; ++w) {
      a += red[w][0];
      s += red[w][1];
    }
    part[2 * (int64_t)blockIdx.x] = a;
    part[2 * (int64_t)blockIdx.x + 1] = s;
  }
}

// one wave per image: the `tiles` workspace pairs of image blockIdx.x in a fixed order
__global__ void __launch_bounds__(64) srm_finish_kernel(const double* __restrict__ part, int tiles, double n_mse,
                                                        double n_ssim, double* __restrict__ mse, double* __restrict__ ssim) {
  const double* pp = part + 2 * (int64_t)blockIdx.x * tiles;
  double a = 0.0, s = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) {
    a += pp[2 * t];
    s += pp[2 * t + 1];
  }
  a = wave_sum_f64(a);
  s = wave_sum_f64(s);
  if (threadIdx.x == 0) {
    mse[blockIdx.x] = a / n_mse;
    ssim[blockIdx.x] = s / n_ssim;
  }
}

// tiles per image (0: bad arguments)
int64_t tiles_per_image(int C, int H, int W, int margin, int win, int& tiles_y, int& tiles_x) {
  const int p = (win - 1) / 2;
  const int Ho = H - 2 * margin - 2 * p, Wo = W - 2 * margin - 2 * p;
  if (Ho <= 0 || Wo <= 0) return 0;
  tiles_y = (Ho + TR - 1) / TR;
  tiles_x = (Wo + TC - 1) / TC;
  return (int64_t)C * tiles_y * tiles_x;
}

int check_shape(const char* who, int N, int C, int H, int W, int margin, int win) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || margin < 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d margin=%d", who, N, C, H, W, margin);
  if (win < 3 || win > 15 || win % 2 == 0) return rdst_fail(RDST_EINVAL, "%s: win=%d must be odd and in [3, 15]", who, win);
  if ((int64_t)H - 2 * (int64_t)margin < win || (int64_t)W - 2 * (int64_t)margin < win)
    return rdst_fail(RDST_EINVAL, "%s: the cropped image (%lld x %lld) is smaller than win=%d", who,
                     (long long)((int64_t)H - 2 * (int64_t)margin), (long long)((int64_t)W - 2 * (int64_t)margin), win);
  if ((int64_t)N * C * H * W > ((int64_t)1 << 31))
    return rdst_fail(RDST_EINVAL, "%s: %lld pixels exceed 2^31", who, (long long)((int64_t)N * C * H * W));
  return 0;
}

}  // namespace

extern "C" size_t rdst_sr_scores_workspace(int N, int C, int H, int W, int margin, int win) {
  if (check_shape("rdst_sr_scores_workspace", N, C, H, W, margin, win)) return 0;
  int ty, tx;
  return (size_t)N * (size_t)tiles_per_image(C, H, W, margin, win, ty, tx) * 2 * sizeof(double);
}

extern "C" int rdst_sr_scores(const float* gt, const float* pred, int N, int C, int H, int W, int margin, int win,
                              double data_range, double* mse, double* ssim, void* workspace, size_t workspace_bytes,
                              void* stream) {
  const char* who = "rdst_sr_scores";
  if (int rc = check_shape(who, N, C, H, W, margin, win)) return rc;
  if (!(data_range > 0.0)) return rdst_fail(RDST_EINVAL, "%s: data_range=%g must be positive", who, data_range);
  if (!gt || !pred || !mse || !ssim || !workspace) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  int ty, tx;
  const int64_t tiles = tiles_per_image(C, H, W, margin, win, ty, tx);
  const size_t need = (size_t)N * (size_t)tiles * 2 * sizeof(double);
  if (workspace_bytes < need)
    return rdst_fail(RDST_EINVAL, "%s: workspace of %zu bytes, %zu needed (rdst_sr_scores_workspace)", who, workspace_bytes,
                     need);
  const int p = (win - 1) / 2;
  const int Hc = H - 2 * margin, Wc = W - 2 * margin;
  const double C1 = (0.01 * data_range) * (0.01 * data_range), C2 = (0.03 * data_range) * (0.03 * data_range);
  const int smem = smem_bytes(win);
  hipStream_t st = (hipStream_t)stream;
  if (int rc = rdst_launch(srm_tile_kernel, dim3((unsigned)(N * tiles)), dim3(NT), smem, st, who, gt, pred, H, W, margin, win, ty, tx,
                           C1, C2, (double*)workspace))
    return rc;
  hipLaunchKernelGGL(srm_finish_kernel, dim3((unsigned)N), dim3(64), 0, st, (const double*)workspace, (int)tiles,
                     (double)C * Hc * Wc, (double)C * (Hc - 2 * p) * (Wc - 2 * p), mse, ssim);
  return rdst_launch_status(who);
}
