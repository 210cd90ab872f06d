// The tile of the SSIM kernels (ssim_loss.hip, msssim_loss.hip): geometry, LDS carve and the phases both kernels are made of.
//
// A 256-thread workgroup takes TR x TC = 16 x 32 pixels of one (image, channel) plane.  A pixel's gradient needs the window
// positions whose window holds it: HL = win-1 more rows above and columns to the left of the tile, so with GRAD the workgroup
// evaluates PR x PC = (TR+HL) x (TC+HL) positions and stages the SR x SC = (PR+win-1) x (PC+win-1) pixels under them (zeros
// outside the image); without, HL = 0.  The phases, a barrier between each (the kernels place the barriers):
//   1  ssim_stage            X (target) and Y (pred) as fp32                                        xs, ys [SR][SC]
//   2  ssim_row_sums         horizontal weighted sums of X, Y, X^2, Y^2, XY in fp64                 hs [5][SR][PC]
//   3  ssim_window_stats     vertical sums -> ux, uy, A2, B2 of one position; ssim_s_terms / ssim_cs_terms turn them into
//                            the term (S or cs = A2 / B2) and the adjoint inputs a, b, c, kept in REGISTERS over a barrier
//   4  ssim_store_abc        over the dead hs planes                                                abc [3][PR][PC]
//   5  ssim_adjoint_rows     the adjoint's vertical sums                                            vs [3][TR][PC]
//   6  ssim_adjoint_quad     the adjoint's horizontal sums of four neighbouring pixels of one row
// `win` is a template parameter: the tap loops unroll, the taps sit in scalar registers and the LDS geometry is constant.
// Phase 3 runs without fused multiply-adds: pred == target then gives A1 == B1 and A2 == B2 bit for bit, S = cs = 1 and a
// zero gradient.
//
// LDS, deliberate: holding the term and a, b, c in registers over a barrier lets abc and vs (and the SSIM loss's sown) reuse
// hs, so a workgroup needs hs + xs + ys = 51.2 KB at win 7 (three workgroups in a CU's 160 KB), 73.7 KB at win 11 (two),
// 99.7 KB at win 15 (one) instead of 75 / 104 / 137 KB with planes of their own (two, one, one).
#pragma once
#include "common.h"

namespace ssim_tile {

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

// phase 1: the SR x SC pixels from (sr0, sc0) of the plane at `origin`, zeros outside the image
template <class G>
__device__ __forceinline__ void ssim_stage(const float* __restrict__ X, const float* __restrict__ Y, int64_t origin, int H, int W,
                                           int sr0, int sc0, float* xs, float* ys, int tid) {
  constexpr int SR = G::SR, SC = G::SC;
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
}

// phase 2
template <int WIN, class G>
__device__ __forceinline__ void ssim_row_sums(const float* xs, const float* ys, double* hs, const SsimTaps& taps, int tid) {
  constexpr int PC = G::PC, SR = G::SR, SC = G::SC;
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
}

struct SsimStats {
  double ux, uy, A2, B2;
};

// phase 3, one position: h = hs + pi * PC + pj
template <int WIN, class G>
__device__ __forceinline__ SsimStats ssim_window_stats(const double* h, const SsimTaps& taps, double cn, double C2) {
#pragma clang fp contract(off)
  constexpr int PC = G::PC;
  constexpr int plane_sz = G::SR * PC;
  double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
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
  return {ux, uy, 2.0 * vxy + C2, vx + vy + C2};
}

// S = A1 A2 / (B1 B2) and, with GRAD, the a, b, c of d S (the comment on rdst_ssim_loss in include/rdst_hip.h)
template <bool GRAD>
__device__ __forceinline__ void ssim_s_terms(const SsimStats& t, double cn, double C1, double& S, double& a, double& b, double& c) {
#pragma clang fp contract(off)
  const double ux = t.ux, uy = t.uy, A2 = t.A2, B2 = t.B2;
  const double A1 = 2.0 * ux * uy + C1, B1 = ux * ux + uy * uy + C1;
  const double iB = 1.0 / (B1 * B2);
  S = (A1 * A2) / (B1 * B2);
  if (GRAD) {
    a = 2.0 * ux * A2 * iB - 2.0 * uy * S / B1 - 2.0 * cn * ux * A1 * iB + 2.0 * cn * uy * S / B2;
    b = -cn * S / B2;
    c = 2.0 * cn * A1 * iB;
  }
}

// cs = A2 / B2 and, with GRAD, the a', b', c' of d cs (include/rdst_hip_msssim.h)
template <bool GRAD>
__device__ __forceinline__ void ssim_cs_terms(const SsimStats& t, double cn, double& cs, double& a, double& b, double& c) {
#pragma clang fp contract(off)
  cs = t.A2 / t.B2;
  if (GRAD) {
    a = 2.0 * cn * (cs * t.uy - t.ux) / t.B2;
    b = -cn * cs / t.B2;
    c = 2.0 * cn / t.B2;
  }
}

// phase 4: a, b, c of the thread's positions into abc [3][PR][PC]
template <class G>
__device__ __forceinline__ void ssim_store_abc(double* abc, const double* ra, const double* rb, const double* rc, int tid) {
  constexpr int PR = G::PR, PC = G::PC;
#pragma unroll
  for (int n = 0; n < G::NPOS; ++n) {
    const int idx = tid + n * NT;
    if (idx < PR * PC) {
      abc[idx] = ra[n];
      abc[PR * PC + idx] = rb[n];
      abc[2 * PR * PC + idx] = rc[n];
    }
  }
}

// phase 5: pixel row pr lies in the windows of the position rows pr .. pr + WIN-1 (local), under tap WIN-1 .. 0
template <int WIN, class G>
__device__ __forceinline__ void ssim_adjoint_rows(const double* abc, double* vs, const SsimTaps& taps, int tid) {
  constexpr int PR = G::PR, PC = G::PC;
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
}

// phase 6: the sums of the pixels (pr, pc .. pc + 3), q = vs + pr * PC + pc
template <int WIN, class G>
__device__ __forceinline__ void ssim_adjoint_quad(const double* q, const SsimTaps& taps, double (&ga)[4], double (&gb)[4],
                                                  double (&gc)[4]) {
  constexpr int PC = G::PC;
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
}

// four gradient values to out[0 .. 3], of which those before column W exist: one 16-byte store where aligned
__device__ __forceinline__ void ssim_store_quad(float* out, const float (&o)[4], int Cc, int W) {
  if (Cc + 3 < W && ((uintptr_t)out & 15) == 0) {
    *reinterpret_cast<float4*>(out) = make_float4(o[0], o[1], o[2], o[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (Cc + e < W) out[e] = o[e];
  }
}

}  // namespace ssim_tile
