// The register-stationary 3x3 convolution (conv3_kernel.h) on fp32 rows in the RDST_F32X3 arithmetic: the arithmetic policy, the
// pack kernel and the entry points of conv.h with their per-shape launch tables.
#include "conv3_kernel.h"

namespace {

__global__ void __launch_bounds__(256) conv3x_pack_kernel(const float* __restrict__ Wc, uint32_t* __restrict__ out, int Cin,
                                                          int Cout, int K, int N, int ksteps, int ctiles, int mode, float s, int cmul,
                                                          int coff) {
  conv3x_pack_block((int)blockIdx.x, Wc, out, Cin, Cout, K, N, ksteps, ctiles, mode, s, cmul, coff);
}

struct C3X3 {
  using T = float;                    // rows: input, residual, output
  using WT = uint32_t;                // packed-weight word
  static constexpr int EB = 4;
  static constexpr bool X3 = true;
  static constexpr const char* STAMPS = "RDST_C3X_STAMPS";
  // pixel (y, x) of the conv's grid = memory pixel (y ymul + yoff, x xmul + xoff) of A (a sub-pixel view)
  struct In { const float* A; int64_t lda; int a_bytes; int ymul, yoff, xmul, xoff; };
  static int pack(const float* Wc, uint32_t* out, int Cin, int Cout, int K, int N, int mode, float s, hipStream_t st, int cmul = 1,
                  int coff = 0) {
    hipLaunchKernelGGL(conv3x_pack_kernel, dim3((unsigned)conv3x_pack_blocks(K, N)), dim3(256), 0, st, Wc, out, Cin, Cout, K, N,
                       (K + 15) / 16, (N + 31) / 32, mode, s, cmul, coff);
    return rdst_launch_status("conv3x_pack");
  }
};
using Args = C3Args<C3X3>;

}  // namespace

size_t conv3x_pack_bytes(int Cin, int Cout) { return c3_pack_bytes<C3X3>(Cin, Cout); }

int conv3x_fwd_shape(int Cin, int Cout, int ks, int r, bool has_res, int in_act) { return c3_fwd_shape(Cin, Cout, ks, r, has_res, in_act); }

int conv3x_fwd_f32(const float* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const float* R, int64_t ldr,
                   float* Y, int64_t ldy, const ConvGeom& g, float s, void* wpack, bool prepacked, hipStream_t st) {
  Args p{};
  int shape;
  if (int rc = c3_fwd_args(p, shape, X, ldx, in_act, Wc, bias, R, ldr, Y, ldy, g, s, wpack, prepacked, st)) return rc;
  p.ymul = 1; p.xmul = 1;
  if (shape == 1) return launch_c3<C3X3, 150, 2, 1, 2, 1, 2, false, false>(p, 0, st, "conv3x_fwd_150_60");
  if (shape == 2) return launch_c3<C3X3, 60, 2, 1, 1, 2, 2, false, false>(p, 0, st, "conv3x_fwd_60_60");
  Args pa = p;
  if (int rc = launch_c3<C3X3, 60, 4, 1, 1, 1, 2, false, true>(pa, 0, st, "conv3x_fwd_60_240_ps_a")) return rc;
  return launch_c3<C3X3, 60, 4, 1, 1, 1, 2, false, true>(p, 4, st, "conv3x_fwd_60_240_ps_b");
}

// conv + PixelShuffle(2): the shuffled dY as it lies — four launches of the 60 -> 60 form, one per sub-pixel q = 2 i + j (dY through a
// stride-2 pixel view, the weights of conv channels 4 c' + q), each accumulating onto the last.
int conv3x_dgrad_f32(const float* Wc, const float* dY, int64_t lddy, float* dX, int64_t lddx, const float* acc, int64_t ldacc,
                     int in_act, const ConvGeom& g, float s, void* wpack, hipStream_t st) {
  Args p{};
  int shape;
  if (int rc = c3_dgrad_args(p, shape, dY, lddy, dX, lddx, acc, ldacc, in_act, g, s, wpack)) return rc;
  p.ymul = 1; p.xmul = 1;
  uint32_t* wp = reinterpret_cast<uint32_t*>(wpack);
  if (shape == 3) {
    constexpr int IMG = 2 * 9 * 4 * 512;   // uint32 per sub-pixel image: 2 channel tiles x 9 taps x 4 k-steps x 2 KB
    for (int q = 0; q < 4; ++q)
      if (int rc = C3X3::pack(Wc, wp + (size_t)q * IMG, g.Cin, g.Cout, 60, g.Cin, PK_DGRAD, s, st, 4, q)) return rc;
    for (int q = 0; q < 4; ++q) {
      Args pq = p;
      pq.Wp = wp + (size_t)q * IMG; pq.ymul = 2; pq.yoff = q >> 1; pq.xmul = 2; pq.xoff = q & 1;
      if (q > 0) { pq.R = dX; pq.ldr = lddx; }
      if (int rc = launch_c3<C3X3, 60, 2, 1, 1, 2, 2, false, false>(pq, 0, st, "conv3x_dgrad_240_60_q")) return rc;
    }
    return 0;
  }
  if (int rc = C3X3::pack(Wc, wp, g.Cin, g.Cout, g.Cout, g.Cin, PK_DGRAD, s, st)) return rc;
  if (shape == 1) {
    Args pa = p;
    if (int rc = launch_c3<C3X3, 60, 4, 1, 1, 1, 2, false, false>(pa, 0, st, "conv3x_dgrad_60_150a")) return rc;
    return launch_c3<C3X3, 60, 1, 1, 1, 4, 4, false, false>(p, 4, st, "conv3x_dgrad_60_150b");
  }
  return launch_c3<C3X3, 60, 2, 1, 1, 2, 2, false, false>(p, 0, st, "conv3x_dgrad_60_60");
}
