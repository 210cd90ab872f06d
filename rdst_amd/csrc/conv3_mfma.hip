// The register-stationary 3x3 convolution (conv3_kernel.h) on bf16 rows: the arithmetic policy, the pack kernel and the entry
// points of conv.h with their per-shape launch tables.
#include "conv3_kernel.h"

namespace {

__global__ void __launch_bounds__(256) conv3_pack_kernel(const float* __restrict__ Wc, bf16* __restrict__ out, int Cin,
                                                         int Cout, int K, int N, int ksteps, int ctiles, int mode, float s) {
  conv3_pack_block((int)blockIdx.x, Wc, out, Cin, Cout, K, N, ksteps, ctiles, mode, s);
}

struct C3Bf16 {
  using T = bf16;                     // rows: input, residual, output
  using WT = bf16;                    // packed-weight word
  static constexpr int EB = 2;
  static constexpr bool X3 = false;
  static constexpr const char* STAMPS = "RDST_C3_STAMPS";
  struct In { const bf16* A; int64_t lda; int a_bytes; };
  static int pack(const float* Wc, bf16* out, int Cin, int Cout, int K, int N, int mode, float s, hipStream_t st) {
    const int ksteps = (K + 15) / 16, ctiles = (N + 31) / 32;
    hipLaunchKernelGGL(conv3_pack_kernel, dim3((unsigned)conv3_pack_blocks(K, N)), dim3(256), 0, st, Wc, out, Cin, Cout, K, N, ksteps,
                       ctiles, mode, s);
    return rdst_launch_status("conv3_pack");
  }
};
using Args = C3Args<C3Bf16>;

}  // namespace

size_t conv3_pack_bytes(int Cin, int Cout) { return c3_pack_bytes<C3Bf16>(Cin, Cout); }

int conv3_fwd_shape(int Cin, int Cout, int ks, int r, bool has_res, int in_act) { return c3_fwd_shape(Cin, Cout, ks, r, has_res, in_act); }

int conv3_fwd_bf16(const bf16* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const bf16* R, int64_t ldr,
                   bf16* Y, int64_t ldy, const ConvGeom& g, float s, void* wpack, bool prepacked, hipStream_t st) {
  Args p{};
  int shape;
  if (int rc = c3_fwd_args(p, shape, X, ldx, in_act, Wc, bias, R, ldr, Y, ldy, g, s, wpack, prepacked, st)) return rc;
  if (shape == 1) return launch_c3<C3Bf16, 150, 2, 1, 1, 2, 2, false, false>(p, 0, st, "conv3_fwd_150_60");
  if (shape == 2) return launch_c3<C3Bf16, 60, 1, 2, 1, 4, 4, false, false>(p, 0, st, "conv3_fwd_60_60");
  return launch_c3<C3Bf16, 60, 4, 2, 1, 1, 2, false, true>(p, 0, st, "conv3_fwd_60_240_ps");
}

int conv3_dgrad_bf16(const float* Wc, const bf16* dY, int64_t lddy, bf16* dX, int64_t lddx, const bf16* acc, int64_t ldacc,
                     int in_act, const ConvGeom& g, float s, void* wpack, hipStream_t st) {
  Args p{};
  int shape;
  if (int rc = c3_dgrad_args(p, shape, dY, lddy, dX, lddx, acc, ldacc, in_act, g, s, wpack)) return rc;
  if (shape == 3 && lddy != 60) return RDST_ENOTSUP;   // sub-pixel pairs contiguous in dY
  if (int rc = C3Bf16::pack(Wc, reinterpret_cast<bf16*>(wpack), g.Cin, g.Cout, g.Cout, g.Cin, shape == 3 ? PK_DGRAD_UNSHUF : PK_DGRAD, s, st))
    return rc;
  if (shape == 1) {
    Args pa = p;
    if (int rc = launch_c3<C3Bf16, 60, 4, 1, 1, 1, 2, false, false>(pa, 0, st, "conv3_dgrad_60_150a")) return rc;
    return launch_c3<C3Bf16, 60, 1, 1, 1, 4, 4, false, false>(p, 4, st, "conv3_dgrad_60_150b");
  }
  if (shape == 2) return launch_c3<C3Bf16, 60, 1, 2, 1, 4, 4, false, false>(p, 0, st, "conv3_dgrad_60_60");
  return launch_c3<C3Bf16, 240, 2, 1, 2, 1, 2, true, false>(p, 0, st, "conv3_dgrad_240_60_unshuf");
}
