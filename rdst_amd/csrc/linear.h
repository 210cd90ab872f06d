// Hooks for the MFMA fast paths of K3 (linear_mfma.hip).  Each returns RDST_ENOTSUP when the shape
// or dtype is not covered, in which case linear.hip falls back to the generic functor GEMM.
// split (fp32 rows only): the RDST_F32X3 form of the kernels (common.h).
#pragma once
#include "common.h"

template <typename T>
int linear_fwd_mfma(const T* X, int64_t ldx, const float* ln_w, const float* ln_b, int in_act, const float* Wt,
                    const float* bias, const T* R, int64_t ldr, T* Y, int64_t ldy, float* stats, int64_t M, int K,
                    int N, float s, bool split, hipStream_t st);
// dA[M][K] = s * dY[M][N] @ Wt[N][K]; has_ln: write fp32 dA, else dX = dA*act'(X) (+dX)
template <typename T>
int linear_dgrad_mfma(const T* X, int64_t ldx, bool has_ln, int in_act, const float* Wt, const T* dY, int64_t lddy,
                      T* dX, int64_t lddx, const T* acc, int64_t ldacc, float* dA, int64_t M, int K, int N, float s,
                      bool split, hipStream_t st);
// dW[N][K] = s * dY^T f(X) and dbias[N] = s * colsum(dY) in one pass (either pointer may be NULL)
template <typename T>
int linear_wgrad_mfma(const T* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* stats, int in_act,
                      const T* dY, int64_t lddy, float* dW, float* dbias, const WsSlab& slab, int64_t M, int K, int N, float s,
                      bool split, hipStream_t st);

// ---- the backward workspace (rdst_ln_linear_bwd_workspace): [dA | G][slabW][small][spare] -------------------------------------
// slab: every kernel below that writes one slab row per workgroup takes its region as a WsSlab of this layout, caps its grid
// by the region's rows and asks rdst_slab_fits() before it launches.
constexpr int kLinWgradSplits = 96;   // split-K slices of the generic weight-gradient GEMM (gemm_valu.h)
// rows of slabW for a Linear of N outputs: one workgroup per CU, or up to four small ones for the narrow projections
inline int linear_wgrad_max_wgs(int N) { return N <= 128 ? 4 * kCUs : N <= 192 ? 2 * kCUs : kCUs; }
struct LinBwdWs {
  float* dA;      // [M][K] fp32 d(LayerNorm output) of the generic path (linear_dgrad_mfma, scale_to_f32 -> ln_bwd_rows); shares its floats with
  float* G;       // [N][K+1] LayerNorm-finish scratch of the fused paths (never both in one call); null where N (K + 1) > M K or without a LayerNorm
  WsSlab slabW;   // [N][K+1] fp32 (or bf16 G4) partials per workgroup: lin_wgrad_mfma, lnlin_bwd, lnlin3_bwd, lnlin3x_bwd; the generic GEMM's [N][K] slices
  WsSlab small;   // colsum rows [N]; [2][K] rows of ln_bwd_rows, ln8_bwd and lin_dgrad_ln
  size_t bytes;
};
// ln: a LayerNorm in front (dA is carved); linear: a weight (slabW is carved; false = LayerNorm only).  The size query asks
// for both, whatever the call then uses.
inline LinBwdWs lin_bwd_layout(void* base, int64_t M, int K, int N, bool ln, bool linear) {
  WsCarver c(base);
  LinBwdWs w{};
  const size_t g = (size_t)N * (K + 1), da = ln ? (size_t)M * K : 0;
  w.dA = c.take<float>(da);
  w.G = ln && linear && g <= da ? w.dA : nullptr;
  const int64_t rows = linear ? linear_wgrad_max_wgs(N) : 0;
  const size_t gen = linear ? (size_t)kLinWgradSplits * N * K : 0, per_wg = (size_t)rows * g;   // two users: the larger need
  w.slabW = WsSlab{c.take<float>(gen > per_wg ? gen : per_wg), rows, (int64_t)g};
  w.small = ws_take_slab(c, kSmallBlocks, N > 2 * K ? N : 2 * K);
  c.take<float>(2 * (size_t)K + kWsSlackFloats);   // spare: a reduced [2][K] row and the slack, as every release has reserved them
  w.bytes = c.bytes();
  return w;
}

// dgrad with the LayerNorm backward fused in (K <= 128): dX written/accumulated, d(gamma)/d(beta) partials in
// slab[*nslab][2][K] for the caller to reduce
template <typename T>
int linear_dgrad_ln_mfma(const T* X, int64_t ldx, const float* stats, const float* gamma, const float* Wt, const T* dY,
                         int64_t lddy, T* dX, int64_t lddx, const T* acc, int64_t ldacc, const WsSlab& slab, int* nslab,
                         int64_t M, int K, int N, float s, hipStream_t st);
// LayerNorm-fused Linear, weight-gradient side finishing the LayerNorm parameters too: the wgrad pass runs on
// x-hat, the reduction then forms dW = s (gamma G + beta db^T), dbias = s db, d(gamma)[k] = s sum_n W[n][k] G[n][k],
// d(beta)[k] = s sum_n W[n][k] db[n].  G: N*(K+1) floats of scratch.
template <typename T>
int linear_wgrad_ln_mfma(const T* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* stats, const float* Wt,
                         const T* dY, int64_t lddy, float* dW, float* dbias, float* dln_w, float* dln_b, const WsSlab& slab,
                         float* G, int64_t M, int K, int N, float s, bool split, hipStream_t st);
// dgrad + LayerNorm backward producing dX only, everything register resident (K <= 128)
template <typename T>
int linear_dgrad_ln2_mfma(const T* X, int64_t ldx, const float* stats, const float* gamma, const float* Wt, const T* dY,
                          int64_t lddy, T* dX, int64_t lddx, const T* acc, int64_t ldacc, int64_t M, int K, int N, float s,
                          bool split, hipStream_t st);
// finish of a LayerNorm-fused weight gradient from G (N, K+1) = [dY^T x-hat | colsum(dY)] (see linear_wgrad_ln_mfma)
int wgrad_ln_finish_launch(const float* G, const float* Wt, const float* ln_w, const float* ln_b, int N, int K, float s,
                           float* dW, float* dbias, float* dln_w, float* dln_b, hipStream_t st);
int wgrad_sum_launch(const float* slab, int nwg, int tot, float* G, hipStream_t st);
int wgrad_reduce_launch(const float* slab, int nwg, int N, int K, float s, float* dW, float* dbias, hipStream_t st);
// LayerNorm + Linear backward (dX, dW, dbias, d(gamma), d(beta)) in ONE pass over (x, dY): lnlin_mfma.hip, which tries ...
int linear_ln_bwd_fused_bf16(const bf16* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* stats,
                             const float* Wt, const bf16* dY, int64_t lddy, bf16* dX, int64_t lddx, const bf16* acc,
                             int64_t ldacc, float* dW, float* dbias, float* dln_w, float* dln_b, const WsSlab& slab, float* G,
                             int64_t M, int K, int N, float s, hipStream_t st, const bf16* acc2 = nullptr, int64_t ldacc2 = 0);
// ... its re-cut for the E1 shapes first (lnlin3_mfma.hip): dX and the per-workgroup bf16 G4 slabs (*grid_out of them, at
// most the region's rows; slab_stride in 8-byte groups) for the caller to reduce; RDST_ENOTSUP for everything else
int lnlin3_bwd_bf16(const bf16* X, int64_t ldx, const float* ln_w, const float* stats, const float* Wt, const bf16* dY,
                    int64_t lddy, bf16* dX, int64_t lddx, const bf16* acc, int64_t ldacc, const bf16* acc2, int64_t ldacc2,
                    const WsSlab& slab, int64_t slab_stride, int64_t M, int K, int N, int* grid_out, hipStream_t st);

// streaming forward for the E1 shapes, bf16 (lin3_mfma.hip); RDST_ENOTSUP for everything else.
// wpack: lin3_pack_bytes(K, N) bytes of 16-byte aligned device scratch (NULL -> RDST_ENOTSUP).
size_t lin3_pack_bytes(int K, int N);
int lin3_kind(int K, int N, bool ln, bool res, int in_act);   // 0 = not covered
int lin3_fwd_bf16(const bf16* X, int64_t ldx, const float* ln_w, const float* ln_b, int in_act, const float* Wt, const float* bias,
                  const bf16* R, int64_t ldr, bf16* Y, int64_t ldy, float* stats, int64_t M, int K, int N, float s, void* wpack,
                  bool prepacked, hipStream_t st);
int lin3_pack_launch(const float* W, const float* gamma, const float* beta, const float* bias, void* out, int N, int K, float s,
                     hipStream_t st);
// fused Mlp forward on the same skeleton (mlp3_mfma.hip): wpack = mlp3_pack_bytes(C, hid) bytes = [fc1 image][fc2 image]
size_t mlp3_pack_bytes(int C, int hid);
bool mlp3_fwd_shape(int C, int hid);   // hid = 2 C, C in {60, 90, 120}
int mlp3_fwd_bf16(const bf16* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* W1, const float* b1, const float* W2,
                  const float* b2, bf16* Y, int64_t ldy, float* stats, int64_t M, int C, int hid, void* wpack, bool prepacked,
                  hipStream_t st);

// the same streaming forward on fp32 rows in the RDST_F32X3 arithmetic (lin3x_mfma.hip); wpack: lin3x_pack_bytes(K, N) bytes (pack.h)
int lin3x_kind(int K, int N, bool ln, bool res, int in_act);   // 0 = not covered
int lin3x_fwd_f32(const float* X, int64_t ldx, const float* ln_w, const float* ln_b, int in_act, const float* Wt, const float* bias,
                  const float* R, int64_t ldr, float* Y, int64_t ldy, float* stats, int64_t M, int K, int N, float s, void* wpack,
                  bool prepacked, hipStream_t st);
int lin3x_pack_launch(const float* W, const float* gamma, const float* beta, const float* bias, void* out, int N, int K, float s,
                      hipStream_t st);
// one-pass Linear backward on fp32 rows in the RDST_F32X3 arithmetic (lnlin3x_mfma.hip): dX (+ LayerNorm backward / GELU' / addends), dW,
// dbias, d(gamma), d(beta); slab: slabW of lin_bwd_layout, G: N (K + 1) floats (LayerNorm only)
int lnlin3x_bwd_kind(int K, int N, bool ln, int in_act);   // 0 = not covered
int lnlin3x_bwd_f32(const float* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* stats, int in_act, const float* Wt,
                    const float* dY, int64_t lddy, float* dX, int64_t lddx, const float* acc, int64_t ldacc, const float* acc2,
                    int64_t ldacc2, float* dW, float* dbias, float* dln_w, float* dln_b, const WsSlab& slab, float* G, int64_t M, int K, int N,
                    float s, hipStream_t st);
