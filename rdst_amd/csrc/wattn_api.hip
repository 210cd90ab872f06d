// C-ABI entry points of the window-attention path (K1/K2), the route tables that say which kernel serves a call, and the
// deterministic d(table) reduction.
#include "common.h"
#include "wattn.h"
#include "reduce_batch.h"

thread_local char g_rdst_err[256] = {0};

extern "C" int rdst_abi_version(void) { return 11; }
extern "C" const char* rdst_last_error(void) { return g_rdst_err; }

// The backward workspace of rdst_wattn_bwd / _bwd_lse / _bwd_drop is one region: a partial d(table) [heads][T] per slab row, one
// row per window.  The kernels that write a row per window refuse fewer rows; the persistent ones cap their grid by them (k2_groups).
static WsSlab wattn_bwd_layout(void* base, int B, int H, int W, int heads, int ws) {
  WsCarver c(base);
  return ws_take_slab(c, (int64_t)B * (H / ws) * (W / ws), (int64_t)heads * (2 * ws - 1) * (2 * ws - 1));
}
extern "C" size_t rdst_wattn_bwd_workspace(int B, int H, int W, int C, int heads, int ws) {
  if (B <= 0 || H <= 0 || W <= 0 || ws <= 0 || heads <= 0) return 0;
  (void)C;
  const WsSlab s = wattn_bwd_layout(nullptr, B, H, W, heads, ws);
  return (size_t)s.rows * s.stride * sizeof(float);
}

namespace {

int make_geom(WinGeom& g, int B, int H, int W, int C, int heads, int ws, int shift, const float* mask, int mask_nw,
              const char* who) {
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || heads <= 0 || ws <= 0)
    return rdst_fail(RDST_EINVAL, "%s: non-positive dimension", who);
  if (C % heads) return rdst_fail(RDST_EINVAL, "%s: C=%d not divisible by heads=%d", who, C, heads);
  if (H % ws || W % ws) return rdst_fail(RDST_EINVAL, "%s: H=%d, W=%d must be multiples of the window size %d", who, H, W, ws);
  if (shift < 0 || shift >= ws) return rdst_fail(RDST_EINVAL, "%s: shift=%d must be in [0, ws=%d)", who, shift, ws);
  if ((int64_t)B * H * W >= (1ll << 31)) return rdst_fail(RDST_EINVAL, "%s: more than 2^31 tokens", who);
  g.B = B; g.H = H; g.W = W; g.C = C; g.heads = heads; g.ws = ws; g.shift = shift;
  g.nWh = H / ws; g.nWw = W / ws; g.N = ws * ws; g.T = (2 * ws - 1) * (2 * ws - 1);
  if (mask && mask_nw <= 0) return rdst_fail(RDST_EINVAL, "%s: mask given with mask_nw=%d", who, mask_nw);
  g.mask = mask; g.mask_nw = mask ? mask_nw : 1;
  g.pdrop = 0.f; g.seed = nullptr;
  return 0;
}

// What every window-attention entry point checks after its dtype, in this order: the geometry (-> g), the pointers, the
// leading dimensions (ld3: rows of 3C elements, ld1: rows of C), and for a backward (workspace_bytes given) the workspace.
constexpr size_t kNoWorkspace = ~(size_t)0;
int wattn_check_args(WinGeom& g, const char* who, int B, int H, int W, int C, int heads, int ws, int shift, const float* mask,
                     int mask_nw, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> ld3,
                     std::initializer_list<int64_t> ld1, size_t workspace_bytes = kNoWorkspace) {
  if (int rc = make_geom(g, B, H, W, C, heads, ws, shift, mask, mask_nw, who)) return rc;
  for (const void* q : ptrs)
    if (!q) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  bool small = false;
  for (int64_t l : ld3) small |= l < 3 * C;
  for (int64_t l : ld1) small |= l < C;
  if (small) return rdst_fail(RDST_EINVAL, "%s: leading dimension too small", who);
  if (workspace_bytes < rdst_wattn_bwd_workspace(B, H, W, C, heads, ws)) return rdst_fail(RDST_EINVAL, "%s: workspace too small", who);
  return 0;
}

// dtable[t * heads + h] = sum over the `rows` slab rows [heads][T] a backward kernel left, in fixed order
int wattn_sum_dtable(const float* slab, int rows, int heads, int T, float* dtable, hipStream_t st) {
  rbatch::SumJob sj{};
  sj.slab = slab; sj.nwg = rows; sj.stride = (int64_t)heads * T; sj.tot = heads * T; sj.map = rbatch::MAP_DTABLE;
  sj.out = dtable; sj.a = heads; sj.b = T;
  return rbatch::sum(sj, st);
}

// ---- which kernel serves rdst_wattn_fwd / rdst_wattn_bwd --------------------------------------------------------------------
// A call walks its table from the top and takes the first route of its dtype that does not pass (RDST_ENOTSUP); every other
// return value, an error included, ends the walk.  The ORDER IS THE POLICY: a route further up is the faster kernel wherever
// both accept a call, and each launcher alone knows what it accepts (shape, alignment, strides; see its file).
//   fp32 / fp32x3:  window 16 -> generic MFMA (ws 8; its split form for fp32x3) -> scalar
//   bf16 forward:   hd (ws 8, 6 heads of dim 10 / 15 / 20) -> window 16 -> generic MFMA (ws 8) -> scalar
//   bf16 backward:  pair (as hd, dense rows, head dims per RDST_K2_DMA) -> hd -> window 16 -> generic MFMA -> scalar
// The scalar kernels of wattn_v0.hip take everything, an explicit mask included.  Debug build only: `off` names an
// environment variable whose first character `offc` takes the route out, and RDST_DISABLE_MFMA=1 takes out all but the scalar one.
#ifndef RDST_K2_DMA
#define RDST_K2_DMA 6   // bit mask over the head dims 10 / 15 / 20 (1 / 2 / 4): which widths take the round-4 re-cut (wattn_bwd_pair.hip:
                        // LDS-DMA ring of section sets, loader / storer waves, passes T / N without the P / dS images).  It hides the row
                        // traffic but is VALU-bound by its recomputed key-tile pass.  Same box, cold, "K2 + table reduce" per call at
                        // C = 60 / 90 / 120: 77.6-80.7 / 78.9 / 78.8 us against 76.0 / 80.5 / 82.5 for the hd kernel; inside the step
                        // (rocprofv3, profiles/r04f_*, before the loaders' cheaper issue code) 65.7 / 69.9 / 69.1 against 64.6 / 70.0 / 72.7:
                        // C = 90 and C = 120 take it, C = 60 (where the old kernel's arithmetic is the cheaper one) does not
#endif
struct FwdCall {
  const void* qkv; int64_t ld; const float* table; void* out; int64_t ldo; const WinGeom& g; float scale; int dtype; bool split;
  hipStream_t st;
};
struct BwdCall {
  const void* qkv; int64_t ld; const float* table; const void* dout; int64_t ldd; void* dqkv; int64_t ldq;
  float* slab; int slab_rows; const WinGeom& g; float scale; int dtype; bool split; int* nslab; hipStream_t st;
};
constexpr int kAnyDtype = -1;
template <class Call>
struct Route {
  int dtype; bool mfma; int (*go)(const Call&); const char* off; char offc;   // row dtype (RDST_F32 covers fp32x3), a matrix-core kernel?
};

const Route<FwdCall> kFwdRoutes[] = {
    {RDST_F32, true, [](const FwdCall& c) { return wattn16_fwd_f32((const float*)c.qkv, c.ld, c.table, (float*)c.out, c.ldo, c.g, c.scale, c.st); }},
    {RDST_BF16, true, [](const FwdCall& c) { return wattn_fwd_mfma_hd(c.qkv, c.ld, c.table, c.out, c.ldo, c.g, c.scale, c.st); }, "RDST_K1_V1", '1'},
    {RDST_BF16, true, [](const FwdCall& c) { return wattn16_fwd_mfma(c.qkv, c.ld, c.table, c.out, c.ldo, c.g, c.scale, c.st); }},
    {kAnyDtype, true, [](const FwdCall& c) { return wattn_fwd_mfma(c.qkv, c.ld, c.table, c.out, c.ldo, c.g, c.scale, c.dtype, c.split, c.st); }},
    {kAnyDtype, false, [](const FwdCall& c) { return wattn_fwd_generic(c.qkv, c.ld, c.table, c.out, c.ldo, c.g, c.scale, c.dtype, c.st); }},
};

// (the scalar backward writes one slab row per window: *nslab = slab_rows, the number of windows)
#define RDST_BWD_ARGS(c) c.qkv, c.ld, c.table, c.dout, c.ldd, c.dqkv, c.ldq, c.slab, c.slab_rows, c.g, c.scale
int bwd_pair(const BwdCall& c) {
  const int d = c.g.heads == 6 && c.g.C % 6 == 0 ? c.g.C / 6 : 0;
  if (!(RDST_K2_DMA & (d == 10 ? 1 : d == 15 ? 2 : d == 20 ? 4 : 0))) return RDST_ENOTSUP;
  return wattn_bwd_pair(RDST_BWD_ARGS(c), c.nslab, c.st);
}
int bwd_scalar(const BwdCall& c) {
  *c.nslab = c.slab_rows;
  return wattn_bwd_generic(c.qkv, c.ld, c.table, c.dout, c.ldd, c.dqkv, c.ldq, c.slab, c.g, c.scale, c.dtype, c.st);
}
const Route<BwdCall> kBwdRoutes[] = {
    {RDST_F32, true, [](const BwdCall& c) {
       return wattn16_bwd_f32((const float*)c.qkv, c.ld, c.table, (const float*)c.dout, c.ldd, (float*)c.dqkv, c.ldq, c.slab,
                              c.slab_rows, c.g, c.scale, c.nslab, c.st);
     }},
    {RDST_BF16, true, bwd_pair, "RDST_K2_PAIR", '0'},
    {RDST_BF16, true, [](const BwdCall& c) { return wattn_bwd_mfma_hd(RDST_BWD_ARGS(c), c.nslab, c.st); }, "RDST_K2_V1", '1'},
    {RDST_BF16, true, [](const BwdCall& c) { return wattn16_bwd_mfma(RDST_BWD_ARGS(c), c.nslab, c.st); }},
    {kAnyDtype, true, [](const BwdCall& c) { return wattn_bwd_mfma(RDST_BWD_ARGS(c), c.dtype, c.split, c.nslab, c.st); }},
    {kAnyDtype, false, bwd_scalar},
};
#undef RDST_BWD_ARGS

template <class Call, size_t NR>
int wattn_route(const Route<Call> (&routes)[NR], const Call& c) {
  const bool no_mfma = mfma_disabled();
  for (const Route<Call>& r : routes) {
    if ((r.dtype != kAnyDtype && r.dtype != c.dtype) || (r.mfma && no_mfma)) continue;
    if (r.off) {
      const char* e = rdst_dbg_getenv(r.off);
      if (e && e[0] == r.offc) continue;
    }
    if (const int rc = r.go(c); rc != RDST_ENOTSUP) return rc;
  }
  return RDST_ENOTSUP;
}

}  // namespace

extern "C" int rdst_wattn_fwd(const void* qkv, int64_t ld_qkv, const float* table, const float* mask, int mask_nw,
                              void* out, int64_t ld_out, int B, int H, int W, int C, int heads, int ws, int shift,
                              float scale, int dtype, void* stream) {
  bool split;
  if (int rc = rdst_dtype(dtype, split, "rdst_wattn_fwd")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_wattn_fwd", B, H, W, C, heads, ws, shift, mask, mask_nw, {qkv, table, out}, {ld_qkv}, {ld_out}))
    return rc;
  return wattn_route(kFwdRoutes, FwdCall{qkv, ld_qkv, table, out, ld_out, g, scale, dtype, split, (hipStream_t)stream});
}

extern "C" int rdst_wattn_bwd(const void* qkv, int64_t ld_qkv, const float* table, const float* mask, int mask_nw,
                              const void* dout, int64_t ld_dout, void* dqkv, int64_t ld_dqkv, float* dtable,
                              void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int heads, int ws,
                              int shift, float scale, int dtype, void* stream) {
  bool split;
  if (int rc = rdst_dtype(dtype, split, "rdst_wattn_bwd")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_wattn_bwd", B, H, W, C, heads, ws, shift, mask, mask_nw,
                                {qkv, table, dout, dqkv, dtable, workspace}, {ld_qkv, ld_dqkv}, {ld_dout}, workspace_bytes))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const WsSlab slab = wattn_bwd_layout(workspace, B, H, W, heads, ws);
  int nslab = 0;   // slab rows written: one per persistent workgroup, or one per window
  if (int rc = wattn_route(kBwdRoutes, BwdCall{qkv, ld_qkv, table, dout, ld_dout, dqkv, ld_dqkv, slab.p, (int)slab.rows, g, scale,
                                               dtype, split, &nslab, st}))
    return rc;
  return wattn_sum_dtable(slab.p, nslab, heads, g.T, dtable, st);
}

// ---- K8: the attention half of a Swin block in one launch (swinattn_fwd.hip) ---------------------------------------------------
extern "C" int rdst_swin_attn_fwd_supported(int C, int heads, int ws, int dtype) {
  if (rdst_dtype(dtype, "rdst_swin_attn_fwd_supported")) return 0;
  return dtype == RDST_BF16 && swinattn_supported(C, heads, ws);
}
extern "C" size_t rdst_swin_attn_fwd_workspace(int C) { return C > 0 ? swinattn_pack_bytes(C) : 0; }
extern "C" int rdst_swin_attn_fwd(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, const float* Wqkv,
                                  const float* bqkv, const float* table, const float* Wproj, const float* bproj, void* qkv,
                                  int64_t ld_qkv, void* a, int64_t ld_a, void* x1, int64_t ld_x1, float* stats, void* workspace,
                                  size_t workspace_bytes, int B, int H, int W, int C, int heads, int ws, int shift, float scale,
                                  int dtype, void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_swin_attn_fwd")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_swin_attn_fwd", B, H, W, C, heads, ws, shift, nullptr, 0,
                                {X, ln_w, ln_b, Wqkv, table, Wproj, qkv, a, x1, stats, workspace}, {ld_qkv}, {ld_x, ld_a, ld_x1}))
    return rc;
  if (dtype != RDST_BF16) return RDST_ENOTSUP;
  const bool prepacked = workspace_bytes == RDST_PREPACKED;
  if (!prepacked && workspace_bytes < swinattn_pack_bytes(C)) return rdst_fail(RDST_EINVAL, "rdst_swin_attn_fwd: workspace too small");
  return swinattn_fwd_bf16((const bf16*)X, ld_x, ln_w, ln_b, Wqkv, bqkv, table, Wproj, bproj, (bf16*)qkv, ld_qkv, (bf16*)a, ld_a,
                           (bf16*)x1, ld_x1, stats, workspace, prepacked, g, scale, (hipStream_t)stream);
}

// ---- window attention with the forward's row statistics kept for the backward (window 16, bf16: wattn16_mfma.hip) ---------------
// nlse[token][head] = -(scale log2e max_j S'_ij + log2 sum_j exp(...)): with it and the forward's output the backward's first pass
// streams its key tiles (no row maximum / sum / normalisation / delta pass).  RDST_ENOTSUP for every shape the plain entry points
// serve with other kernels: the caller then uses rdst_wattn_fwd / rdst_wattn_bwd.
extern "C" int rdst_wattn_fwd_lse(const void* qkv, int64_t ld_qkv, const float* table, void* out, int64_t ld_out, float* nlse,
                                  int B, int H, int W, int C, int heads, int ws, int shift, float scale, int dtype, void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_wattn_fwd_lse")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_wattn_fwd_lse", B, H, W, C, heads, ws, shift, nullptr, 0, {qkv, table, out, nlse}, {ld_qkv}, {ld_out}))
    return rc;
  if (dtype != RDST_BF16) return RDST_ENOTSUP;
  return wattn16_fwd_mfma(qkv, ld_qkv, table, out, ld_out, g, scale, (hipStream_t)stream, nlse);
}

extern "C" int rdst_wattn_bwd_lse(const void* qkv, int64_t ld_qkv, const float* table, const void* dout, int64_t ld_dout,
                                  const void* out, int64_t ld_out, const float* nlse, void* dqkv, int64_t ld_dqkv, float* dtable,
                                  void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int heads, int ws,
                                  int shift, float scale, int dtype, void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_wattn_bwd_lse")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_wattn_bwd_lse", B, H, W, C, heads, ws, shift, nullptr, 0,
                                {qkv, table, dout, out, nlse, dqkv, dtable, workspace}, {ld_qkv, ld_dqkv}, {ld_dout, ld_out}, workspace_bytes))
    return rc;
  if (dtype != RDST_BF16) return RDST_ENOTSUP;
  hipStream_t st = (hipStream_t)stream;
  const WsSlab slab = wattn_bwd_layout(workspace, B, H, W, heads, ws);
  int nslab = 0;
  if (int rc = wattn16_bwd_mfma(qkv, ld_qkv, table, dout, ld_dout, dqkv, ld_dqkv, slab.p, (int)slab.rows, g, scale, &nslab, st, out,
                                ld_out, nlse))
    return rc;
  return wattn_sum_dtable(slab.p, nslab, heads, g.T, dtable, st);
}

// ---- attention dropout (WindowAttention.attn_drop > 0 in training, swin_transformer_sr.py:102,136): the generic kernels with
// a counter-based mask; `seed` is a DEVICE pointer to the call's 64-bit seed (drawn by the host from its generator: a HIP graph
// replay then sees a new seed without re-capturing); the backward must get the same attn_drop and seed as its forward.
namespace {
int drop_args(WinGeom& g, float attn_drop, const unsigned long long* seed, const char* who) {
  if (!(attn_drop >= 0.f && attn_drop < 1.f)) return rdst_fail(RDST_EINVAL, "%s: attn_drop=%g must be in [0, 1)", who, (double)attn_drop);
  if (attn_drop > 0.f && !seed) return rdst_fail(RDST_EINVAL, "%s: attn_drop > 0 needs a seed", who);
  g.pdrop = attn_drop;
  g.seed = attn_drop > 0.f ? seed : nullptr;
  return 0;
}
}  // namespace

extern "C" int rdst_wattn_fwd_drop(const void* qkv, int64_t ld_qkv, const float* table, const float* mask, int mask_nw,
                                   void* out, int64_t ld_out, int B, int H, int W, int C, int heads, int ws, int shift,
                                   float scale, int dtype, float attn_drop, const unsigned long long* seed, void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_wattn_fwd_drop")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_wattn_fwd_drop", B, H, W, C, heads, ws, shift, mask, mask_nw, {qkv, table, out}, {ld_qkv}, {ld_out}))
    return rc;
  if (int rc = drop_args(g, attn_drop, seed, "rdst_wattn_fwd_drop")) return rc;
  return wattn_fwd_generic(qkv, ld_qkv, table, out, ld_out, g, scale, dtype, (hipStream_t)stream);
}

extern "C" int rdst_wattn_bwd_drop(const void* qkv, int64_t ld_qkv, const float* table, const float* mask, int mask_nw,
                                   const void* dout, int64_t ld_dout, void* dqkv, int64_t ld_dqkv, float* dtable,
                                   void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int heads, int ws,
                                   int shift, float scale, int dtype, float attn_drop, const unsigned long long* seed,
                                   void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_wattn_bwd_drop")) return rc;
  WinGeom g;
  if (int rc = wattn_check_args(g, "rdst_wattn_bwd_drop", B, H, W, C, heads, ws, shift, mask, mask_nw,
                                {qkv, table, dout, dqkv, dtable, workspace}, {ld_qkv, ld_dqkv}, {ld_dout}, workspace_bytes))
    return rc;
  if (int rc = drop_args(g, attn_drop, seed, "rdst_wattn_bwd_drop")) return rc;
  hipStream_t st = (hipStream_t)stream;
  const WsSlab slab = wattn_bwd_layout(workspace, B, H, W, heads, ws);
  if (int rc = wattn_bwd_generic(qkv, ld_qkv, table, dout, ld_dout, dqkv, ld_dqkv, slab.p, g, scale, dtype, st)) return rc;
  return wattn_sum_dtable(slab.p, (int)slab.rows, heads, g.T, dtable, st);   // one slab row per (window, head) workgroup: [nwin][heads][T]
}

// The multipliers (0 or 1 / (1 - attn_drop)) the two entry points above apply: out[(window * heads + head)][N][N] floats
// (inspection and tests: the kernels never store the mask).
extern "C" int rdst_wattn_drop_mask(float* out, int B, int H, int W, int heads, int ws, float attn_drop,
                                    const unsigned long long* seed, void* stream) {
  if (!out || !seed || B <= 0 || H <= 0 || W <= 0 || heads <= 0 || ws <= 0 || H % ws || W % ws)
    return rdst_fail(RDST_EINVAL, "rdst_wattn_drop_mask: bad argument");
  if (!(attn_drop > 0.f && attn_drop < 1.f)) return rdst_fail(RDST_EINVAL, "rdst_wattn_drop_mask: attn_drop must be in (0, 1)");
  return wattn_drop_mask(out, (int64_t)B * (H / ws) * (W / ws) * heads, ws * ws, attn_drop, seed, (hipStream_t)stream);
}
