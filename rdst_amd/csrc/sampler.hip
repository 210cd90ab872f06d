// Training batches cut and degraded on the device (rdst_amd/data.py): the bicubic resize of the reference's datasets
// (datasets/basic_dataset.py:65-123, cv2.resize(INTER_CUBIC) on float images) and the batch of
// BasicMultiSRTrain.__getitem__ (datasets/basic_dataset.py:190-217: one random HR crop per slice, SingleImageRandomCrop
// :482-499, and the resize of every crop down to the LR patch), which the reference builds on the CPU in DataLoader
// workers and copies to the device (models/trans_sr_trainer.py:116-121, :143).
//
// The resize is separable with four taps per axis (Keys kernel, a = -0.75, half-pixel mapping, tap indices clamped to
// the image, no antialiasing, no clamping of the values).  Tap indices and weights of an axis come from a table the host
// computed in float64 and rounded once to fp32 (rdst_amd.data.tap_table); at hp = 4 lp the taps of an LR pixel are its
// own 4 x 4 group of HR pixels with the weights -3/32, 19/32, 19/32, -3/32, which the fast path of the sampler uses
// without a table.  Every output of both entry points is formed by tap4() below: horizontal sums of the four tap rows
// first, then the vertical sum, taps in ascending order, one explicit fmaf per tap.  So a patch resized by the sampler
// equals the same patch resized by rdst_resize_bicubic bit for bit, on either path.
//
// Bandwidth kernels: no MFMA, no atomics, no scratch.  Crop origins are arbitrary, so source rows are only 4-byte
// aligned: they are read as four dwords at alignment 4 (one global_load_dwordx4 where the compiler can, which the
// hardware accepts at dword alignment); the HR and LR outputs are written with aligned 16-byte stores where
// hp % 4 == 0.
//
// rdst_sample_patches_d8 is the same batch with patch b cut, then turned by T_k (k = variant[b] & 7, the numbering of
// rdst_unfold_tiles_d8 / tiling.dihedral), then degraded: the LR patch is the resize of the TURNED HR patch, formed by the
// same tap4() chains over the turned rows and columns (the chain is not flip invariant in fp32, so resizing first and turning
// afterwards would give other bits).  Reads run with lanes along a source row and stores with lanes along an output row: a
// flipped row is a reversed run, and the four transposed variants pass through 32 x 32 LDS blocks with rows of 33 floats.
//
// Both sampler entry points share one host plan (sample_tap4).  At hp = 4 lp they have a kernel each, two designs (a thread
// per 4 x 4 group; a workgroup per 32 x 32 block through LDS); at any other ratio one kernel source, sample_tab_kernel<V4, D8>,
// whose D8 == false instantiation has no turn in it.  The argument checks are tap_host.h's, f4 and clampi tapk.h's.
#include "tap_host.h"
#include "tapk.h"

namespace {

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at dword alignment
struct __attribute__((packed, aligned(1))) u8x4 { uint32_t v; };     // four label bytes at any address

// one output value from four taps, in ascending order with one rounding per tap
__device__ __forceinline__ float tap4(float v0, float v1, float v2, float v3, float w0, float w1, float w2, float w3) {
  return fmaf(w3, v3, fmaf(w2, v2, fmaf(w1, v1, __fmul_rn(w0, v0))));
}

// ---- rdst_resize_bicubic: one thread per output pixel ----------------------------------------------------------------
__global__ void __launch_bounds__(NT) resize_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W, int oh,
                                                    int ow, const int4* __restrict__ iy, const f4* __restrict__ wy,
                                                    const int4* __restrict__ ix, const f4* __restrict__ wx, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % ow);
  const int64_t t = i / ow;
  const int oy = (int)(t % oh);
  const int64_t plane = t / oh;
  int4 jx = ix[ox], jy = iy[oy];
  const f4 fx = wx[ox], fy = wy[oy];
  // the tables are the caller's: an index outside the image must not become an address
  jx.x = clampi(jx.x, 0, W - 1), jx.y = clampi(jx.y, 0, W - 1), jx.z = clampi(jx.z, 0, W - 1), jx.w = clampi(jx.w, 0, W - 1);
  jy.x = clampi(jy.x, 0, H - 1), jy.y = clampi(jy.y, 0, H - 1), jy.z = clampi(jy.z, 0, H - 1), jy.w = clampi(jy.w, 0, H - 1);
  const float* p = x + plane * H * W;
  const float* r0 = p + (int64_t)jy.x * W;
  const float* r1 = p + (int64_t)jy.y * W;
  const float* r2 = p + (int64_t)jy.z * W;
  const float* r3 = p + (int64_t)jy.w * W;
  const float h0 = tap4(r0[jx.x], r0[jx.y], r0[jx.z], r0[jx.w], fx.x, fx.y, fx.z, fx.w);
  const float h1 = tap4(r1[jx.x], r1[jx.y], r1[jx.z], r1[jx.w], fx.x, fx.y, fx.z, fx.w);
  const float h2 = tap4(r2[jx.x], r2[jx.y], r2[jx.z], r2[jx.w], fx.x, fx.y, fx.z, fx.w);
  const float h3 = tap4(r3[jx.x], r3[jx.y], r3[jx.z], r3[jx.w], fx.x, fx.y, fx.z, fx.w);
  y[i] = tap4(h0, h1, h2, h3, fy.x, fy.y, fy.z, fy.w);
}

// the window of patch b, clamped into the stack (the index table is device memory nobody checked)
struct Window {
  int64_t slice;
  int top, left;
};
__device__ __forceinline__ Window window_of(const int* __restrict__ index, int b, int S, int H, int W, int hp) {
  Window w;
  w.slice = clampi(index[3 * b], 0, S - 1);
  w.top = clampi(index[3 * b + 1], 0, H - hp);
  w.left = clampi(index[3 * b + 2], 0, W - hp);
  return w;
}

// ---- rdst_sample_patches, hp = 4 lp: one thread per LR pixel = per 4 x 4 group of HR pixels --------------------------
__global__ void __launch_bounds__(NT) sample4_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ labels,
                                                     const int* __restrict__ index, float* __restrict__ hr,
                                                     float* __restrict__ lr, uint8_t* __restrict__ lab, int S, int C, int H,
                                                     int W, int lp, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int hp = 4 * lp;
  const int ox = (int)(i % lp);
  int64_t t = i / lp;
  const int oy = (int)(t % lp);
  t /= lp;
  const int c = (int)(t % C);
  const int b = (int)(t / C);
  const Window w = window_of(index, b, S, H, W, hp);
  const float* src = stack + ((w.slice * C + c) * H + w.top + 4 * oy) * W + w.left + 4 * ox;
  float* dst = hr + (((int64_t)b * C + c) * hp + 4 * oy) * hp + 4 * ox;
  constexpr float K0 = -3.f / 32.f, K1 = 19.f / 32.f;
  float h[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f4 v = *reinterpret_cast<const f4u*>(src + (int64_t)j * W);
    *reinterpret_cast<f4*>(dst + (int64_t)j * hp) = v;
    h[j] = tap4(v.x, v.y, v.z, v.w, K0, K1, K1, K0);
  }
  lr[i] = tap4(h[0], h[1], h[2], h[3], K0, K1, K1, K0);
  if (labels != nullptr && c == 0) {
    const uint8_t* ls = labels + (w.slice * H + w.top + 4 * oy) * W + w.left + 4 * ox;
    uint8_t* ld = lab + ((int64_t)b * hp + 4 * oy) * hp + 4 * ox;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<uint32_t*>(ld + (int64_t)j * hp) = reinterpret_cast<const u8x4*>(ls + (int64_t)j * W)->v;
  }
}

// band `band` of nb: its LR rows [o0, o1), the HR rows it stages [tap_lo, tap_hi), owns [own_lo, own_hi) and walks [row_lo,
// row_hi)
struct Band {
  int o0, o1, tap_lo, tap_hi, own_lo, own_hi, row_lo, row_hi;
};
__device__ __forceinline__ Band band_of(const int4* __restrict__ it, int band, int nb, int LB, int hp, int lp, int max_rows) {
  Band d;
  d.o0 = band * LB, d.o1 = min(d.o0 + LB, lp);
  d.tap_lo = clampi(it[d.o0].x, 0, hp - 1);
  d.tap_hi = min(max(clampi(it[d.o1 - 1].w, 0, hp - 1) + 1, d.tap_lo + 1), d.tap_lo + max_rows);
  d.own_lo = band == 0 ? 0 : d.tap_lo;
  d.own_hi = band == nb - 1 ? hp : max(clampi(it[d.o1].x, 0, hp - 1), d.own_lo);
  d.row_lo = min(d.own_lo, d.tap_lo), d.row_hi = max(d.own_hi, d.tap_hi);
  return d;
}

// the LR rows [o0, o1) of one plane from the staged rows [tap_lo, tap_lo + staged) of its HR patch (tile: rows of hp floats)
__device__ __forceinline__ void lr_rows_from_tile(const float* tile, float* out, int hp, int lp, int o0, int o1, int tap_lo,
                                                  int staged, const int4* it, const f4* wt) {
  for (int e = threadIdx.x; e < (o1 - o0) * lp; e += NT) {
    const int oy = o0 + e / lp, ox = e % lp;
    const int4 jx = it[ox], jy = it[oy];
    const f4 fx = wt[ox], fy = wt[oy];
    const int x0 = clampi(jx.x, 0, hp - 1), x1 = clampi(jx.y, 0, hp - 1), x2 = clampi(jx.z, 0, hp - 1), x3 = clampi(jx.w, 0, hp - 1);
    // (a well-formed table keeps every tap row inside the staged rows; the clamp is for the other kind)
    const float* r0 = tile + clampi(clampi(jy.x, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float* r1 = tile + clampi(clampi(jy.y, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float* r2 = tile + clampi(clampi(jy.z, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float* r3 = tile + clampi(clampi(jy.w, 0, hp - 1) - tap_lo, 0, staged - 1) * hp;
    const float h0 = tap4(r0[x0], r0[x1], r0[x2], r0[x3], fx.x, fx.y, fx.z, fx.w);
    const float h1 = tap4(r1[x0], r1[x1], r1[x2], r1[x3], fx.x, fx.y, fx.z, fx.w);
    const float h2 = tap4(r2[x0], r2[x1], r2[x2], r2[x3], fx.x, fx.y, fx.z, fx.w);
    const float h3 = tap4(r3[x0], r3[x1], r3[x2], r3[x3], fx.x, fx.y, fx.z, fx.w);
    out[(int64_t)oy * lp + ox] = tap4(h0, h1, h2, h3, fy.x, fy.y, fy.z, fy.w);
  }
}

// ---- rdst_sample_patches_d8 --------------------------------------------------------------------------------------------------
// T_k(x)[i][j] = x[a][b] with (a, b) = (j, i) if k & 4 else (i, j), then a = hp - 1 - a if k & 2, b = hp - 1 - b if k & 1.  The
// output rows follow the source rows (the source columns if transposed) and the output columns the other axis:
struct Turn {
  bool tr, frow, fcol;   // transposed; the output rows / the output columns run against their source axis
};
__device__ __forceinline__ Turn turn_of(const int* __restrict__ variant, int b) {
  const int k = variant[b] & 7;   // device memory nobody checked, as the origins are
  Turn t;
  t.tr = k & 4;
  t.frow = t.tr ? (k & 1) : (k & 2), t.fcol = t.tr ? (k & 2) : (k & 1);
  return t;
}

constexpr int TB = 32;         // the turned patch is handled in TB x TB blocks, partial at the far edges
constexpr int TBP = TB + 1;    // the padded LDS row of floats (tools/lds_banks.py: d8 blocks)
constexpr int TBL = TB + 4;    // the LDS row of label bytes (rows stay 4-byte aligned)
constexpr int BLK_BYTES = TB * TBP * (int)sizeof(float) + TB * TBL;

__device__ __forceinline__ f4 reversed(f4 v) {
  f4 r;
  r.x = v.w, r.y = v.z, r.z = v.y, r.w = v.x;
  return r;
}

// hp = 4 lp, 16-byte flavour: one workgroup per (patch, channel, TB x TB block of the OUTPUT patch), blockIdx.x =
// ((b * C + c) * nbk + block row) * nbk + block column, nbk = ceil(hp / TB).  The source block is read once, lanes along its
// rows, four pixels per lane, into LDS; then thread (r, q) forms the four output pixels 4 q .. 4 q + 3 of output row r, which
// are the taps of one horizontal sum, and one wave adds the four sums of every LR pixel of the block: the chains of
// sample4_kernel over the turned patch.
__global__ void __launch_bounds__(NT) sample4_d8_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ labels,
                                                        const int* __restrict__ index, const int* __restrict__ variant,
                                                        float* __restrict__ hr, float* __restrict__ lr, uint8_t* __restrict__ lab,
                                                        int S, int C, int H, int W, int lp, int nbk) {
  __shared__ float blk[TB][TBP];
  __shared__ float hs[TB][TB / 4 + 2];   // the horizontal sums; rows of 10: the four rows of an LR pixel's column sum 8 banks apart
  __shared__ __attribute__((aligned(4))) uint8_t lblk[TB][TBL];
  const int hp = 4 * lp;
  int64_t t = blockIdx.x;
  const int j0 = (int)(t % nbk) * TB;
  t /= nbk;
  const int i0 = (int)(t % nbk) * TB;
  t /= nbk;
  const int c = (int)(t % C);
  const int b = (int)(t / C);
  const Window w = window_of(index, b, S, H, W, hp);
  const Turn u = turn_of(variant, b);
  const int ni = min(TB, hp - i0), nj = min(TB, hp - j0);            // output rows [i0, i0 + ni), columns [j0, j0 + nj)
  const int oi = u.frow ? hp - i0 - ni : i0, oj = u.fcol ? hp - j0 - nj : j0;
  const int a0 = u.tr ? oj : oi, b0 = u.tr ? oi : oj;               // the source block: rows from a0, columns from b0
  const int na = u.tr ? nj : ni, nbw = u.tr ? ni : nj;              // (all multiples of four: hp % 4 == 0)
  const bool with_labels = labels != nullptr && c == 0;
  const int r = threadIdx.x / (TB / 4), q = threadIdx.x % (TB / 4), q0 = 4 * q;
  if (r < na && q0 < nbw) {
    const int64_t at = (w.top + a0 + r) * (int64_t)W + w.left + b0 + q0;
    const f4 v = *reinterpret_cast<const f4u*>(stack + (w.slice * C + c) * H * W + at);
    blk[r][q0] = v.x, blk[r][q0 + 1] = v.y, blk[r][q0 + 2] = v.z, blk[r][q0 + 3] = v.w;
    if (with_labels) *reinterpret_cast<uint32_t*>(&lblk[r][q0]) = reinterpret_cast<const u8x4*>(labels + w.slice * H * W + at)->v;
  }
  __syncthreads();
  constexpr float K0 = -3.f / 32.f, K1 = 19.f / 32.f;
  if (r < ni && q0 < nj) {
    const int lr_ = u.frow ? ni - 1 - r : r;
    float v[4];
    uint32_t lv = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int lc = u.fcol ? nj - 1 - (q0 + e) : q0 + e;
      v[e] = u.tr ? blk[lc][lr_] : blk[lr_][lc];
      if (with_labels) lv |= (uint32_t)(u.tr ? lblk[lc][lr_] : lblk[lr_][lc]) << (8 * e);
    }
    f4 o;
    o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
    *reinterpret_cast<f4*>(hr + (((int64_t)b * C + c) * hp + i0 + r) * hp + j0 + q0) = o;
    if (with_labels) *reinterpret_cast<uint32_t*>(lab + ((int64_t)b * hp + i0 + r) * hp + j0 + q0) = lv;
    hs[r][q] = tap4(v[0], v[1], v[2], v[3], K0, K1, K1, K0);
  }
  __syncthreads();
  if (threadIdx.x < (TB / 4) * (TB / 4)) {
    const int oy = threadIdx.x / (TB / 4), ox = threadIdx.x % (TB / 4);
    if (4 * oy < ni && 4 * ox < nj)
      lr[(((int64_t)b * C + c) * lp + i0 / 4 + oy) * lp + j0 / 4 + ox] =
          tap4(hs[4 * oy][ox], hs[4 * oy + 1][ox], hs[4 * oy + 2][ox], hs[4 * oy + 3][ox], K0, K1, K1, K0);
  }
}

// ---- rdst_sample_patches and rdst_sample_patches_d8, any ratio: one workgroup per (patch, channel, band of LB rows of the LR
// patch) ------------------------------------------------------------------------------------------------------------------
// The bands partition the rows of the HR patch: band k owns the rows from the first tap row of its first LR row up to the
// first tap row of the next band (band 0 from row 0, the last band to row hp - 1).  A workgroup walks the rows it owns and
// the tap rows of its LR rows once: an owned row goes to the HR output, a tap row into the LDS tile, most rows both, from one
// load.  The tap rows a band shares with the next one (three at most when shrinking) are read by both, from the L2.  Then
// the LR rows are formed from the tile.  V4: hp % 4 == 0 and 16-byte aligned outputs, four pixels per lane and access.
// D8: the rows are those of the TURNED patch.  A flip-only variant walks them as the plain kernel does, each from the source
// row and the run of columns it mirrors.  A transposed variant covers the rows it walks with TB x TB blocks: a block of source
// rows is read with lanes along them into LDS (behind the tile: all LDS is dynamic, so the tile keeps its 16-byte base) and
// written out with lanes along the output rows, to the HR output, the tile, or both.  Without D8 `variant` is not read, and
// the turn, the mirrored addresses and the transposed branch are not compiled.
template <bool V4, bool D8>
__global__ void __launch_bounds__(NT) sample_tab_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ labels,
                                                        const int* __restrict__ index, const int* __restrict__ variant,
                                                        float* __restrict__ hr, float* __restrict__ lr,
                                                        uint8_t* __restrict__ lab, int S, int C, int H, int W, int hp, int lp,
                                                        const int4* __restrict__ it, const f4* __restrict__ wt, int LB, int nb,
                                                        int max_rows) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [max_rows][hp]; D8: then blk [TB][TBP], then lblk [TB][TBL]
  float(*blk)[TBP] = reinterpret_cast<float(*)[TBP]>(tile + max_rows * hp);
  uint8_t(*lblk)[TBL] = reinterpret_cast<uint8_t(*)[TBL]>(blk + TB);
  const int band = (int)(blockIdx.x % (unsigned)nb);
  const int plane = (int)(blockIdx.x / (unsigned)nb);
  const int c = plane % C, b = plane / C;
  const Window w = window_of(index, b, S, H, W, hp);
  Turn u = {false, false, false};   // (constants without D8: the mirrored addresses below fold to the plain ones)
  if constexpr (D8) u = turn_of(variant, b);
  const Band bd = band_of(it, band, nb, LB, hp, lp, max_rows);
  const float* src = stack + ((w.slice * C + c) * H + w.top) * W + w.left;
  float* dst = hr + ((int64_t)b * C + c) * hp * hp;
  const uint8_t* ls = labels != nullptr && c == 0 ? labels + (w.slice * H + w.top) * W + w.left : nullptr;
  uint8_t* ld = lab + (int64_t)b * hp * hp;
  constexpr int V = V4 ? 4 : 1;
  if (!u.tr) {
    const int per_row = hp / V;
    for (int e = threadIdx.x; e < (bd.row_hi - bd.row_lo) * per_row; e += NT) {
      const int r = bd.row_lo + e / per_row, col = (e % per_row) * V;
      const bool own = r >= bd.own_lo && r < bd.own_hi, tap = r >= bd.tap_lo && r < bd.tap_hi;
      if (!own && !tap) continue;
      const int64_t at = (int64_t)(u.frow ? hp - 1 - r : r) * W + (u.fcol ? hp - V - col : col);
      if (V4) {
        f4 v = *reinterpret_cast<const f4u*>(src + at);
        if (u.fcol) v = reversed(v);
        if (own) *reinterpret_cast<f4*>(dst + (int64_t)r * hp + col) = v;
        if (tap) *reinterpret_cast<f4*>(tile + (r - bd.tap_lo) * hp + col) = v;
        if (own && ls != nullptr) {
          const uint32_t lv = reinterpret_cast<const u8x4*>(ls + at)->v;
          *reinterpret_cast<uint32_t*>(ld + (int64_t)r * hp + col) = u.fcol ? __builtin_bswap32(lv) : lv;
        }
      } else {
        const float v = src[at];
        if (own) dst[(int64_t)r * hp + col] = v;
        if (tap) tile[(r - bd.tap_lo) * hp + col] = v;
        if (own && ls != nullptr) ld[(int64_t)r * hp + col] = ls[at];
      }
    }
  } else if constexpr (D8) {
    constexpr int TPR = TB / V;   // threads along an output row
    const int cc = threadIdx.x % TB, q0 = (int)(threadIdx.x % TPR) * V;
    for (int i0 = bd.row_lo; i0 < bd.row_hi; i0 += TB) {
      const int ni = min(TB, bd.row_hi - i0);                 // output rows [i0, i0 + ni) = source columns from b0
      const int b0 = u.frow ? hp - i0 - ni : i0;
      for (int j0 = 0; j0 < hp; j0 += TB) {
        const int nj = min(TB, hp - j0);                      // output columns [j0, j0 + nj) = source rows from a0
        const int a0 = u.fcol ? hp - j0 - nj : j0;
        if (cc < ni) {
          for (int rr = threadIdx.x / TB; rr < nj; rr += NT / TB) {
            const int64_t at = (int64_t)(a0 + rr) * W + b0 + cc;
            blk[rr][cc] = src[at];
            if (ls != nullptr) lblk[rr][cc] = ls[at];
          }
        }
        __syncthreads();
        if (q0 < nj) {   // (nj % V == 0: V == 4 only when hp % 4 == 0)
          for (int r = threadIdx.x / TPR; r < ni; r += NT / TPR) {
            const int i = i0 + r;
            const bool own = i >= bd.own_lo && i < bd.own_hi, tap = i >= bd.tap_lo && i < bd.tap_hi;
            if (!own && !tap) continue;
            const int lr_ = u.frow ? ni - 1 - r : r;
            float v[V];
            uint32_t lv = 0;
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const int lc = u.fcol ? nj - 1 - (q0 + e) : q0 + e;
              v[e] = blk[lc][lr_];
              if (ls != nullptr) lv |= (uint32_t)lblk[lc][lr_] << (8 * e);
            }
            if constexpr (V4) {
              f4 o;
              o.x = v[0], o.y = v[1], o.z = v[2], o.w = v[3];
              if (own) *reinterpret_cast<f4*>(dst + (int64_t)i * hp + j0 + q0) = o;
              if (tap) *reinterpret_cast<f4*>(tile + (i - bd.tap_lo) * hp + j0 + q0) = o;
              if (own && ls != nullptr) *reinterpret_cast<uint32_t*>(ld + (int64_t)i * hp + j0 + q0) = lv;
            } else {
              if (own) dst[(int64_t)i * hp + j0 + q0] = v[0];
              if (tap) tile[(i - bd.tap_lo) * hp + j0 + q0] = v[0];
              if (own && ls != nullptr) ld[(int64_t)i * hp + j0 + q0] = (uint8_t)lv;
            }
          }
        }
        __syncthreads();   // the next block overwrites blk
      }
    }
  }
  __syncthreads();
  lr_rows_from_tile(tile, lr + ((int64_t)b * C + c) * lp * lp, hp, lp, bd.o0, bd.o1, bd.tap_lo, bd.tap_hi - bd.tap_lo, it, wt);
}

}  // namespace

extern "C" int rdst_resize_bicubic(const float* x, float* y, int N, int C, int H, int W, int oh, int ow,
                                   const int32_t* tap_index_y, const float* tap_weight_y, const int32_t* tap_index_x,
                                   const float* tap_weight_x, void* stream) {
  const char* who = "rdst_resize_bicubic";
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d H=%d W=%d -> %d x %d", who, N, C, H, W, oh, ow);
  if (!x || !y || !tap_index_y || !tap_weight_y || !tap_index_x || !tap_weight_x)
    return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if (!rdst_aligned(16, {tap_index_y, tap_weight_y, tap_index_x, tap_weight_x}, {}))
    return rdst_fail(RDST_EINVAL, "%s: the tap tables must be 16-byte aligned", who);
  const int64_t total = (int64_t)N * C * oh * ow;
  const int64_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: %lld output pixels are too many for one launch", who, (long long)total);
  hipLaunchKernelGGL(resize_kernel, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, y, H, W, oh, ow,
                     (const int4*)tap_index_y, (const f4*)tap_weight_y, (const int4*)tap_index_x, (const f4*)tap_weight_x,
                     total);
  return rdst_launch_status(who);
}

namespace {

// LB LR rows per band: the largest power of two whose tap rows, (LB - 1) hp / lp + 5 at most, fit a tile of `budget` bytes
// (0 if not even one row's do)
int band_rows(int hp, int lp, int budget, int* max_rows) {
  for (int LB = 32; LB >= 1; LB >>= 1) {
    *max_rows = (int)(((int64_t)(LB - 1) * hp + lp - 1) / lp) + 5;
    if (*max_rows > hp) *max_rows = hp;
    if ((int64_t)*max_rows * hp * (int64_t)sizeof(float) <= budget) return LB;
  }
  return 0;
}

// rdst_sample_patches (variant == nullptr) and rdst_sample_patches_d8 behind their argument checks: one plan, one launch
int sample_tap4(const char* who, const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant, float* hr,
                float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp, const int32_t* tap_index,
                const float* tap_weight, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const bool d8 = variant != nullptr;
  const bool wide = hp % 4 == 0 && rdst_aligned(16, {hr}, {}) && rdst_aligned(4, {label_out}, {});
  if (hp == 4 * lp && wide) {
    if (d8) {
      const int nbk = (hp + TB - 1) / TB;
      const int64_t blocks = (int64_t)B * C * nbk * nbk;
      if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: B=%d C=%d hp=%d is too large for one launch", who, B, C, hp);
      hipLaunchKernelGGL(sample4_d8_kernel, dim3((unsigned)blocks), dim3(NT), 0, st, stack, labels, index, variant, hr, lr,
                         label_out, S, C, H, W, lp, nbk);
    } else {
      const int64_t total = (int64_t)B * C * lp * lp;
      hipLaunchKernelGGL(sample4_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, stack, labels, index, hr, lr,
                         label_out, S, C, H, W, lp, total);
    }
    return rdst_launch_status(who);
  }
  if (!tap_index || !tap_weight) return rdst_fail(RDST_EINVAL, "%s: hp=%d lp=%d needs the tap table", who, hp, lp);
  if (!rdst_aligned(16, {tap_index, tap_weight}, {})) return rdst_fail(RDST_EINVAL, "%s: the tap table must be 16-byte aligned", who);
  const int blk_bytes = d8 ? BLK_BYTES : 0;   // the transposing block shares the dynamic LDS
  int max_rows = 0;
  const int LB = band_rows(hp, lp, LDS_BUDGET - blk_bytes, &max_rows);
  if (LB < 1) return rdst_fail(RDST_ENOTSUP, "%s: hp=%d is wider than the table path's tile holds", who, hp);
  const int nb = (lp + LB - 1) / LB;
  const int smem = max_rows * hp * (int)sizeof(float) + blk_bytes;
  const unsigned grid = (unsigned)((int64_t)B * C * nb);
  auto launch = [&](auto kern) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), smem, st, stack, labels, index, variant, hr, lr, label_out, S, C, H, W, hp, lp,
                       (const int4*)tap_index, (const f4*)tap_weight, LB, nb, max_rows);
  };
  if (!d8) wide ? launch(sample_tab_kernel<true, false>) : launch(sample_tab_kernel<false, false>);
  else wide ? launch(sample_tab_kernel<true, true>) : launch(sample_tab_kernel<false, true>);
  return rdst_launch_status(who);
}

}  // namespace

extern "C" int rdst_sample_patches(const float* stack, const uint8_t* labels, const int32_t* index, float* hr, float* lr,
                                   uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp,
                                   const int32_t* tap_index, const float* tap_weight, void* stream) {
  const char* who = "rdst_sample_patches";
  if (int rc = sample_refusal(who, stack, labels, index, hr, lr, label_out, S, C, H, W, B, hp, lp)) return rc;
  return sample_tap4(who, stack, labels, index, nullptr, hr, lr, label_out, S, C, H, W, B, hp, lp, tap_index, tap_weight, stream);
}

extern "C" int rdst_sample_patches_d8(const float* stack, const uint8_t* labels, const int32_t* index, const int32_t* variant,
                                      float* hr, float* lr, uint8_t* label_out, int S, int C, int H, int W, int B, int hp, int lp,
                                      const int32_t* tap_index, const float* tap_weight, void* stream) {
  const char* who = "rdst_sample_patches_d8";
  if (int rc = sample_refusal(who, stack, labels, index, hr, lr, label_out, S, C, H, W, B, hp, lp)) return rc;
  if (!variant) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  return sample_tap4(who, stack, labels, index, variant, hr, lr, label_out, S, C, H, W, B, hp, lp, tap_index, tap_weight, stream);
}
