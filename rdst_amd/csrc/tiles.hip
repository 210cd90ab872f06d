// Tiled whole-slice inference (rdst_amd/tiling.py): the reference's ImageFolder / UnFolder / Folder
// (datasets/basic_dataset.py:347-449, wired up per scale in datasets/OASIS_dataset.py:246-271).  The reference unfolds an LR
// slice into overlapping fixed-size patches with nn.Unfold (pad + im2col + a transposed copy), runs the network on them and
// folds the SR patches back with nn.Fold (a transposed copy + col2im) times a precomputed reciprocal divisor image.  Here each
// direction is one launch:
//
//   unfold  one thread per (up to four) tile pixels: the tile pixel's own source pixel, zero or the clamped edge outside the
//           image, zeros in the slots past the last tile.  A pure copy.
//   fold    one thread per (up to four) output pixels: the covering tile pixels are gathered and summed in ascending tile
//           row, then ascending tile column, and the sum is multiplied once by 1.0f / (float)count.  The count is the number
//           of covering tiles, which the thread knows from its loop bounds: no divisor image is stored or read, nothing is
//           scattered, so there are no atomics and every run gives the same bits.
//
// Along an axis of n pixels with (patch, stride, pad, L), tile t covers the padded coordinates [t stride, t stride + patch)
// and pixel o sits at o + pad; the tiles that cover it are t in [ceil((o + pad - patch + 1) / stride), (o + pad) / stride]
// cut to [0, L - 1].  The entry points refuse every plan that leaves that range empty for some pixel, so `count` >= 1.
//
// Bandwidth kernels: no MFMA, no atomics, no scratch.  Tile origins are arbitrary, so source runs are only 4-byte aligned:
// four pixels that stay inside one row are read as four dwords at alignment 4 (one global_load_dwordx4, which the hardware
// accepts at dword alignment); outputs are written with aligned 16-byte stores where the row length and the base allow.
//
// The x8 geometric self-ensemble (SRTester(self_ensemble=True)) adds one launch in each direction.  The eight transforms of a
// square p x p tile are numbered k = 0..7:  T_k(x)[i][j] = x[a][b]  with (a, b) = (j, i) if k & 4, else (i, j); then
// a = p - 1 - a if k & 2 and b = p - 1 - b if k & 1  (flip the columns, flip the rows, then transpose).
//
//   unfold_d8  one block per 32 x 32 block of a tile: the block is read once (the pad rule applied) into a padded LDS block
//              and written eight times, slot 8 t + k holding T_k(tile t).  Lanes always run along an output row; the four
//              transposed variants read the LDS block by columns.
//   merge_d8   one block per 32 x 32 block of an output tile: out[t] = (((T_0^-1(y[8 t]) + T_1^-1(y[8 t + 1])) + ...) +
//              T_7^-1(y[8 t + 7])) * 0.125f.  The four flip-only terms are read straight from global memory (a reversed run
//              is one contiguous segment), the four transposed ones are staged through LDS with lanes along their rows.
//              One thread owns an output pixel and adds its eight sources in ascending k: no atomics, the same bits on
//              every run.
// The LDS rows are 33 floats: lane l of a column read sits at dword 33 l + const, 32 distinct banks per half wave, and the
// reads of the 16-byte variants (row 4 q + e, column r; 8 values of q and 4 of r per half wave) at bank (4 q + e + r) % 32,
// distinct too (tools/lds_banks.py, d8_blocks).
#include "common.h"

namespace {

constexpr int NT = 256;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // four floats at dword alignment

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// ---- rdst_unfold_tiles: V tile pixels of one tile row per thread --------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(NT) unfold_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W,
                                                    int p, int s, int pad_y, int pad_x, int Ly, int Lx, int clamp_edge,
                                                    int64_t first_tile, int64_t n_tiles, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int per_row = p / V;
  const int px = (int)(i % per_row) * V;
  int64_t t = i / per_row;
  const int py = (int)(t % p);
  t /= p;
  const int c = (int)(t % C);
  const int64_t slot = t / C;
  const int64_t tile = first_tile + slot;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = 0.f;
  if (tile < n_tiles) {   // (first_tile >= 0 is the entry point's check)
    const int tx = (int)(tile % Lx);
    const int64_t u = tile / Lx;
    const int ty = (int)(u % Ly);
    const int64_t n = u / Ly;
    int sy = ty * s - pad_y + py;
    const int sx = tx * s - pad_x + px;
    bool row = sy >= 0 && sy < H;
    if (clamp_edge) sy = clampi(sy, 0, H - 1), row = true;
    if (row) {
      const float* src = x + ((n * C + c) * H + sy) * W;
      bool run = false;   // four pixels inside the source row: one 16-byte load
      if constexpr (V == 4) {
        run = sx >= 0 && sx + 3 < W;
        if (run) {
          const f4 q = *reinterpret_cast<const f4u*>(src + sx);
          v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
      }
      if (!run) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const int xx = sx + j;
          if (clamp_edge) v[j] = src[clampi(xx, 0, W - 1)];
          else if (xx >= 0 && xx < W) v[j] = src[xx];
        }
      }
    }
  }
  float* dst = out + ((slot * C + c) * p + py) * p + px;
  if constexpr (V == 4) {
    f4 q;
    q.x = v[0], q.y = v[1], q.z = v[2], q.w = v[3];
    *reinterpret_cast<f4*>(dst) = q;
  } else {
    dst[0] = v[0];
  }
}

// ---- rdst_fold_tiles: V output pixels of one row per thread -------------------------------------------------------------
// first and last covering tile of the padded coordinate X on an axis (patch P, stride S, L tiles); first <= last for every
// pixel of a plan the entry point accepted
__device__ __forceinline__ int cover_lo(int X, int P, int S) { return X < P ? 0 : (X - P) / S + 1; }
__device__ __forceinline__ int cover_hi(int X, int S, int L) { return min(X / S, L - 1); }

template <int V>
__global__ void __launch_bounds__(NT) fold_kernel(const float* __restrict__ tiles, float* __restrict__ out, int C, int H, int W,
                                                  int P, int S, int pad_y, int pad_x, int Ly, int Lx, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const int per_row = W / V;
  const int ox = (int)(i % per_row) * V;
  int64_t t = i / per_row;
  const int oy = (int)(t % H);
  t /= H;
  const int c = (int)(t % C);
  const int64_t n = t / C;
  const int Y = oy + pad_y, X = ox + pad_x;
  const int ty0 = cover_lo(Y, P, S), ty1 = cover_hi(Y, S, Ly);
  int lo[V], hi[V];
#pragma unroll
  for (int j = 0; j < V; ++j) lo[j] = cover_lo(X + j, P, S), hi[j] = cover_hi(X + j, S, Lx);
  float acc[V];
#pragma unroll
  for (int j = 0; j < V; ++j) acc[j] = 0.f;
  // both bounds grow with X: [lo[0], hi[V - 1]] holds the covering tiles of all V pixels, and tile tx covers pixel j
  // exactly when its column X + j - tx S lies in [0, P)
  for (int ty = ty0; ty <= ty1; ++ty) {
    const int qy = Y - ty * S;   // in [0, P) by the bounds above
    for (int tx = lo[0]; tx <= hi[V - 1]; ++tx) {
      const float* row = tiles + (((((n * Ly + ty) * Lx + tx) * C + c) * P) + qy) * P;
      const int qx = X - tx * S;
      bool run = false;   // four pixels inside the tile row: one 16-byte load
      if constexpr (V == 4) {
        run = qx >= 0 && qx + 3 < P;
        if (run) {
          const f4 q = *reinterpret_cast<const f4u*>(row + qx);
          acc[0] += q.x, acc[1] += q.y, acc[2] += q.z, acc[3] += q.w;
        }
      }
      if (!run) {
#pragma unroll
        for (int j = 0; j < V; ++j)
          if (qx + j >= 0 && qx + j < P) acc[j] += row[qx + j];
      }
    }
  }
  const int ny = ty1 - ty0 + 1;
  float r[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int count = max(ny * (hi[j] - lo[j] + 1), 1);   // (>= 1 for an accepted plan; never a division by zero)
    r[j] = __fmul_rn(acc[j], __fdiv_rn(1.0f, (float)count));
  }
  float* dst = out + ((n * C + c) * H + oy) * W + ox;
  if constexpr (V == 4) {
    f4 q;
    q.x = r[0], q.y = r[1], q.z = r[2], q.w = r[3];
    *reinterpret_cast<f4*>(dst) = q;
  } else {
    dst[0] = r[0];
  }
}

// ---- the x8 self-ensemble: rdst_unfold_tiles_d8 / rdst_merge_tiles_d8 ---------------------------------------------------
constexpr int TB = 32;         // a tile is handled in TB x TB blocks, partial at the far edges when p is no multiple of TB
constexpr int TBP = TB + 1;    // the padded LDS row

// v[e] = row[f(c0 + e)], e < V, with f(c) = n - 1 - c if `flip`, else c: V neighbouring pixels of a row of n, read through a
// flip.  V == 4 needs row + c0 and n to be multiples of four floats (one aligned 16-byte load either way).
template <int V>
__device__ __forceinline__ void load_run(const float* __restrict__ row, int n, int c0, bool flip, float (&v)[V]) {
  if constexpr (V == 4) {
    const f4 q = *reinterpret_cast<const f4*>(row + (flip ? n - 4 - c0 : c0));
    v[0] = flip ? q.w : q.x, v[1] = flip ? q.z : q.y, v[2] = flip ? q.y : q.z, v[3] = flip ? q.x : q.w;
  } else {
    v[0] = row[flip ? n - 1 - c0 : c0];
  }
}

template <int V>
__device__ __forceinline__ void store_run(float* __restrict__ dst, const float (&v)[V]) {
  if constexpr (V == 4) {
    f4 q;
    q.x = v[0], q.y = v[1], q.z = v[2], q.w = v[3];
    *reinterpret_cast<f4*>(dst) = q;
  } else {
    dst[0] = v[0];
  }
}

// blockIdx.x = ((tile of the launch * C + c) * nb + block row) * nb + block column, nb = ceil(p / TB)
template <int V>
__global__ void __launch_bounds__(NT) unfold_d8_kernel(const float* __restrict__ x, float* __restrict__ out, int C, int H, int W,
                                                       int p, int s, int pad_y, int pad_x, int Ly, int Lx, int clamp_edge,
                                                       int64_t first_tile, int64_t n_tiles, int nb) {
  __shared__ float blk[TB][TBP];
  int64_t t = blockIdx.x;
  const int b0 = (int)(t % nb) * TB;
  t /= nb;
  const int a0 = (int)(t % nb) * TB;
  t /= nb;
  const int c = (int)(t % C);
  const int64_t lt = t / C;                       // its slots are 8 lt + k
  const int64_t tile = first_tile + lt;
  const int ah = min(TB, p - a0), bw = min(TB, p - b0);   // rows [a0, a0 + ah) and columns [b0, b0 + bw) of the tile
  {   // the block of the source tile, zero or the clamped edge outside the image, zeros past the last tile; lanes along a row
    const int cc = threadIdx.x % TB;
    const bool live = tile < n_tiles && cc < bw;   // (first_tile >= 0 is the entry point's check)
    const int tx = (int)(tile % Lx);
    const int64_t u = tile / Lx;
    const int ty = (int)(u % Ly);
    const int64_t n = u / Ly;
    int sx = tx * s - pad_x + b0 + cc;
    bool col = sx >= 0 && sx < W;
    if (clamp_edge) sx = clampi(sx, 0, W - 1), col = true;
    for (int rr = threadIdx.x / TB; rr < ah; rr += NT / TB) {
      int sy = ty * s - pad_y + a0 + rr;
      bool row = sy >= 0 && sy < H;
      if (clamp_edge) sy = clampi(sy, 0, H - 1), row = true;
      float v = 0.f;
      if (live && row && col) v = x[((n * C + c) * H + sy) * W + sx];
      blk[rr][cc] = v;
    }
  }
  __syncthreads();
  constexpr int TPR = TB / V;                     // threads along an output row
  const int q0 = (int)(threadIdx.x % TPR) * V;
  const int64_t slot_stride = (int64_t)C * p * p;
  float* base = out + (lt * 8 * C + c) * (int64_t)p * p;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    // the output rows follow the source rows (the source columns if transposed), the output columns the other axis
    const bool tr = k & 4;
    const bool frow = tr ? (k & 1) : (k & 2), fcol = tr ? (k & 2) : (k & 1);
    const int nr = tr ? bw : ah, nc = tr ? ah : bw;
    const int r0 = tr ? b0 : a0, c0 = tr ? a0 : b0;
    const int io = frow ? p - r0 - nr : r0, jo = fcol ? p - c0 - nc : c0;     // where the block lands in T_k(tile)
    if (q0 < nc) {   // (nc % V == 0: V == 4 only when p % 4 == 0)
      for (int r = threadIdx.x / TPR; r < nr; r += NT / TPR) {
        const int lr = frow ? nr - 1 - r : r;
        float v[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const int lc = fcol ? nc - 1 - (q0 + e) : q0 + e;
          v[e] = tr ? blk[lc][lr] : blk[lr][lc];
        }
        store_run<V>(base + k * slot_stride + (int64_t)(io + r) * p + jo + q0, v);
      }
    }
  }
}

// blockIdx.x = ((t * C + c) * nb + block row) * nb + block column of the output tile, nb = ceil(P / TB).
// T_k^-1(y)[i][j] = y[i'][j'] with a = P - 1 - i if k & 2 else i, b = P - 1 - j if k & 1 else j, (i', j') = (b, a) if k & 4
// else (a, b).
template <int V>
__global__ void __launch_bounds__(NT) merge_d8_kernel(const float* __restrict__ y, float* __restrict__ out, int C, int P, int nb) {
  __shared__ float blk[4][TB][TBP];
  int64_t t = blockIdx.x;
  const int j0 = (int)(t % nb) * TB;
  t /= nb;
  const int i0 = (int)(t % nb) * TB;
  t /= nb;
  const int c = (int)(t % C);
  t /= C;
  const int ih = min(TB, P - i0), jw = min(TB, P - j0);   // output rows [i0, i0 + ih), columns [j0, j0 + jw)
  const int64_t plane = (int64_t)P * P, slot_stride = C * plane;
  const float* src = y + (t * 8 * C + c) * plane;
  constexpr int TPR = TB / V;
  const int q0 = (int)(threadIdx.x % TPR) * V;
  // the transposed terms: blk[k - 4][jj][ii] = y_k[b(j0 + jj)][a(i0 + ii)], lanes along ii (a row of y_k)
  if (q0 < ih) {   // (ih % V == 0: V == 4 only when P % 4 == 0)
#pragma unroll
    for (int k = 4; k < 8; ++k) {
      const float* yk = src + k * slot_stride;
      for (int jj = threadIdx.x / TPR; jj < jw; jj += NT / TPR) {
        const int row = (k & 1) ? P - 1 - (j0 + jj) : j0 + jj;
        float v[V];
        load_run<V>(yk + (int64_t)row * P, P, i0 + q0, k & 2, v);
#pragma unroll
        for (int e = 0; e < V; ++e) blk[k - 4][jj][q0 + e] = v[e];
      }
    }
  }
  __syncthreads();
  if (q0 < jw) {
    for (int r = threadIdx.x / TPR; r < ih; r += NT / TPR) {
      float acc[V];
#pragma unroll
      for (int k = 0; k < 4; ++k) {   // the flip-only terms, straight from global memory
        const int row = (k & 2) ? P - 1 - (i0 + r) : i0 + r;
        float v[V];
        load_run<V>(src + k * slot_stride + (int64_t)row * P, P, j0 + q0, k & 1, v);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = k == 0 ? v[e] : __fadd_rn(acc[e], v[e]);
      }
#pragma unroll
      for (int k = 4; k < 8; ++k)
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = __fadd_rn(acc[e], blk[k - 4][q0 + e][r]);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = __fmul_rn(acc[e], 0.125f);
      store_run<V>(out + (t * C + c) * plane + (int64_t)(i0 + r) * P + j0 + q0, acc);
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

constexpr int MAX_EXTENT = 1 << 24;   // every coordinate and every padded extent of an axis stays far inside an int

// the plan of one axis: n pixels, patch, stride, pad, L tiles.  0, or a message for rdst_fail.
const char* bad_axis(int n, int patch, int stride, int pad, int L) {
  if (n <= 0 || patch <= 0 || stride <= 0 || L <= 0) return "non-positive size";
  if (pad < 0) return "negative padding";
  if (n > MAX_EXTENT || patch > MAX_EXTENT || stride > MAX_EXTENT || pad > MAX_EXTENT || L > MAX_EXTENT) return "size too large";
  if (stride > patch) return "stride > patch leaves pixels between the tiles uncovered";
  const int64_t reach = (int64_t)(L - 1) * stride + patch;
  if (reach > MAX_EXTENT) return "size too large";
  if (reach < (int64_t)pad + n) return "the tiles do not reach the end of the axis";
  return nullptr;
}

}  // namespace

extern "C" int rdst_unfold_tiles(const float* x, float* out, int N, int C, int H, int W, int p, int s, int pad_y, int pad_x,
                                 int Ly, int Lx, int pad_mode, int64_t first_tile, int n_slots, void* stream) {
  const char* who = "rdst_unfold_tiles";
  if (N <= 0 || C <= 0 || n_slots <= 0 || first_tile < 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d first_tile=%lld n_slots=%d", who, N, C, (long long)first_tile, n_slots);
  const char* bad = bad_axis(H, p, s, pad_y, Ly);
  if (!bad) bad = bad_axis(W, p, s, pad_x, Lx);
  if (bad)
    return rdst_fail(RDST_EINVAL, "%s: %s (H=%d W=%d patch=%d stride=%d pad=%d,%d tiles=%d x %d)", who, bad, H, W, p, s, pad_y,
                     pad_x, Ly, Lx);
  if (pad_mode != 0 && pad_mode != 1) return rdst_fail(RDST_EINVAL, "%s: bad pad mode %d", who, pad_mode);
  if (!x || !out) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if ((double)N * C * H * W > (double)((int64_t)1 << 40) || (double)n_slots * C * p * p > (double)((int64_t)1 << 40))
    return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d n_slots=%d is too large for one launch", who, N, C, n_slots);
  const int64_t n_tiles = (int64_t)N * Ly * Lx;
  const bool wide = p % 4 == 0 && aligned16(out);
  const int64_t total = (int64_t)n_slots * C * p * (p / (wide ? 4 : 1));
  const int64_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: %lld tile pixels are too many for one launch", who, (long long)total);
  if (wide)
    hipLaunchKernelGGL(unfold_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, out, C, H, W, p, s, pad_y,
                       pad_x, Ly, Lx, pad_mode, first_tile, n_tiles, total);
  else
    hipLaunchKernelGGL(unfold_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, out, C, H, W, p, s, pad_y,
                       pad_x, Ly, Lx, pad_mode, first_tile, n_tiles, total);
  return rdst_launch_status(who);
}

extern "C" int rdst_fold_tiles(const float* tiles, float* out, int N, int C, int H, int W, int P, int S, int pad_y, int pad_x,
                               int Ly, int Lx, void* stream) {
  const char* who = "rdst_fold_tiles";
  if (N <= 0 || C <= 0) return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d", who, N, C);
  const char* bad = bad_axis(H, P, S, pad_y, Ly);
  if (!bad) bad = bad_axis(W, P, S, pad_x, Lx);
  if (bad)
    return rdst_fail(RDST_EINVAL, "%s: %s (H=%d W=%d patch=%d stride=%d pad=%d,%d tiles=%d x %d)", who, bad, H, W, P, S, pad_y,
                     pad_x, Ly, Lx);
  if (!tiles || !out) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if ((double)N * C * H * W > (double)((int64_t)1 << 40) || (double)N * Ly * Lx * C * P * P > (double)((int64_t)1 << 40))
    return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d with %d x %d tiles is too large for one launch", who, N, C, Ly, Lx);
  const bool wide = W % 4 == 0 && aligned16(out);
  const int64_t total = (int64_t)N * C * H * (W / (wide ? 4 : 1));
  const int64_t blocks = (total + NT - 1) / NT;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: %lld pixels are too many for one launch", who, (long long)total);
  if (wide)
    hipLaunchKernelGGL(fold_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, tiles, out, C, H, W, P, S, pad_y,
                       pad_x, Ly, Lx, total);
  else
    hipLaunchKernelGGL(fold_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, tiles, out, C, H, W, P, S, pad_y,
                       pad_x, Ly, Lx, total);
  return rdst_launch_status(who);
}

extern "C" int rdst_unfold_tiles_d8(const float* x, float* out, int N, int C, int H, int W, int p, int s, int pad_y, int pad_x,
                                    int Ly, int Lx, int pad_mode, int64_t first_tile, int n_slots, void* stream) {
  const char* who = "rdst_unfold_tiles_d8";
  if (N <= 0 || C <= 0 || n_slots <= 0 || first_tile < 0)
    return rdst_fail(RDST_EINVAL, "%s: bad shape N=%d C=%d first_tile=%lld n_slots=%d", who, N, C, (long long)first_tile, n_slots);
  if (n_slots % 8) return rdst_fail(RDST_EINVAL, "%s: n_slots=%d is not a multiple of 8 (eight slots per tile)", who, n_slots);
  const char* bad = bad_axis(H, p, s, pad_y, Ly);
  if (!bad) bad = bad_axis(W, p, s, pad_x, Lx);
  if (bad)
    return rdst_fail(RDST_EINVAL, "%s: %s (H=%d W=%d patch=%d stride=%d pad=%d,%d tiles=%d x %d)", who, bad, H, W, p, s, pad_y,
                     pad_x, Ly, Lx);
  if (pad_mode != 0 && pad_mode != 1) return rdst_fail(RDST_EINVAL, "%s: bad pad mode %d", who, pad_mode);
  if (!x || !out) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if ((double)N * C * H * W > (double)((int64_t)1 << 40) || (double)n_slots * C * p * p > (double)((int64_t)1 << 40))
    return rdst_fail(RDST_EINVAL, "%s: N=%d C=%d n_slots=%d is too large for one launch", who, N, C, n_slots);
  const int64_t n_tiles = (int64_t)N * Ly * Lx;
  const int nb = (p + TB - 1) / TB;
  const int64_t blocks = (int64_t)(n_slots / 8) * C * nb * nb;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: %lld tile blocks are too many for one launch", who, (long long)blocks);
  if (p % 4 == 0 && aligned16(out))
    hipLaunchKernelGGL(unfold_d8_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, out, C, H, W, p, s,
                       pad_y, pad_x, Ly, Lx, pad_mode, first_tile, n_tiles, nb);
  else
    hipLaunchKernelGGL(unfold_d8_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, x, out, C, H, W, p, s,
                       pad_y, pad_x, Ly, Lx, pad_mode, first_tile, n_tiles, nb);
  return rdst_launch_status(who);
}

extern "C" int rdst_merge_tiles_d8(const float* y, float* out, int n_tiles, int C, int P, void* stream) {
  const char* who = "rdst_merge_tiles_d8";
  if (n_tiles <= 0 || C <= 0 || P <= 0) return rdst_fail(RDST_EINVAL, "%s: bad shape n_tiles=%d C=%d P=%d", who, n_tiles, C, P);
  if (P > MAX_EXTENT) return rdst_fail(RDST_EINVAL, "%s: size too large (P=%d)", who, P);
  if (!y || !out) return rdst_fail(RDST_EINVAL, "%s: null pointer", who);
  if (8.0 * n_tiles * C * P * P > (double)((int64_t)1 << 40))
    return rdst_fail(RDST_EINVAL, "%s: n_tiles=%d C=%d P=%d is too large for one launch", who, n_tiles, C, P);
  const int nb = (P + TB - 1) / TB;
  const int64_t blocks = (int64_t)n_tiles * C * nb * nb;
  if (blocks > 0x7fffffff) return rdst_fail(RDST_EINVAL, "%s: %lld tile blocks are too many for one launch", who, (long long)blocks);
  if (P % 4 == 0 && aligned16(y) && aligned16(out))
    hipLaunchKernelGGL(merge_d8_kernel<4>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, y, out, C, P, nb);
  else
    hipLaunchKernelGGL(merge_d8_kernel<1>, dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)stream, y, out, C, P, nb);
  return rdst_launch_status(who);
}
