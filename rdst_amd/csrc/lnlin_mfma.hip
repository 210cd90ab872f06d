// The first one-pass Linear backward (bf16): what lnlin3_mfma.hip, its re-cut for the E1 shapes, falls back to.
// Backward of a LayerNorm-fused Linear (norm1 + qkv) in ONE pass over (x, dY): the same skeleton as the Mlp
// backward (mlp_mfma.hip) without the recompute.  Unfused, dY (3C wide) and x are read twice (data-gradient kernel, weight-
// gradient kernel); here every tile is staged once and feeds both products:
//   phase 2  wave w: G[n-tile w][c] += dY^T x-hat   (both operands read transposed from the token-major tiles)
//   phase 3  waves 0..K/32: dX-hat^T = (W gamma)^T dY^T (W gamma read transposed from its one LDS image, dY rows as
//            they lie), LayerNorm backward, + dX_add (the residual fan-out), 16-B row stores
// G (N, K+1) goes through the same sum / LayerNorm-finish kernels as linear_wgrad_ln_mfma.
#include "linear.h"
#include "mfma.h"
#include "reduce_batch.h"
#include "wattn_hd.h"
#include <stdlib.h>

namespace {
using namespace wahd;
using MM = Mma<bf16>;

// loads through an explicitly GLOBAL pointer (address space 1): the value is copied out of the qualified lvalue here
typedef __attribute__((address_space(1))) const char* gcp;
__device__ __forceinline__ u32x4_a4 gload16(gcp q) {
  const u32x4_a4 v = *reinterpret_cast<__attribute__((address_space(1))) const u32x4_a4*>(q);
  return v;
}
__device__ __forceinline__ float2 gload8(gcp q) {
  const float x = *reinterpret_cast<__attribute__((address_space(1))) const float*>(q);
  const float y = *reinterpret_cast<__attribute__((address_space(1))) const float*>(q + 4);
  return make_float2(x, y);
}

__host__ __device__ inline int lnlin_ldy(int NP) {   // dY tile row stride: see the stride note in the kernel
  const int b = NP * 2 + 16;
  return (b & 255) < 48 ? b + 64 : b;
}

struct LnLinArgs {
  const bf16* X; int64_t ldx; const float* stats; const float* lnw; const float* W;
  const bf16* dY; int64_t lddy; bf16* dX; int64_t lddx; const bf16* Acc; int64_t ldacc;
  float* slab; int64_t slab_stride;
  int64_t M; int K; int N; int NW; int NWV; int64_t ntiles; int tiles_per_wg;   // NW n-tiles, NWV >= NW waves launched
  unsigned long long* stamps;   // RDST_LNLIN_STAMPS=n (debug)
};

// LN = false: plain Linear (proj): x-hat is x itself, no LayerNorm backward, W unscaled
template <int NCT, bool LN>
__global__ void __launch_bounds__(768, 3) lnlin_bwd_kernel(const LnLinArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // LDS row strides.  The tiles are read TRANSPOSED (4 consecutive rows x 64 B per 16 lanes): a stride of 16 (mod 256)
  // — 272 B for the 256-B rows of C = 120 — stacks the four rows on the same banks (4-way conflicts, measured: the
  // whole phase was LDS-throughput bound); 80 (mod 256) keeps b128 row reads conflict-free too (odd 16-B slot count)
  constexpr int CP = 32 * NCT, PK = CP / 8, LDW = NCT == 4 ? 288 : CP * 2 + 16, LDX = NCT == 4 ? 336 : CP * 2 + 16;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, hh = lane >> 5;
  const int K = p.K, N = p.N, NW = p.NW, NT = 64 * p.NWV;
  const int NP = 32 * NW, KN = 2 * NW, LDY = lnlin_ldy(NP);
  const int OFF_XH = NP * LDW, OFF_AC = OFF_XH + 32 * LDX, OFF_DY = OFF_AC + 32 * LDX, OFF_SM = OFF_DY + 32 * LDY,
            OFF_RED = OFF_SM + 128;
  float* sm = reinterpret_cast<float*>(smem + OFF_SM);
  float* red = reinterpret_cast<float*>(smem + OFF_RED);
  int nst = 0;
  auto stamp = [&]() {
    if (RDST_DBGV(p.stamps) && tid == 0 && nst < 14) p.stamps[(size_t)blockIdx.x * 16 + nst++] = __builtin_readcyclecounter();
  };
  stamp();

  // ---- prologue: zero padding, ones column, W*gamma image ----
  lds_zero16(smem, OFF_SM, tid, NT);
  {
    const int pk = tid % PK, jr = tid / PK, c0 = 8 * pk, rpp = NT / PK;   // rows per pass
    float gq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) gq[e] = LN ? p.lnw[c0 + e < K ? c0 + e : K - 1] : 1.0f;
#pragma unroll
    for (int e = 0; e < 8; ++e) gq[e] = c0 + e < K ? gq[e] : 0.f;
    const int cl = c0 < K - 8 ? c0 : K - 8, sh = c0 - cl;
    __syncthreads();   // zero fill done
    for (int n0 = 0; n0 < N; n0 += 4 * rpp) {
      float w[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = n0 + u * rpp + jr;
        const float* src = p.W + (int64_t)(n < N ? n : N - 1) * K + cl;
        const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(src), b = *reinterpret_cast<const u32x4_a4*>(src + 4);
        w[u][0] = __uint_as_float(a.x); w[u][1] = __uint_as_float(a.y); w[u][2] = __uint_as_float(a.z); w[u][3] = __uint_as_float(a.w);
        w[u][4] = __uint_as_float(b.x); w[u][5] = __uint_as_float(b.y); w[u][6] = __uint_as_float(b.z); w[u][7] = __uint_as_float(b.w);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int n = n0 + u * rpp + jr;
        if (n < N && sh < 8) {
          float f[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float x = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) x = (k == e + sh) ? w[u][k] : x;
            f[e] = x * gq[e];
          }
          *reinterpret_cast<Pack16*>(smem + n * LDW + c0 * 2) = MM::pack(f);
        }
      }
    }
    if (tid < 32) *reinterpret_cast<uint16_t*>(smem + OFF_XH + tid * LDX + K * 2) = 0x3f80;   // ones column of x-hat
  }

  // ---- loader plan: up to 4 chunk slots per thread over [dY chunks | x chunks | dX_add chunks] (the x range is no
  // longer than the thread count, so a thread owns at most one x chunk and needs one statistics pair).  Kept in
  // TWO registers per slot (meta = byte offset in the row | tile row << 16 | kind << 24 | aligned << 28, LDS offset):
  // the kernel runs three waves per SIMD and every register not spent here lets the LDS reads of the phases below
  // be issued in batches instead of one round trip per MFMA ----
  const int PKY = (N * 2 + 15) >> 4;
  const int nY = 32 * PKY, nX = 32 * PK, nA = p.Acc ? 32 * PK : 0;
  int lds_off[4], meta[4];   // kind: 0 dY, 1 x, 2 dX_add, 7 none
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    // LN form (wide dY): slot u has a fixed kind — 0, 1: dY, 2: x, 3: dX_add; plain form: slots dealt out in order
    const int g = tid + NT * u;
    const int kd = LN ? (u < 2 ? (g < nY ? 0 : -1) : u == 2 ? (tid < nX ? 1 : -1) : (tid < nA ? 2 : -1))
                      : (g < nY ? 0 : g < nY + nX ? 1 : g < nY + nX + nA ? 2 : -1);
    const int idx = LN ? (u < 2 ? g : tid) : (kd == 0 ? g : kd == 1 ? g - nY : g - nY - nX);
    const int per = kd == 0 ? PKY : PK, rowbytes = kd == 0 ? N * 2 : K * 2;
    const int row = (kd < 0 ? 0 : idx / per), chk = kd < 0 ? 0 : idx - row * per;
    int o = chk * 16;
    const bool on = kd >= 0 && o < rowbytes;
    if (o + 16 > rowbytes) o = rowbytes - 16;
    if (!on) o = 0;
    const int lr = row & 31;
    meta[u] = o | (lr << 16) | ((on ? kd : 7) << 24) | (((o & 15) == 0 ? 1 : 0) << 28);
    lds_off[u] = (kd == 0 ? OFF_DY + lr * LDY : (kd == 2 ? OFF_AC : OFF_XH) + lr * LDX) + o;
  }
  auto m_off = [](int m) { return m & 0xffff; };
  auto m_row = [](int m) { return (m >> 16) & 31; };
  auto m_kind = [](int m) { return (m >> 24) & 7; };
  auto m_al = [](int m) { return ((m >> 28) & 1) != 0; };
  const uint32_t ldb_y = (uint32_t)(p.lddy * 2), ldb_x = (uint32_t)(p.ldx * 2), ldb_a = (uint32_t)(p.ldacc * 2);   // row strides, bytes
  u32x4_a4 rd[4];
  float2 rst = make_float2(0.f, 1.f);
  // explicitly GLOBAL pointers: a pointer that went through an integer or a select is a flat pointer to the compiler,
  // flat loads count on the LDS counter as well, and the next barrier then waits for the whole prefetch (measured)
  const gcp base_s = (gcp)(uintptr_t)p.stats;
  const uint32_t Mu = (uint32_t)p.M;
  // plain form (dynamic slot kinds): one global pointer per slot, set up once (a run-time select between base
  // addresses inside the loop was lowered to a scratch table and flat loads)
  const char* gp[4];
  uint32_t gld[4];
  if constexpr (!LN) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kd = m_kind(meta[u]);
      const bf16* b0 = kd == 0 ? p.dY : kd == 2 ? p.Acc : p.X;
      gp[u] = reinterpret_cast<const char*>(b0 ? b0 : p.X) + m_off(meta[u]);
      gld[u] = kd == 0 ? ldb_y : kd == 2 ? ldb_a : ldb_x;
    }
  }
  auto fetch = [&](int64_t tile) {   // byte offsets fit 32 bits (checked by the launcher); no conditional loads either:
                                     // a lane-masked load is a branch with a wait at its end
    if constexpr (!LN) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        uint32_t row = (uint32_t)(tile * 32) + (uint32_t)m_row(meta[u]);
        row = row < Mu ? row : Mu - 1;
        rd[u] = *reinterpret_cast<const u32x4_a4*>(gp[u] + (size_t)(row * gld[u]));
      }
      return;
    }
    uint32_t srow = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      // LN form: the slot's kind is a compile-time constant (0, 1: dY, 2: x, 3: dX_add) — no pointer selects
      const int kd = u < 2 ? 0 : u == 2 ? 1 : 2;
      uint32_t row = (uint32_t)(tile * 32) + (uint32_t)m_row(meta[u]);
      row = row < Mu ? row : Mu - 1;
      const gcp base = kd == 0 ? (gcp)(uintptr_t)p.dY : kd == 2 ? (gcp)(uintptr_t)(p.Acc ? p.Acc : p.X) : (gcp)(uintptr_t)p.X;
      const uint32_t ldb = kd == 0 ? ldb_y : kd == 2 ? ldb_a : ldb_x;
      rd[u] = gload16(base + (row * ldb + (uint32_t)m_off(meta[u])));
      srow = kd == 1 ? row : srow;
    }
    if (LN) rst = gload8(base_s + 8 * (size_t)srow);
  };
  auto put16 = [&](char* dst, const Pack16& v, bool aligned) {
    if (aligned) *reinterpret_cast<Pack16*>(dst) = v;
    else {
      uint32_t* d = reinterpret_cast<uint32_t*>(dst);
      d[0] = v.w[0]; d[1] = v.w[1]; d[2] = v.w[2]; d[3] = v.w[3];
    }
  };
  auto stash = [&](int64_t tile) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (m_kind(meta[u]) == 7) continue;
      const int kd = LN ? (u < 2 ? 0 : u == 2 ? 1 : 2) : m_kind(meta[u]);
      const bool valid = (uint32_t)(tile * 32) + (uint32_t)m_row(meta[u]) < Mu;
      Pack16 v;
      if (LN && kd == 1) {
        float f[8];
        unpack8(rd[u], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = valid ? (f[e] - rst.x) * rst.y : 0.f;
        v = MM::pack(f);
        if (m_off(meta[u]) == 0) sm[m_row(meta[u])] = rst.y;
      } else {
        v.w[0] = valid ? rd[u].x : 0u; v.w[1] = valid ? rd[u].y : 0u; v.w[2] = valid ? rd[u].z : 0u; v.w[3] = valid ? rd[u].w : 0u;
      }
      put16(smem + lds_off[u], v, m_al(meta[u]));
    }
  };

  const int q = (lane & 15) >> 2, pp = lane & 3, gq1 = (lane >> 4) & 1;
  const int trc = (16 * gq1 + 4 * pp) * 2;
  const lds_cp ytr = (lds_cp)(smem + OFF_DY + (8 * hh + q) * LDY + trc + wave * 64);   // dY columns of the wave's n-tile
  const lds_cp xtr = (lds_cp)(smem + OFF_XH + (8 * hh + q) * LDX + trc);
  const lds_cp wtr = (lds_cp)(smem + (8 * hh + q) * LDW + trc + wave * 64);            // wave < NCT: channel tile = wave
  const lds_cp yrow = (lds_cp)(smem + OFF_DY + r * LDY + hh * 16);

  f32x16 G[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int v = 0; v < 16; ++v) G[ct][v] = 0.f;

  const int64_t t0 = (int64_t)blockIdx.x * p.tiles_per_wg;
  const int64_t t1 = t0 + p.tiles_per_wg < p.ntiles ? t0 + p.tiles_per_wg : p.ntiles;
  const float invK = 1.0f / (float)K;
  __syncthreads();   // W image, ones column
  stamp();   // 1: prologue
  if (t0 < t1) fetch(t0);
  for (int64_t tile = t0; tile < t1; ++tile) {
    stash(tile);
    fetch(tile + 1 < t1 ? tile + 1 : tile);   // every iteration defines the whole prefetch set
    __syncthreads();   // B1
    stamp();   // staged
    // ---- phase 2 (waves that own an n-tile)
    if (wave < NW) {
      // every operand of the tile is read before the first MFMA (one LDS round trip, not one per MFMA)
      Pack16 ya[2], xb[NCT][2];
#pragma unroll
      for (int s = 0; s < 2; ++s) ya[s] = lds_tr_pack(ytr + 16 * s * LDY, ytr + (16 * s + 4) * LDY);
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int s = 0; s < 2; ++s) xb[ct][s] = lds_tr_pack(xtr + 16 * s * LDX + ct * 64, xtr + (16 * s + 4) * LDX + ct * 64);
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) MM::mma(G[ct], ya[s], xb[ct][s]);   // rows = output features n, columns = channels (column K = d(bias))
    }
    // ---- phase 3
    f32x16 dx;
    float rstd = 0.f;
    if (wave < NCT) {
      f32x16 dx2;
#pragma unroll
      for (int v = 0; v < 16; ++v) { dx[v] = 0.f; dx2[v] = 0.f; }
      for (int kk = 0; kk < KN; kk += 4) {   // KN = 2 NW: groups of four k-steps (the last group may hold two), read together
        Pack16 wa[4], yb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int k2 = kk + i < KN ? kk + i : KN - 1;
          wa[i] = lds_tr_pack(wtr + 16 * k2 * LDW, wtr + (16 * k2 + 4) * LDW);
          yb[i] = lds_pack(yrow + 32 * k2);
        }
        MM::mma(dx, wa[0], yb[0]);   // rows = channels, columns = tokens
        MM::mma(dx2, wa[1], yb[1]);
        if (kk + 2 < KN) {
          MM::mma(dx, wa[2], yb[2]);
          MM::mma(dx2, wa[3], yb[3]);
        }
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) dx[v] += dx2[v];
      if (LN) {
      rstd = sm[r];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const u32x2_t xv = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + OFF_XH + r * LDX) + (32 * wave + 8 * g4 + 4 * hh) * 2);
        const float xh[4] = {bf16lo(xv.x), bf16hi(xv.x), bf16lo(xv.y), bf16hi(xv.y)};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s1 += dx[4 * g4 + e];
          s2 = fmaf(dx[4 * g4 + e], xh[e], s2);
        }
      }
      s1 = half_swap_sum(s1);
      s2 = half_swap_sum(s2);
      if (hh == 0) *reinterpret_cast<float2*>(red + (wave * 32 + r) * 2) = make_float2(s1, s2);
      }
    }
    if (LN) __syncthreads();   // B3
    stamp();   // phases 2, 3a
    if (wave < NCT) {
      float s1 = 0.f, s2 = 0.f;
      if (LN) {
#pragma unroll
      for (int w = 0; w < NCT; ++w) {
        const float2 v = *reinterpret_cast<const float2*>(red + (w * 32 + r) * 2);
        s1 += v.x; s2 += v.y;
      }
      s1 *= invK; s2 *= invK;
      }
      float o[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int cb = (32 * wave + 8 * g4 + 4 * hh) * 2;
        const u32x2_t xv = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + OFF_XH + r * LDX) + cb);
        const u32x2_t av = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + OFF_AC + r * LDX) + cb);   // zeros without dX_add
        const float xh[4] = {bf16lo(xv.x), bf16hi(xv.x), bf16lo(xv.y), bf16hi(xv.y)};
        const float ac[4] = {bf16lo(av.x), bf16hi(av.x), bf16lo(av.y), bf16hi(av.y)};
#pragma unroll
        for (int e = 0; e < 4; ++e) o[4 * g4 + e] = LN ? fmaf(rstd, dx[4 * g4 + e] - s1 - xh[e] * s2, ac[e]) : dx[4 * g4 + e] + ac[e];
      }
      const int64_t row = tile * 32 + r;
      if (row < p.M) {
        bf16* drow = p.dX + row * p.lddx;
#pragma unroll
        for (int gp2 = 0; gp2 < 2; ++gp2) {
          float c8[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[8 * gp2 + e]), __float_as_uint(o[8 * gp2 + 4 + e]), false, false);
            c8[e] = __uint_as_float(sw[0]);
            c8[4 + e] = __uint_as_float(sw[1]);
          }
          const int cb = 32 * wave + 8 * (2 * gp2 + hh);
          if (cb + 8 <= K) {
            u32x4_a4 u;
            u.x = pack_bf16x2(c8[0], c8[1]); u.y = pack_bf16x2(c8[2], c8[3]);
            u.z = pack_bf16x2(c8[4], c8[5]); u.w = pack_bf16x2(c8[6], c8[7]);
            *reinterpret_cast<u32x4_a4*>(drow + cb) = u;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (cb + e < K) drow[cb + e] = __float2bfloat16(c8[e]);
          }
        }
      }
    }
    __syncthreads();   // B4
    stamp();   // 3b
  }
  if (RDST_DBGV(p.stamps) && tid == 0) p.stamps[(size_t)blockIdx.x * 16 + 14] = __builtin_readcyclecounter();   // slot 14: loop done
  // bf16 slab in groups of 4 rows (reduce_batch.h, "G4"): G [N][K+1]; p.slab_stride counts 8-byte groups
  uint2* my = reinterpret_cast<uint2*>(p.slab) + (int64_t)blockIdx.x * p.slab_stride;
  if (wave < NW)
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int c = 32 * ct + r;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int n0 = 32 * wave + 8 * g4 + 4 * hh;
      if (n0 < N && c <= K)
        my[(int64_t)(n0 >> 2) * (K + 1) + c] = make_uint2(pack_bf16x2(G[ct][4 * g4], G[ct][4 * g4 + 1]), pack_bf16x2(G[ct][4 * g4 + 2], G[ct][4 * g4 + 3]));
    }
  }
  if (RDST_DBGV(p.stamps) && tid == 0) p.stamps[(size_t)blockIdx.x * 16 + 15] = __builtin_readcyclecounter();   // slot 15: kernel end
}
}  // namespace

// fixed-order sums of the per-workgroup bf16 G4 slabs (+ the LayerNorm finish) of the one-pass Linear backward kernels
static int lnlin_bwd_reduce(float* slab, int grid, int64_t slab_stride, bool ln, const float* Wt, const float* ln_w,
                            const float* ln_b, float* dW, float* dbias, float* dln_w, float* dln_b, float* G, int N, int K,
                            hipStream_t st) {
  rbatch::SumJob sj{};
  sj.slab = slab; sj.nwg = grid; sj.stride = slab_stride; sj.g4 = 1; sj.a2 = N; sj.b2 = K + 1; sj.tot = ((N + 3) / 4) * (K + 1);
  if (!ln) {
    sj.map = rbatch::MAP_LINEAR; sj.out = dW; sj.out2 = dbias; sj.a = K; sj.b = K + 1; sj.s = 1.0f;
    return rbatch::sum(sj, st);
  }
  sj.map = rbatch::MAP_COPY; sj.out = G;
  if (int rc = rbatch::sum(sj, st)) return rc;
  return wgrad_ln_finish_launch(G, Wt, ln_w, ln_b, N, K, 1.0f, dW, dbias, dln_w, dln_b, st);
}

// Linear backward in one pass over (x, dY), with (ln_w != NULL) or without a LayerNorm in front: bf16, K+1 <= 128,
// N <= 384, out_scale 1, no input activation; RDST_ENOTSUP otherwise
int linear_ln_bwd_fused_bf16(const bf16* X, int64_t ldx, const float* ln_w, const float* ln_b, const float* stats,
                             const float* Wt, const bf16* dY, int64_t lddy, bf16* dX, int64_t lddx, const bf16* acc,
                             int64_t ldacc, float* dW, float* dbias, float* dln_w, float* dln_b, const WsSlab& slab, float* G,
                             int64_t M, int K, int N, float s, hipStream_t st, const bf16* acc2, int64_t ldacc2) {
  static int off = -1;
  if (off < 0) { const char* e = rdst_dbg_getenv("RDST_LNLIN_V1"); off = e ? atoi(e) : 0; }   // 1: all off, 2: the plain-Linear form off
  const bool ln = ln_w != nullptr;
  if (off == 1 || (off == 2 && !ln) || s != 1.0f || M <= 0) return RDST_ENOTSUP;
  const int nct = (K + 1 + 31) / 32;
  if (nct < 2 || nct > 4 || (K & 1) || K < 8 || (N & 1) || N < 8) return RDST_ENOTSUP;
  const int NW = (N + 31) / 32;
  if (NW > 12) return RDST_ENOTSUP;
  const int PK = 4 * nct, PKY = (N * 2 + 15) / 16;
  // waves launched: one per n-tile, at least the K/32 of phase 3, and enough threads for the loader's fixed slots
  int NWV = NW > nct ? NW : nct;
  if (ln && NWV < 2 * nct) NWV = 2 * nct;
  const int NT = 64 * NWV;
  if (4 * NT < 32 * (PKY + PK * (acc ? 2 : 1))) return RDST_ENOTSUP;
  if (ln && (NT < 32 * PK || 2 * NT < 32 * PKY)) return RDST_ENOTSUP;   // fixed slot kinds: dY in two slots, x and dX_add in one each
  if (((uintptr_t)X & 3) || ((uintptr_t)dY & 3) || ((uintptr_t)dX & 3) || ((uintptr_t)acc & 3) || (ldx & 1) || (lddy & 1) ||
      (lddx & 1) || (ldacc & 1))
    return RDST_ENOTSUP;
  if ((uint64_t)M * (uint64_t)(lddy > ldx ? (lddy > ldacc ? lddy : ldacc) : (ldx > ldacc ? ldx : ldacc)) * 2 >= (1ull << 31)) return RDST_ENOTSUP;   // 32-bit byte offsets in the loader
  const int64_t slab_stride = (int64_t)((N + 3) / 4) * (K + 1);   // bf16 G4 slab: 8-byte groups
  {  // the re-cut kernel for the E1 shapes (lnlin3_mfma.hip)
    int g3 = 0;
    if (acc2 && (((uintptr_t)acc2 & 3) || (ldacc2 & 1) || (uint64_t)M * (uint64_t)ldacc2 * 2 >= (1ull << 31))) return RDST_ENOTSUP;
    const int rc3 = lnlin3_bwd_bf16(X, ldx, ln_w, stats, Wt, dY, lddy, dX, lddx, acc, ldacc, acc2, ldacc2, slab, slab_stride, M, K,
                                    N, &g3, st);
    if (rc3 == 0) return lnlin_bwd_reduce(slab.p, g3, slab_stride, ln, Wt, ln_w, ln_b, dW, dbias, dln_w, dln_b, G, N, K, st);
    if (rc3 != RDST_ENOTSUP || acc2) return rc3;   // (only the re-cut kernel takes a second addend)
  }
  const int CP = 32 * nct, LDW = nct == 4 ? 288 : CP * 2 + 16, LDX = nct == 4 ? 336 : CP * 2 + 16, NP = 32 * NW, LDY = lnlin_ldy(NP);
  const int smem = NP * LDW + 2 * 32 * LDX + 32 * LDY + 128 + nct * 32 * 8;
  if (smem > 160 * 1024) return RDST_ENOTSUP;
  LnLinArgs p{};
  p.X = X; p.ldx = ldx; p.stats = stats; p.lnw = ln_w; p.W = Wt; p.dY = dY; p.lddy = lddy; p.dX = dX; p.lddx = lddx;
  p.Acc = acc; p.ldacc = ldacc; p.M = M; p.K = K; p.N = N; p.NW = NW; p.NWV = NWV;
  p.ntiles = (M + 31) / 32;
  // small workgroups (the C -> C projections: 2-4 waves) share a CU: up to 12 waves and the LDS that fits
  int per_cu = ln ? 1 : 12 / NWV;
  if (per_cu > 160 * 1024 / smem) per_cu = 160 * 1024 / smem;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 2) per_cu = 2;   // more workgroups only add slab traffic (measured)
  { const char* e = rdst_dbg_getenv("RDST_LNLIN_PERCU"); if (e && atoi(e) > 0) per_cu = atoi(e); }
  p.slab = slab.p;
  p.slab_stride = slab_stride;
  const int64_t grid = rdst_tile_grid(p.ntiles, slab.cap((int64_t)kCUs * per_cu, 2 * slab_stride), &p.tiles_per_wg);   // (8-byte groups: 2 floats)
  if (int rc = rdst_slab_fits(slab, grid, 2 * slab_stride, "lnlin_bwd")) return rc;
  int rc = 0;
#define RDST_LNLIN(NC)                                                                                               \
  {                                                                                                                  \
    auto kern = ln ? lnlin_bwd_kernel<NC, true> : lnlin_bwd_kernel<NC, false>;                                       \
    rc = rdst_launch(kern, dim3((unsigned)grid), dim3(NT), smem, st, "lnlin_bwd", p);                                 \
  }
  p.stamps = rdst_stamps_begin("RDST_LNLIN_STAMPS", grid, 16, st);
  if (nct == 2) RDST_LNLIN(2) else if (nct == 3) RDST_LNLIN(3) else RDST_LNLIN(4)
#undef RDST_LNLIN
  rdst_stamps_end(p.stamps, grid, 16, RDST_STAMPS_TICKS, st, "lnlin_bwd K=%d N=%d ln=%d", K, N, (int)ln);
  if (rc) return rc;
  return lnlin_bwd_reduce(slab.p, (int)grid, p.slab_stride, ln, Wt, ln_w, ln_b, dW, dbias, dln_w, dln_b, G, N, K, st);
}
