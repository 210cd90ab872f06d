// K7: the Mlp half of a Swin block — y = x + fc2(GELU(fc1(LayerNorm(x)))) (swin_transformer_sr.py:24-27, :272) —
// fused END TO END in the bf16 throughput mode: the backward is ONE kernel that reads x and dY and writes dX.
//
// Why: unfused, the Mlp backward moves 16 row-widths of HBM traffic per token (dH written and read twice, the
// fc1 pre-activation read twice, x and dY read three times) through four kernels plus their slab reductions.
// Fused it moves 3 (x, dY in; dX out): the hidden activations are RECOMPUTED from x on the matrix cores (cheap:
// the kernel stays far from the MFMA roof) and live only in registers / LDS.
//
// One workgroup per CU, NJ = hid/32 waves; wave w owns hidden units j in [32w, 32w+32).  Per 32-token tile:
//   stash    every thread moves one 16-B chunk of x (normalised with the forward's statistics -> x-hat) and dY
//            into token-major LDS tiles (the next tile's chunks are already in flight in registers)
//   phase 1  H  = x-hat (W1 gamma)^T + b1'   and   dH = dY W2     for the wave's 32 hidden units, accumulators in the
//            NON-transposed orientation (hidden unit on the lane, tokens in the registers): after GELU / GELU'
//            they are, as they stand, the A operands of the two weight-gradient products (contraction over tokens)
//   phase 2  G1[j, c] += dHp^T x-hat,  dW2^T[j, c] += h^T dY    (x-hat / dY read transposed from the tiles, in the
//            token order the accumulator registers hold); a ones column of x-hat / a ones row of h make d(bias)
//            fall out of the same MFMAs.  The accumulators stay in registers for the whole kernel.
//   phase 3  waves 0..C/32: dX-hat^T = (W1 gamma)^T dHp^T (contraction over all hidden units: dHp goes through a
//            [hidden][token] LDS image, W1 gamma is read transposed from its one LDS image), LayerNorm backward
//            with the two row sums exchanged through LDS, + dY (the residual branch), 16-B row stores.
// The LayerNorm is handled as in linear_mfma.hip's re-cut: the kernel works on x-hat with gamma folded into W1
// and beta into the bias; the reduction forms dW1 = gamma G + beta db^T, d(gamma), d(beta) from G.
#include "linear.h"
#include "mfma.h"
#include "reduce_batch.h"
#include "wattn_hd.h"
#include <stdlib.h>

// ablation bits of the fused Mlp backward (1 no GELU-table reads, 2 no phase-1 MFMAs, 4 no phase 2, 8 no phase-3 MFMAs):
// from MlpArgs.dbg in a debug build, or fixed at compile time in a release build (-DMLP_ABL=n through tools/abl_build.sh)
#ifdef MLP_ABL
#define MLP_DBG(p) (MLP_ABL)
#else
#define MLP_DBG(p) RDST_DBGV((p).dbg)
#endif

namespace {
using namespace wahd;
using MM = Mma<bf16>;

struct MlpArgs {
  const bf16* X; int64_t ldx; const float* stats; const float* lnw; const float* lnb;
  const float* W1; const float* b1; const float* W2; const float* b2;
  const bf16* dY; int64_t lddy; bf16* dX; int64_t lddx;
  float* slab; int64_t slab_stride;   // per-workgroup partials: G1 [hid][C+1], then dW2^T [hid+1][C]
  int64_t M; int C; int hid; int64_t ntiles; int tiles_per_wg;
  unsigned long long* stamps;   // RDST_MLP_STAMPS=n (debug): [grid][16] s_memtime stamps of thread 0
  int dbg;                      // RDST_MLP_DBG (debug build): ablation bits of mlp_bwd_kernel
};

template <int NCT> struct MlpCfg {
  static constexpr int NJ = 2 * NCT, NT = 64 * NJ, CP = 32 * NCT, JP = 32 * NJ;
  static constexpr int KC = CP / 16, KJ = JP / 16, PK = CP / 8;   // PK: 16-B chunk slots per row = NT / 32
  // row strides: 80 (mod 256) for the 256-B rows of C = 120 — 272 would stack the four rows of a transposed read on
  // the same banks (see lnlin_bwd_kernel) — and still an odd number of 16-B slots for the b128 row reads
  static constexpr int LDW = NCT == 4 ? 336 : CP * 2 + 16, LDX = LDW, LDH = 64;
  static constexpr int OFF_W1 = 0, OFF_XH = OFF_W1 + JP * LDW, OFF_DY = OFF_XH + 32 * LDX, OFF_DH = OFF_DY + 32 * LDX,
                       OFF_B1 = OFF_DH + JP * LDH, OFF_SM = OFF_B1 + JP * 4, OFF_RED = OFF_SM + 32 * 4,
                       OFF_TAB = OFF_RED + NCT * 32 * 8, OFF_W2L = OFF_TAB + RDST_GELU_TAB_BYTES;
  // C = 120: the last W2L of the wave's KC W2^T packs live in LDS, not in registers (128 accumulators + 32 pack registers
  // + the tiles' fragments do not fit 256: hipcc spilled three packs and RELOADED them in every tile behind a
  // vmcnt(0), which also waits for the next tile's prefetch)
  static constexpr int W2L = NCT == 4 ? 3 : 0, SMEM = OFF_W2L + W2L * NJ * 1024;
};

// GELU(erf) for TWO elements at a time on the packed fp32 pipes (the fallback forward below): erf by Abramowitz & Stegun
// 7.1.26 as in common.h (|error| <= 1.5e-7); the coefficients carry the factor 1/2:
//   q = (1/2) erfc(|x|/sqrt2),  cdf = x >= 0 ? 1 - q : q,  pdf*sqrt(2 pi) = ex = exp(-x^2/2)
__device__ __forceinline__ void gelu_pair(f32x2 x, f32x2& cdf, f32x2& ex) {
  const f32x2 z = x * 0.70710678118654752440f;
  f32x2 az;
  az.x = __builtin_fabsf(z.x); az.y = __builtin_fabsf(z.y);
  const f32x2 den = __builtin_elementwise_fma(az, (f32x2)(0.3275911f), (f32x2)(1.0f));
  f32x2 t;
  t.x = __builtin_amdgcn_rcpf(den.x); t.y = __builtin_amdgcn_rcpf(den.y);
  f32x2 pl = __builtin_elementwise_fma(t, (f32x2)(0.5f * 1.061405429f), (f32x2)(0.5f * -1.453152027f));
  pl = __builtin_elementwise_fma(pl, t, (f32x2)(0.5f * 1.421413741f));
  pl = __builtin_elementwise_fma(pl, t, (f32x2)(0.5f * -0.284496736f));
  pl = __builtin_elementwise_fma(pl, t, (f32x2)(0.5f * 0.254829592f));
  pl = pl * t;
  const f32x2 a2 = (z * -1.4426950408889634f) * z;
  ex.x = __builtin_amdgcn_exp2f(a2.x); ex.y = __builtin_amdgcn_exp2f(a2.y);
  const f32x2 qn = pl * ex, qp = (f32x2)(1.0f) - qn;
  cdf.x = x.x >= 0.f ? qp.x : qn.x;
  cdf.y = x.y >= 0.f ? qp.y : qn.y;
}

template <int NCT, bool SPLIT>
__global__ void __launch_bounds__(128 * NCT, 2) mlp_bwd_kernel(const MlpArgs p) {
  using CF = MlpCfg<NCT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = CF::NT, JP = CF::JP, LDW = CF::LDW, LDX = CF::LDX, PK = CF::PK, NJ = CF::NJ;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, hh = lane >> 5;
  const int C = p.C, hid = p.hid;
  const int j = 32 * wave + r;   // the lane's hidden unit
  float* b1s = reinterpret_cast<float*>(smem + CF::OFF_B1);
  float* sm = reinterpret_cast<float*>(smem + CF::OFF_SM);
  float* red = reinterpret_cast<float*>(smem + CF::OFF_RED);
  const lds_cp gtab = (lds_cp)(smem + CF::OFF_TAB);
  gelu_tab_fill(smem + CF::OFF_TAB, tid, NT);   // visible after the prologue's barriers
  int nst = 0;
  auto stamp = [&]() {
    if (RDST_DBGV(p.stamps) && tid == 0 && nst < 14) p.stamps[(size_t)blockIdx.x * 16 + nst++] = __builtin_readcyclecounter();
  };
  stamp();   // 0: start

  // ---- prologue ------------------------------------------------------------------------------------
  // W2^T tile of the wave, in registers for the whole kernel: pack t, element e = W2[16t + 8hh + e][j]
  Pack16 w2b[CF::KC - CF::W2L];
  const lds_cp w2l = (lds_cp)(smem + CF::OFF_W2L + (wave * 64 + lane) * 16);   // + NJ * 1024 per pack
  {
    float f[CF::KC][8];
#pragma unroll
    for (int t = 0; t < CF::KC; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = 16 * t + 8 * hh + e;   // unconditional loads (clamped), zeroed afterwards: all of them in flight at once
        f[t][e] = p.W2[(int64_t)(c < C ? c : C - 1) * hid + (j < hid ? j : hid - 1)];
      }
#pragma unroll
    for (int t = 0; t < CF::KC; ++t) {
#pragma unroll
      for (int e = 0; e < 8; ++e) f[t][e] = (16 * t + 8 * hh + e < C && j < hid) ? f[t][e] : 0.f;
      if (t < CF::KC - CF::W2L) w2b[t < CF::KC - CF::W2L ? t : 0] = MM::pack(f[t]);
      else {   // read back by this lane only
        const Pack16 pk = MM::pack(f[t]);
        u32x4_t v; v.x = pk.w[0]; v.y = pk.w[1]; v.z = pk.w[2]; v.w = pk.w[3];
        *reinterpret_cast<LDS_AS u32x4_t*>(w2l + (t - (CF::KC - CF::W2L)) * NJ * 1024) = v;
      }
    }
  }
  stamp();   // W2 tile loaded
  lds_zero16(smem + CF::OFF_W1, CF::OFF_DH - CF::OFF_W1, tid, NT);   // W1 image and both tiles: padding rows / columns
  // W1 (hid, C) -> bf16 image of W1*gamma, and the per-pack partial dot products with beta (b1' = b1 + W1 beta)
  const int pk = tid % PK, jr = tid / PK, c0 = 8 * pk;
  {
    float gq[8], bq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {   // unconditional loads, masked afterwards
      const int c = c0 + e < C ? c0 + e : C - 1;
      gq[e] = p.lnw[c];
      bq[e] = p.lnb[c];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gq[e] = c0 + e < C ? gq[e] : 0.f;
      bq[e] = c0 + e < C ? bq[e] : 0.f;
    }
    // every pack is read as the 8 floats at min(c0, C-8) of its row and shifted down by `sh` (zeros shifted in):
    // no conditional loads, so all NJ passes are in flight together
    const int cl = c0 < C - 8 ? c0 : C - 8, sh = c0 - cl;
    float w[NJ][8];
#pragma unroll
    for (int ps = 0; ps < NJ; ++ps) {
      const int jj = jr + 32 * ps;
      const float* src = p.W1 + (int64_t)(jj < hid ? jj : hid - 1) * C + cl;
      const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(src), b = *reinterpret_cast<const u32x4_a4*>(src + 4);
      w[ps][0] = __uint_as_float(a.x); w[ps][1] = __uint_as_float(a.y); w[ps][2] = __uint_as_float(a.z); w[ps][3] = __uint_as_float(a.w);
      w[ps][4] = __uint_as_float(b.x); w[ps][5] = __uint_as_float(b.y); w[ps][6] = __uint_as_float(b.z); w[ps][7] = __uint_as_float(b.w);
    }
    if (sh != 0) {   // the row's tail pack (sh = 2, 4, 6) or a pack past the row (sh = 8)
#pragma unroll
      for (int ps = 0; ps < NJ; ++ps) {
        float t4[8], t2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t4[e] = (sh & 4) ? (e + 4 < 8 ? w[ps][e + 4 < 8 ? e + 4 : 7] : 0.f) : w[ps][e];
#pragma unroll
        for (int e = 0; e < 8; ++e) t2[e] = (sh & 2) ? (e + 2 < 8 ? t4[e + 2 < 8 ? e + 2 : 7] : 0.f) : t4[e];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[ps][e] = sh >= 8 ? 0.f : t2[e];
      }
    }
    __syncthreads();   // zero fill done
    stamp();   // W1 loads issued + zero fill
    float* part = reinterpret_cast<float*>(smem + CF::OFF_DH);
#pragma unroll
    for (int ps = 0; ps < NJ; ++ps) {
      const int jj = jr + 32 * ps;
      if (jj < hid) {
        float f[8], dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          f[e] = w[ps][e] * gq[e];
          dot = fmaf(w[ps][e], bq[e], dot);
        }
        *reinterpret_cast<Pack16*>(smem + CF::OFF_W1 + jj * LDW + c0 * 2) = MM::pack(f);
        part[jj * PK + pk] = dot;
      }
    }
    if (tid < 32) *reinterpret_cast<uint16_t*>(smem + CF::OFF_XH + tid * LDX + C * 2) = 0x3f80;   // ones column of x-hat
  }
  __syncthreads();
  stamp();   // W1 image written
  {
    const float* part = reinterpret_cast<const float*>(smem + CF::OFF_DH);
    for (int jj = tid; jj < JP; jj += NT) {
      float v = 0.f;
      if (jj < hid) {
        v = p.b1 ? p.b1[jj] : 0.f;
#pragma unroll
        for (int k = 0; k < PK; ++k) v += part[jj * PK + k];
      }
      b1s[jj] = v;
    }
  }
  __syncthreads();

  stamp();   // 1: prologue done
  // ---- the loaders' plan: 16-B chunks of x and of dY, one per thread, or (SPLIT) two per thread of waves NCT..2NCT-1
  // only.  Waves 0..NCT-1 store dX, and loads and stores share one in-order counter (vmcnt): a wave that does both
  // waits for its stores' acknowledgements before it may touch the prefetched chunks.
  constexpr int NU = SPLIT ? 2 : 1;
  const bool loader = SPLIT ? wave >= NCT : true;
  const int rowbytes = C * 2;
  int lrow[NU], loff[NU];
  bool lact[NU], lal[NU], lfirst[NU];
  const char* xp[NU];    // the thread's chunk in the current prefetch tile (advanced by 32 rows per tile)
  const char* yp[NU];
  const float* sp[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int idx = SPLIT ? (tid - 64 * NCT) + 64 * NCT * u : tid;   // 0 .. 32*PK-1
    lrow[u] = (idx / PK) & 31;
    const int chk = idx - (idx / PK) * PK;
    lact[u] = loader && chk * 16 < rowbytes;
    int o = chk * 16;
    if (o + 16 > rowbytes) o = rowbytes - 16;   // the row's last chunk overlaps its neighbour
    if (!lact[u]) o = 0;
    loff[u] = o;
    lal[u] = (o & 15) == 0;
    lfirst[u] = lact[u] && chk == 0;
  }
  u32x4_a4 rx[NU], rdy[NU];
  float2 rst[NU];
  auto seek = [&](int64_t tile) {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      int64_t row = tile * 32 + lrow[u];
      row = row < p.M ? row : p.M - 1;
      xp[u] = reinterpret_cast<const char*>(p.X + row * p.ldx) + loff[u];
      yp[u] = reinterpret_cast<const char*>(p.dY + row * p.lddy) + loff[u];
      sp[u] = p.stats + 2 * row;
    }
  };
  auto fetch = [&]() {
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      rx[u] = *reinterpret_cast<const u32x4_a4*>(xp[u]);
      rdy[u] = *reinterpret_cast<const u32x4_a4*>(yp[u]);
      rst[u] = *reinterpret_cast<const float2*>(sp[u]);
    }
  };
  const int64_t xstep = 32 * p.ldx * 2, ystep = 32 * p.lddy * 2;
  auto advance = [&]() {   // to the next tile: plain 64-bit adds (the ragged last tile is re-sought)
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      xp[u] += xstep;
      yp[u] += ystep;
      sp[u] += 64;
    }
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
    for (int u = 0; u < NU; ++u) {
      const bool valid = tile * 32 + lrow[u] < p.M;
      if (lact[u]) {
        float f[8];
        unpack8(rx[u], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = valid ? (f[e] - rst[u].x) * rst[u].y : 0.f;
        put16(smem + CF::OFF_XH + lrow[u] * LDX + loff[u], MM::pack(f), lal[u]);
        Pack16 d;
        d.w[0] = valid ? rdy[u].x : 0u; d.w[1] = valid ? rdy[u].y : 0u; d.w[2] = valid ? rdy[u].z : 0u; d.w[3] = valid ? rdy[u].w : 0u;
        put16(smem + CF::OFF_DY + lrow[u] * LDX + loff[u], d, lal[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (lfirst[u]) sm[lrow[u]] = rst[u].y;
  };

  // ---- per-lane LDS positions (loop invariant) ------------------------------------------------------------
  // Bank rules (tools/lds_banks.py; rows are an odd number of 16-B slots long for the b128 row reads): a transposed read
  // takes four rows FOUR APART (c, c+4, c+8, c+12: their 64-byte segments tile the 256-byte bank row exactly; four
  // consecutive rows overlap, 2-way), so
  //   * row i of the phase-1 MFMAs (lane r = i) is the tile's LDS row sg = sigma(i), sigma(16s + 8x + 4h + q) =
  //     16s + 4q + 2x + h: the accumulator registers of a lane half then hold LDS rows {4q + hh} and {4q + hh + 2}
  //     (+ 16s), which is what the phase-2 reads fetch; phase 3's token of lane r is sigma(r) as well;
  //   * the contraction order of phase 3 over a 16-block of hidden units is 4q + hh + 2x for W1^T, and the dHp image
  //     keeps hidden unit 16k + 4q + y at row 16k + 4y + q (consecutive rows of a 64-byte-row image ARE the exact
  //     tiling), its 8-byte pieces XOR-swizzled by (row >> 1) & 7 so that the 16 lanes of a ds_write_b64 group land on
  //     32 different banks (unswizzled: 8-way).
  const int q = (lane & 15) >> 2, pp = lane & 3, gq1 = (lane >> 4) & 1;
  const int sg = (r & 16) + 4 * (r & 3) + ((r >> 2) & 1) + 2 * ((r >> 3) & 1);
  const lds_cp xrow = (lds_cp)(smem + CF::OFF_XH + sg * LDX + hh * 16);
  const lds_cp yrow = (lds_cp)(smem + CF::OFF_DY + sg * LDX + hh * 16);
  const lds_cp wrow = (lds_cp)(smem + CF::OFF_W1 + j * LDW + hh * 16);
  const int dhpos = 32 * wave + (r & 16) + 4 * (r & 3) + ((r >> 2) & 3);          // image row of hidden unit j
  const uint32_t dho = (uint32_t)dhpos * CF::LDH + 8u * ((dhpos >> 1) & 7);        // piece P of it: dho ^ (8 P)
  const lds_cp dhb = (lds_cp)(smem + CF::OFF_DH);
  // transposed reads: rows 4q + hh (then + 2) of the tiles and of W1; rows 4hh + q (then + 8) of the dHp image
  const lds_cp xtr = (lds_cp)(smem + CF::OFF_XH + (4 * q + hh) * LDX + (16 * gq1 + 4 * pp) * 2);
  const lds_cp ytr = (lds_cp)(smem + CF::OFF_DY + (4 * q + hh) * LDX + (16 * gq1 + 4 * pp) * 2);
  const lds_cp wtr = (lds_cp)(smem + CF::OFF_W1 + (4 * q + hh) * LDW + (16 * gq1 + 4 * pp) * 2 + wave * 64);
  const lds_cp dtr0 = dhb + (4 * hh + q) * CF::LDH + 8 * ((4 * gq1 + pp) ^ ((2 * hh + (q >> 1)) & 7));
  const lds_cp dtr1 = dhb + (4 * hh + 8 + q) * CF::LDH + 8 * ((4 * gq1 + pp) ^ ((2 * hh + 4 + (q >> 1)) & 7));
  static_assert(CF::LDH == 64 && CF::OFF_DH % 64 == 0, "dHp image: 64-byte rows, XOR swizzle of the 8-byte pieces");

  f32x16 G1[NCT], W2g[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
    for (int v = 0; v < 16; ++v) { G1[ct][v] = 0.f; W2g[ct][v] = 0.f; }

  const int64_t t0 = (int64_t)blockIdx.x * p.tiles_per_wg;
  const int64_t t1 = t0 + p.tiles_per_wg < p.ntiles ? t0 + p.tiles_per_wg : p.ntiles;
  const float invC = 1.0f / (float)C;
  const int64_t full_tiles = p.M / 32;   // tiles below this index have 32 valid rows: their addresses are plain increments
  if (loader && t0 < t1) {
    seek(t0);
    fetch();
  }
  for (int64_t tile = t0; tile < t1; ++tile) {
    if (loader) {
      stash(tile);
      if (tile + 1 < t1) {   // past the end the last tile is re-read: every iteration defines the whole prefetch set
        if (tile + 1 < full_tiles) advance();
        else seek(tile + 1);
      }
      fetch();
    }
    __syncthreads();   // B1: tiles staged
    stamp();   // 2 (+4i): staged
    // ---- phase 1
    Pack16 hA[2], dA[2];
    {
      f32x16 ah, ad;
      const float bj = b1s[j];
#pragma unroll
      for (int v = 0; v < 16; ++v) { ah[v] = bj; ad[v] = 0.f; }
      if (!(MLP_DBG(p) & 2))
#pragma unroll
      for (int t = 0; t < CF::KC; ++t) {
        const Pack16 xa = lds_pack(xrow + 32 * t), wb = lds_pack(wrow + 32 * t), ya = lds_pack(yrow + 32 * t);
        MM::mma(ah, xa, wb);        // rows (registers) = tokens, columns (lanes) = hidden units
        if (t < CF::KC - CF::W2L) MM::mma(ad, ya, w2b[t < CF::KC - CF::W2L ? t : 0]);
        else MM::mma(ad, ya, lds_pack(w2l + (t - (CF::KC - CF::W2L)) * NJ * 1024));
      }
      const bool ones = j == hid;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        // GELU and GELU' from the LDS table (common.h): LB reads in flight before the first is used (8, or 4 where the
        // 128 weight-gradient accumulators of C = 120 leave no registers: a spill inside this loop costs a vmcnt(0),
        // i.e. the whole prefetch of the next tile)
        constexpr int LB = NCT == 4 ? 4 : 8;
#pragma unroll
        for (int b = 0; b < 8; b += LB) {
          float fr[LB];
          u32x2_t en[LB];
#pragma unroll
          for (int k = 0; k < LB; ++k) {
            uint32_t off;
            fr[k] = gelu_tab_index(ah[8 * s + b + k], off);
            if (MLP_DBG(p) & 1) { en[k].x = off; en[k].y = off + 1; }
            else en[k] = *reinterpret_cast<const LDS_AS u32x2_t*>(gtab + off);
          }
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int k = 0; k < LB; k += 2) {
            const int v = 8 * s + b + k;
            const float h0 = ah[v] * gelu_tab_lerp(fr[k], en[k].x), h1 = ah[v + 1] * gelu_tab_lerp(fr[k + 1], en[k + 1].x);
            const float d0 = ad[v] * gelu_tab_lerp(fr[k], en[k].y), d1 = ad[v + 1] * gelu_tab_lerp(fr[k + 1], en[k + 1].y);
            const uint32_t hp = pack_bf16x2(h0, h1);
            hA[s].w[(b + k) / 2] = ones ? 0x3f803f80u : hp;   // the ones row: d(bias) of fc2
            dA[s].w[(b + k) / 2] = pack_bf16x2(d0, d1);
          }
        }
        // dHp -> [hidden][token] image: registers 8s..8s+3 are tokens 16s+4hh.., 8s+4..8s+7 tokens 16s+8+4hh..
        u32x2_t lo, hi;
        lo.x = dA[s].w[0]; lo.y = dA[s].w[1]; hi.x = dA[s].w[2]; hi.y = dA[s].w[3];
        *reinterpret_cast<LDS_AS u32x2_t*>(dhb + (dho ^ (uint32_t)(8 * (4 * s + hh)))) = lo;
        *reinterpret_cast<LDS_AS u32x2_t*>(dhb + (dho ^ (uint32_t)(8 * (4 * s + 2 + hh)))) = hi;
      }
    }
    __syncthreads();   // B2: dHp image complete
    stamp();   // 3: phase 1 done
    // ---- phase 2: weight gradients (contraction over the tile's 32 tokens, 2 k-steps)
    if (!(MLP_DBG(p) & 4))
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const Pack16 xb = lds_tr_pack(xtr + 16 * s * LDX + ct * 64, xtr + (16 * s + 2) * LDX + ct * 64);
        const Pack16 yb = lds_tr_pack(ytr + 16 * s * LDX + ct * 64, ytr + (16 * s + 2) * LDX + ct * 64);
        MM::mma(G1[ct], dA[s], xb);    // rows = hidden units, columns = channels (column C = d(bias))
        MM::mma(W2g[ct], hA[s], yb);
      }
    // ---- phase 3: data gradient + LayerNorm backward on waves 0..NCT-1 (channel tile = wave)
    f32x16 dx;
    float rstd = 0.f;
    if (wave < NCT) {
      f32x16 dx2;   // two independent accumulation chains: only one wave per SIMD is in this phase
#pragma unroll
      for (int v = 0; v < 16; ++v) { dx[v] = 0.f; dx2[v] = 0.f; }
      if (!(MLP_DBG(p) & 8))
#pragma unroll
      for (int kk = 0; kk < CF::KJ; kk += 2) {
        const Pack16 wa = lds_tr_pack(wtr + 16 * kk * LDW, wtr + (16 * kk + 2) * LDW);
        const Pack16 db = lds_tr_pack(dtr0 + 16 * kk * CF::LDH, dtr1 + 16 * kk * CF::LDH);
        const Pack16 wa2 = lds_tr_pack(wtr + 16 * (kk + 1) * LDW, wtr + (16 * (kk + 1) + 2) * LDW);
        const Pack16 db2 = lds_tr_pack(dtr0 + 16 * (kk + 1) * CF::LDH, dtr1 + 16 * (kk + 1) * CF::LDH);
        MM::mma(dx, wa, db);   // rows = channels, columns = tokens
        MM::mma(dx2, wa2, db2);
      }
#pragma unroll
      for (int v = 0; v < 16; ++v) dx[v] += dx2[v];
      rstd = sm[sg];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const u32x2_t xv = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + CF::OFF_XH + sg * LDX) + (32 * wave + 8 * g4 + 4 * hh) * 2);
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
    __syncthreads();   // B3: row sums exchanged
    stamp();   // 4: phases 2, 3a done
    if (wave < NCT) {
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int w = 0; w < NCT; ++w) {
        const float2 v = *reinterpret_cast<const float2*>(red + (w * 32 + r) * 2);
        s1 += v.x; s2 += v.y;
      }
      s1 *= invC; s2 *= invC;
      float o[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int cb = (32 * wave + 8 * g4 + 4 * hh) * 2;
        const u32x2_t xv = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + CF::OFF_XH + sg * LDX) + cb);
        const u32x2_t yv = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + CF::OFF_DY + sg * LDX) + cb);
        const float xh[4] = {bf16lo(xv.x), bf16hi(xv.x), bf16lo(xv.y), bf16hi(xv.y)};
        const float dy[4] = {bf16lo(yv.x), bf16hi(yv.x), bf16lo(yv.y), bf16hi(yv.y)};
#pragma unroll
        for (int e = 0; e < 4; ++e) o[4 * g4 + e] = fmaf(rstd, dx[4 * g4 + e] - s1 - xh[e] * s2, dy[e]);
      }
      const int64_t row = tile * 32 + sg;   // the lane's token
      if (row < p.M) {
        bf16* drow = p.dX + row * p.lddx;
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          float c8[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[8 * gp + e]), __float_as_uint(o[8 * gp + 4 + e]), false, false);
            c8[e] = __uint_as_float(sw[0]);
            c8[4 + e] = __uint_as_float(sw[1]);
          }
          const int cb = 32 * wave + 8 * (2 * gp + hh);
          if (cb + 8 <= C) {
            u32x4_a4 u;
            u.x = pack_bf16x2(c8[0], c8[1]); u.y = pack_bf16x2(c8[2], c8[3]);
            u.z = pack_bf16x2(c8[4], c8[5]); u.w = pack_bf16x2(c8[6], c8[7]);
            *reinterpret_cast<u32x4_a4*>(drow + cb) = u;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (cb + e < C) drow[cb + e] = __float2bfloat16(c8[e]);
          }
        }
      }
    }
    __syncthreads();   // B4: tiles free for the next stash
    stamp();   // 5: stores done
  }
  if (RDST_DBGV(p.stamps) && tid == 0) p.stamps[(size_t)blockIdx.x * 16 + 14] = __builtin_readcyclecounter();   // slot 14: loop done
  // ---- epilogue: the workgroup's partial weight gradients
  // bf16 slabs in groups of 4 rows (reduce_batch.h, "G4"): the lane's 4 consecutive rows of a register group = one 8-B store.
  // region 1: G1 [hid][C+1]; region 2: dW2^T [hid+1][C] (row hid = d(b2)); p.slab_stride counts 8-byte groups
  uint2* my = reinterpret_cast<uint2*>(p.slab) + (int64_t)blockIdx.x * p.slab_stride;
  uint2* my2 = my + (int64_t)((hid + 3) / 4) * (C + 1);
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int c = 32 * ct + r;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int j0 = 32 * wave + 8 * g4 + 4 * hh;   // rows j0 .. j0 + 3
      if (j0 < hid && c <= C)
        my[(int64_t)(j0 >> 2) * (C + 1) + c] = make_uint2(pack_bf16x2(G1[ct][4 * g4], G1[ct][4 * g4 + 1]), pack_bf16x2(G1[ct][4 * g4 + 2], G1[ct][4 * g4 + 3]));
      if (j0 <= hid && c < C)
        my2[(int64_t)(j0 >> 2) * C + c] = make_uint2(pack_bf16x2(W2g[ct][4 * g4], W2g[ct][4 * g4 + 1]), pack_bf16x2(W2g[ct][4 * g4 + 2], W2g[ct][4 * g4 + 3]));
    }
  }
  if (RDST_DBGV(p.stamps) && tid == 0) p.stamps[(size_t)blockIdx.x * 16 + 15] = __builtin_readcyclecounter();   // slot 15: kernel end
}

// ---------------------------------------------------------------------------------------------------------
// Forward: y = x + fc2(GELU(fc1(LayerNorm(x)))) in one pass, the hidden activations never leave the CU.
// Same workgroup shape as the backward (wave w = hidden units 32w..32w+31, one 32-token tile per step), but in the
// TRANSPOSED orientation (token on the lane, hidden unit / channel in the registers): a lane then needs the
// LayerNorm statistics of its own token only, and the outputs leave as 16-B row stores.
//   stash    raw x chunks -> token-major LDS tile, plus per-chunk (sum, M2) partials of the row statistics
//   phase 1  H^T = (W1 gamma) x^T on the RAW rows; the lane combines its token's partials into (mean, rstd) while
//            the MFMAs run, then h = GELU(rstd (H - mean S) + b1'), S[j] = sum_c (W1 gamma)[j][c]   -> bf16 tile [token][hidden]
//   phase 2  waves 0..C/32: Y^T = W2 h^T + b2 + x (contraction over all hidden units from the LDS tile)
// The statistics (mean, rstd) are written out for the backward.
template <int NCT> struct MlpFwdCfg {
  static constexpr int NJ = 2 * NCT, NT = 64 * NJ, CP = 32 * NCT, JP = 32 * NJ;
  static constexpr int KC = CP / 16, KJ = JP / 16, PK = CP / 8;
  static constexpr int LDW = CP * 2 + 16, LDX = CP * 2 + 16, LD2 = JP * 2 + 16;
  // the W1 image holds `hid` rows and the W2 image `C` rows: the MFMAs of the last tiles read on into the next
  // region, which always holds finite bf16 data, and what they produce there meets zero weights or is not stored
  static constexpr int off_w2(int hid) { return hid * LDW; }
  static constexpr int off_x(int hid, int C) { return off_w2(hid) + C * LD2; }
  static constexpr int off_h(int hid, int C) { return off_x(hid, C) + 32 * LDX; }
  static constexpr int off_pst(int hid, int C) { return off_h(hid, C) + 32 * LD2; }
  static constexpr int off_s(int hid, int C) { return off_pst(hid, C) + 32 * 16 * 8; }
  static constexpr int smem(int hid, int C) { return off_s(hid, C) + 2 * JP * 4 + CP * 4; }
};

struct MlpFwdArgs {
  const bf16* X; int64_t ldx; const float* lnw; const float* lnb;
  const float* W1; const float* b1; const float* W2; const float* b2;
  bf16* Y; int64_t ldy; float* stats;
  int64_t M; int C; int hid; int64_t ntiles; int tiles_per_wg;
  unsigned long long* stamps;   // RDST_MLPF_STAMPS=n (debug)
};

template <int NCT>
__global__ void __launch_bounds__(128 * NCT, 2) mlp_fwd_kernel(const MlpFwdArgs p) {
  using CF = MlpFwdCfg<NCT>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NT = CF::NT, JP = CF::JP, CP = CF::CP, LDW = CF::LDW, LDX = CF::LDX, LD2 = CF::LD2, PK = CF::PK, NJ = CF::NJ;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), r = lane & 31, hh = lane >> 5;
  const int C = p.C, hid = p.hid;
  const int OFF_W2 = CF::off_w2(hid), OFF_X = CF::off_x(hid, C), OFF_H = CF::off_h(hid, C), OFF_PST = CF::off_pst(hid, C),
            OFF_S = CF::off_s(hid, C);
  float* Ss = reinterpret_cast<float*>(smem + OFF_S);   // [JP] column sums of the bf16 W1*gamma image
  float* b1s = Ss + JP;                                  // [JP] b1 + W1 beta
  float* b2s = b1s + JP;                                 // [CP]
  float2* pst = reinterpret_cast<float2*>(smem + OFF_PST);   // [32 rows][16] (sum, M2) of each 16-B chunk
  int nst = 0;
  auto stamp = [&]() {
    if (RDST_DBGV(p.stamps) && tid == 0 && nst < 16) p.stamps[(size_t)blockIdx.x * 16 + nst++] = __builtin_readcyclecounter();
  };
  stamp();

  // ---- prologue: both weight images ----
  lds_zero16(smem, OFF_H, tid, NT);   // W1, W2 images and the x tile: padding columns
  const int pk = tid % PK, jr = tid / PK, c0 = 8 * pk;
  {
    float gq[8], bq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = c0 + e < C ? c0 + e : C - 1;
      gq[e] = p.lnw[c];
      bq[e] = p.lnb[c];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gq[e] = c0 + e < C ? gq[e] : 0.f;
      bq[e] = c0 + e < C ? bq[e] : 0.f;
    }
    const int cl = c0 < C - 8 ? c0 : C - 8, sh = c0 - cl;
    float w[NJ][8];
#pragma unroll
    for (int ps = 0; ps < NJ; ++ps) {
      const int jj = jr + 32 * ps;
      const float* src = p.W1 + (int64_t)(jj < hid ? jj : hid - 1) * C + cl;
      const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(src), b = *reinterpret_cast<const u32x4_a4*>(src + 4);
      w[ps][0] = __uint_as_float(a.x); w[ps][1] = __uint_as_float(a.y); w[ps][2] = __uint_as_float(a.z); w[ps][3] = __uint_as_float(a.w);
      w[ps][4] = __uint_as_float(b.x); w[ps][5] = __uint_as_float(b.y); w[ps][6] = __uint_as_float(b.z); w[ps][7] = __uint_as_float(b.w);
    }
    if (sh != 0) {
#pragma unroll
      for (int ps = 0; ps < NJ; ++ps) {
        float t4[8], t2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t4[e] = (sh & 4) ? (e + 4 < 8 ? w[ps][e + 4 < 8 ? e + 4 : 7] : 0.f) : w[ps][e];
#pragma unroll
        for (int e = 0; e < 8; ++e) t2[e] = (sh & 2) ? (e + 2 < 8 ? t4[e + 2 < 8 ? e + 2 : 7] : 0.f) : t4[e];
#pragma unroll
        for (int e = 0; e < 8; ++e) w[ps][e] = sh >= 8 ? 0.f : t2[e];
      }
    }
    __syncthreads();   // zero fill done
    stamp();   // 1: W1 loads arrived
    // scratch for the per-pack partial dot products with beta: the h tile is free until the first phase 1
    float* part = reinterpret_cast<float*>(smem + OFF_H);
#pragma unroll
    for (int ps = 0; ps < NJ; ++ps) {
      const int jj = jr + 32 * ps;
      if (jj < hid) {
        float f[8], dot = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          f[e] = w[ps][e] * gq[e];
          dot = fmaf(w[ps][e], bq[e], dot);
        }
        *reinterpret_cast<Pack16*>(smem + jj * LDW + c0 * 2) = MM::pack(f);
        part[jj * PK + pk] = dot;
      }
    }
    stamp();   // 2: W1 image written
    // W2 (C, hid) -> bf16 image [c][hid]: thread -> (row, pack of 8) by flat index, 16-B loads where the pack is whole
    const int P2 = (hid + 7) >> 3;   // packs per row
    for (int base = tid; base < C * P2; base += NT * 4) {
      float v[4][8];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        int idx = base + NT * u;
        idx = idx < C * P2 ? idx : C * P2 - 1;
        const int c = idx / P2, pq = idx - c * P2;
        const int k0 = 8 * pq < hid - 8 ? 8 * pq : hid - 8;   // the row's tail pack: its last 8 floats, shifted below
        const float* src = p.W2 + (int64_t)c * hid + k0;
        const u32x4_a4 a = *reinterpret_cast<const u32x4_a4*>(src), b = *reinterpret_cast<const u32x4_a4*>(src + 4);
        v[u][0] = __uint_as_float(a.x); v[u][1] = __uint_as_float(a.y); v[u][2] = __uint_as_float(a.z); v[u][3] = __uint_as_float(a.w);
        v[u][4] = __uint_as_float(b.x); v[u][5] = __uint_as_float(b.y); v[u][6] = __uint_as_float(b.z); v[u][7] = __uint_as_float(b.w);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int idx = base + NT * u;
        if (idx < C * P2) {
          const int c = idx / P2, pq = idx - c * P2;
          const int k0 = 8 * pq < hid - 8 ? 8 * pq : hid - 8, s2 = 8 * pq - k0;
          float f[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float x = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) x = (k == e + s2) ? v[u][k] : x;
            f[e] = x;
          }
          *reinterpret_cast<Pack16*>(smem + OFF_W2 + c * LD2 + pq * 16) = MM::pack(f);
        }
      }
    }
  }
  __syncthreads();
  stamp();   // 3: W2 image written
  {
    const float* part = reinterpret_cast<const float*>(smem + OFF_H);
    for (int jj = tid; jj < JP; jj += NT) {
      float v = 0.f, sv = 0.f;
      if (jj < hid) {
        v = p.b1 ? p.b1[jj] : 0.f;
#pragma unroll
        for (int k = 0; k < PK; ++k) {
          v += part[jj * PK + k];
          // the row sums are those of the ROUNDED weights the MFMAs will see: read back from the image
          float fr[8];
          MM::unpack(*reinterpret_cast<const Pack16*>(smem + jj * LDW + k * 16), fr);
#pragma unroll
          for (int e = 0; e < 8; ++e) sv += fr[e];
        }
      }
      b1s[jj] = v;
      Ss[jj] = sv;
    }
    for (int c = tid; c < CP; c += NT) b2s[c] = (c < C && p.b2) ? p.b2[c] : 0.f;
  }
  __syncthreads();

  stamp();   // 4: prologue done
  // ---- loader plan: one 16-B chunk of one row of x per thread ----
  const int lrow = tid / PK, lchk = tid - lrow * PK;
  const int rowbytes = C * 2;
  const int nchunk = (rowbytes + 15) >> 4;
  const bool lact = lchk < nchunk;
  int loff = lchk * 16;
  if (loff + 16 > rowbytes) loff = rowbytes - 16;
  if (!lact) loff = 0;
  const bool lal = (loff & 15) == 0;
  const int lskip = lact ? 8 * lchk - (loff >> 1) : 0;   // leading elements of the (overlapping) last chunk that belong to its neighbour
  const float linv = 1.0f / (float)(8 - lskip);
  u32x4_a4 rx;
  const char* xp = nullptr;
  auto seek = [&](int64_t tile) {
    int64_t row = tile * 32 + lrow;
    row = row < p.M ? row : p.M - 1;
    xp = reinterpret_cast<const char*>(p.X + row * p.ldx) + loff;
  };
  const int64_t xstep = 32 * p.ldx * 2;
  auto stash = [&]() {
    if (lact) {
      Pack16 v;
      v.w[0] = rx.x; v.w[1] = rx.y; v.w[2] = rx.z; v.w[3] = rx.w;
      char* dst = smem + OFF_X + lrow * LDX + loff;
      if (lal) *reinterpret_cast<Pack16*>(dst) = v;
      else {
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        d[0] = v.w[0]; d[1] = v.w[1]; d[2] = v.w[2]; d[3] = v.w[3];
      }
      float f[8];
      unpack8(rx, f);
      float sum = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) sum += e >= lskip ? f[e] : 0.f;
      const float mi = sum * linv;
      float m2 = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = e >= lskip ? f[e] - mi : 0.f;
        m2 = fmaf(d, d, m2);
      }
      pst[lchk * 32 + lrow] = make_float2(sum, m2);   // [chunk][row]: the readers' lanes are consecutive rows
    }
  };

  const int j0 = 32 * wave;
  const lds_cp xrow = (lds_cp)(smem + OFF_X + r * LDX + hh * 16);
  const lds_cp wrow = (lds_cp)(smem + (j0 + r) * LDW + hh * 16);
  const lds_cp hwr = (lds_cp)(smem + OFF_H + r * LD2 + (j0 + 4 * hh) * 2);
  const lds_cp hrd = (lds_cp)(smem + OFF_H + r * LD2 + hh * 16);
  const lds_cp w2row = (lds_cp)(smem + OFF_W2 + (j0 + r) * LD2 + hh * 16);   // wave < NCT: channel tile = wave
  // loop invariants of the lane: S, b1' of its 16 hidden units, b2 of its 16 channels (register v <-> unit j0 + acc_row(v, hh))
  float Sr[16], B1r[16], B2r[16];
#pragma unroll
  for (int g4 = 0; g4 < 4; ++g4) {
    const float4 s4 = *reinterpret_cast<const float4*>(Ss + j0 + 8 * g4 + 4 * hh);
    const float4 b4 = *reinterpret_cast<const float4*>(b1s + j0 + 8 * g4 + 4 * hh);
    const float4 c4 = *reinterpret_cast<const float4*>(b2s + (wave < NCT ? j0 : 0) + 8 * g4 + 4 * hh);
    Sr[4 * g4] = s4.x; Sr[4 * g4 + 1] = s4.y; Sr[4 * g4 + 2] = s4.z; Sr[4 * g4 + 3] = s4.w;
    B1r[4 * g4] = b4.x; B1r[4 * g4 + 1] = b4.y; B1r[4 * g4 + 2] = b4.z; B1r[4 * g4 + 3] = b4.w;
    B2r[4 * g4] = c4.x; B2r[4 * g4 + 1] = c4.y; B2r[4 * g4 + 2] = c4.z; B2r[4 * g4 + 3] = c4.w;
  }
  const int64_t t0 = (int64_t)blockIdx.x * p.tiles_per_wg;
  const int64_t t1 = t0 + p.tiles_per_wg < p.ntiles ? t0 + p.tiles_per_wg : p.ntiles;
  const int64_t full_tiles = p.M / 32;
  const float invC = 1.0f / (float)C;
  const int nlast = C - 8 * (nchunk - 1);   // elements the row's last chunk contributes
  const float inv_nlast = 1.0f / (float)nlast;
  if (t0 < t1) {
    seek(t0);
    rx = *reinterpret_cast<const u32x4_a4*>(xp);
  }
  for (int64_t tile = t0; tile < t1; ++tile) {
    stash();
    if (tile + 1 < t1) {
      if (tile + 1 < full_tiles) xp += xstep;
      else seek(tile + 1);
    }
    rx = *reinterpret_cast<const u32x4_a4*>(xp);
    __syncthreads();   // B1: raw tile + partials staged
    stamp();
    // ---- phase 1
    {
      f32x16 ah, ah2;   // two accumulation chains
#pragma unroll
      for (int v = 0; v < 16; ++v) { ah[v] = 0.f; ah2[v] = 0.f; }
#pragma unroll
      for (int t = 0; t < CF::KC; t += 2) {
        const Pack16 wa = lds_pack(wrow + 32 * t), xb = lds_pack(xrow + 32 * t);
        const Pack16 wa2 = lds_pack(wrow + 32 * (t + 1)), xb2 = lds_pack(xrow + 32 * (t + 1));
        MM::mma(ah, wa, xb);   // rows (registers) = hidden units, columns (lanes) = tokens
        MM::mma(ah2, wa2, xb2);
      }
      // the lane's token: combine the chunk partials (Chan's formula) while the MFMAs run; each lane half takes
      // every other chunk, the halves are added by a swap
      float2 q2[PK / 2];
#pragma unroll
      for (int k = 0; k < PK / 2; ++k) q2[k] = pst[(2 * k + hh) * 32 + r];
      float sum = 0.f;
#pragma unroll
      for (int k = 0; k < PK / 2; ++k) sum += 2 * k + hh < nchunk ? q2[k].x : 0.f;
      sum = half_swap_sum(sum);
      const float mean = sum * invC;
      float m2 = 0.f;
#pragma unroll
      for (int k = 0; k < PK / 2; ++k) {
        const int kc = 2 * k + hh;
        const bool last = kc == nchunk - 1;
        const float d = q2[k].x * (last ? inv_nlast : 0.125f) - mean;
        m2 += kc < nchunk ? fmaf((last ? (float)nlast : 8.0f) * d, d, q2[k].y) : 0.f;
      }
      m2 = half_swap_sum(m2);
#pragma unroll
      for (int v = 0; v < 16; ++v) ah[v] += ah2[v];
      const float rstd = 1.0f / sqrtf(m2 * invC + 1e-5f);
      const int64_t row = tile * 32 + r;
      if (wave == 0 && hh == 0 && row < p.M) *reinterpret_cast<float2*>(p.stats + 2 * row) = make_float2(mean, rstd);
      const float nm = -mean * rstd;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const float sq[4] = {Sr[4 * g4], Sr[4 * g4 + 1], Sr[4 * g4 + 2], Sr[4 * g4 + 3]};
        const float bq[4] = {B1r[4 * g4], B1r[4 * g4 + 1], B1r[4 * g4 + 2], B1r[4 * g4 + 3]};
        float hv[4];
#pragma unroll
        for (int e2 = 0; e2 < 2; ++e2) {
          f32x2 x, cdf, ex;
          x.x = fmaf(ah[4 * g4 + 2 * e2], rstd, fmaf(nm, sq[2 * e2], bq[2 * e2]));
          x.y = fmaf(ah[4 * g4 + 2 * e2 + 1], rstd, fmaf(nm, sq[2 * e2 + 1], bq[2 * e2 + 1]));
          gelu_pair(x, cdf, ex);
          hv[2 * e2] = x.x * cdf.x;
          hv[2 * e2 + 1] = x.y * cdf.y;
        }
        u32x2_t w2;
        w2.x = pack_bf16x2(hv[0], hv[1]); w2.y = pack_bf16x2(hv[2], hv[3]);
        *reinterpret_cast<LDS_AS u32x2_t*>(hwr + 16 * g4) = w2;
      }
    }
    __syncthreads();   // B2: h tile complete
    stamp();
    // ---- phase 2: waves 0..NCT-1 (channel tile = wave)
    if (wave < NCT) {
      f32x16 y0, y1;
#pragma unroll
      for (int v = 0; v < 16; ++v) { y0[v] = B2r[v]; y1[v] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < CF::KJ; kk += 2) {
        const Pack16 wa = lds_pack(w2row + 32 * kk), hb = lds_pack(hrd + 32 * kk);
        const Pack16 wa2 = lds_pack(w2row + 32 * (kk + 1)), hb2 = lds_pack(hrd + 32 * (kk + 1));
        MM::mma(y0, wa, hb);   // rows = channels, columns = tokens
        MM::mma(y1, wa2, hb2);
      }
      float o[16];
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const u32x2_t xv = *reinterpret_cast<const LDS_AS u32x2_t*>((lds_cp)(smem + OFF_X + r * LDX) + (j0 + 8 * g4 + 4 * hh) * 2);
        const float xr[4] = {bf16lo(xv.x), bf16hi(xv.x), bf16lo(xv.y), bf16hi(xv.y)};
#pragma unroll
        for (int e = 0; e < 4; ++e) o[4 * g4 + e] = y0[4 * g4 + e] + y1[4 * g4 + e] + xr[e];
      }
      const int64_t row = tile * 32 + r;
      if (row < p.M) {
        bf16* yrow = p.Y + row * p.ldy;
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          float c8[8];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[8 * gp + e]), __float_as_uint(o[8 * gp + 4 + e]), false, false);
            c8[e] = __uint_as_float(sw[0]);
            c8[4 + e] = __uint_as_float(sw[1]);
          }
          const int cb = j0 + 8 * (2 * gp + hh);
          if (cb + 8 <= C) {
            u32x4_a4 u;
            u.x = pack_bf16x2(c8[0], c8[1]); u.y = pack_bf16x2(c8[2], c8[3]);
            u.z = pack_bf16x2(c8[4], c8[5]); u.w = pack_bf16x2(c8[6], c8[7]);
            *reinterpret_cast<u32x4_a4*>(yrow + cb) = u;
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (cb + e < C) yrow[cb + e] = __float2bfloat16(c8[e]);
          }
        }
      }
    }
    __syncthreads();   // B3: tiles free for the next stash
    stamp();
  }
}

int mlp_nct(int C, int hid) {
  const int nct = (C + 1 + 31) / 32;
  if (nct < 2 || nct > 4) return 0;
  if (hid + 1 > 64 * nct || hid < 32) return 0;
  if ((C & 1) || C * 2 < 16) return 0;
  // the forward keeps both weight images in LDS
  const int fs = nct == 2 ? MlpFwdCfg<2>::smem(hid, C) : nct == 3 ? MlpFwdCfg<3>::smem(hid, C) : MlpFwdCfg<4>::smem(hid, C);
  if (fs > 160 * 1024) return 0;
  return nct;
}

// the fused Mlp kernels (bf16 rows) cover (C, hid)
bool mlp_fused(int C, int hid) {
  static int off = -1;
  if (off < 0) {
    const char* e = rdst_dbg_getenv("RDST_MLP_V1");
    off = (e && e[0] == '1') ? 1 : 0;
  }
  return !off && mlp_nct(C, hid) != 0;
}

}  // namespace

extern "C" int rdst_mlp_fused_supported(int C, int hid, int dtype) {
  if (rdst_dtype(dtype, "rdst_mlp_fused_supported")) return 0;
  return dtype == RDST_BF16 && mlp_fused(C, hid);
}

// ---- the backward workspace: [slab][G] ---------------------------------------------------------------------------------------------
namespace {
struct MlpBwdWs {
  WsSlab slab;   // mlp_bwd per workgroup: fp32-sized rows [hid][C+1] | [hid+1][C], written as bf16 G4 groups (half the floats)
  float* G;      // [hid][C+1]: the summed region 1, for the LayerNorm finish (wgrad_ln_finish)
  size_t bytes;
};
MlpBwdWs mlp_bwd_layout(void* base, int C, int hid) {
  WsCarver c(base);
  MlpBwdWs w{};
  w.slab = ws_take_slab(c, 2 * kCUs, (int64_t)hid * (C + 1) + (int64_t)(hid + 1) * C);   // two workgroups per CU at the narrow widths
  w.G = c.take<float>((size_t)hid * (C + 1) + kWsSlackFloats);
  w.bytes = c.bytes();
  return w;
}
}  // namespace

extern "C" size_t rdst_mlp_bwd_workspace(int64_t M, int C, int hid) {
  (void)M;
  if (C <= 0 || hid <= 0) return 0;
  return mlp_bwd_layout(nullptr, C, hid).bytes;
}

extern "C" int rdst_mlp_bwd(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, const float* stats,
                            const float* W1, const float* b1, const float* W2, const void* dY, int64_t ld_dy, void* dX,
                            int64_t ld_dx, float* dW1, float* db1, float* dW2, float* db2, float* dln_w, float* dln_b,
                            void* workspace, size_t workspace_bytes, int64_t M, int C, int hid, int dtype, void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_mlp_bwd")) return rc;
  if (!X || !ln_w || !ln_b || !stats || !W1 || !W2 || !dY || !dX || !dW1 || !db1 || !dW2 || !db2 || !dln_w || !dln_b || !workspace)
    return rdst_fail(RDST_EINVAL, "rdst_mlp_bwd: null pointer");
  if (M < 0 || C <= 0 || hid <= 0 || ld_x < C || ld_dy < C || ld_dx < C) return rdst_fail(RDST_EINVAL, "rdst_mlp_bwd: bad dimensions");
  if (dtype != RDST_BF16 || !mlp_fused(C, hid)) return RDST_ENOTSUP;
  if (((uintptr_t)X & 3) || ((uintptr_t)dY & 3) || ((uintptr_t)dX & 3) || (ld_x & 1) || (ld_dy & 1) || (ld_dx & 1)) return RDST_ENOTSUP;
  if (workspace_bytes < rdst_mlp_bwd_workspace(M, C, hid)) return rdst_fail(RDST_EINVAL, "rdst_mlp_bwd: workspace too small");
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int nct = mlp_nct(C, hid);
  MlpArgs p{};
  p.X = (const bf16*)X; p.ldx = ld_x; p.stats = stats; p.lnw = ln_w; p.lnb = ln_b; p.W1 = W1; p.b1 = b1; p.W2 = W2;
  p.dY = (const bf16*)dY; p.lddy = ld_dy; p.dX = (bf16*)dX; p.lddx = ld_dx;
  p.M = M; p.C = C; p.hid = hid;
  p.ntiles = (M + 31) / 32;
  // narrow layers (4 waves, <= 256 registers in total per SIMD lane pair, 37 KB of LDS) run TWO workgroups per CU: one
  // wave per SIMD hides no latency, and two independent workgroups overlap each other's phases
  int64_t cap = nct == 2 ? 2 * kCUs : kCUs;
  { const char* e = rdst_dbg_getenv("RDST_MLP_GRID"); if (e && atoi(e) > 0) cap = atoi(e); }
  const MlpBwdWs w = mlp_bwd_layout(workspace, C, hid);
  p.slab = w.slab.p;
  // bf16 G4 slabs: (hid/4) x (C+1) groups of region 1 + (hid/4 + 1) x C groups of region 2, 8 bytes each (2 floats)
  p.slab_stride = (int64_t)((hid + 3) / 4) * (C + 1) + (int64_t)((hid + 4) / 4) * C;
  const int64_t grid = rdst_tile_grid(p.ntiles, w.slab.cap(cap, 2 * p.slab_stride), &p.tiles_per_wg);
  if (int rc = rdst_slab_fits(w.slab, grid, 2 * p.slab_stride, "mlp_bwd")) return rc;
  float* const G = w.G;
  int rc = 0;
#define RDST_MLPB(NC)                                                                                                \
  {                                                                                                                  \
    auto kern = split ? mlp_bwd_kernel<NC, true> : mlp_bwd_kernel<NC, false>;                                                                                \
    constexpr int smem = MlpCfg<NC>::SMEM;                                                                           \
    rc = rdst_launch(kern, dim3((unsigned)grid), dim3(128 * NC), smem, st, "mlp_bwd", p);                             \
  }
  static int split = -1;
  if (split < 0) { const char* e = rdst_dbg_getenv("RDST_MLP_SPLIT"); split = (e && e[0] == '1') ? 1 : 0; }
  { const char* e = rdst_dbg_getenv("RDST_MLP_DBG"); p.dbg = e ? atoi(e) : 0; }
  p.stamps = rdst_stamps_begin("RDST_MLP_STAMPS", grid, 16, st);
  if (nct == 2) RDST_MLPB(2) else if (nct == 3) RDST_MLPB(3) else RDST_MLPB(4)
#undef RDST_MLPB
  rdst_stamps_end(p.stamps, grid, 16, RDST_STAMPS_TICKS, st, "mlp_bwd C=%d hid=%d", C, hid);
  if (rc) return rc;
  const int tot = (int)p.slab_stride;
  {
    (void)tot;
    rbatch::SumJob s1{};   // region 1 -> G [hid][C+1] for the LayerNorm finish
    s1.slab = p.slab; s1.nwg = (int)grid; s1.stride = p.slab_stride; s1.g4 = 1; s1.a2 = hid; s1.b2 = C + 1;
    s1.tot = ((hid + 3) / 4) * (C + 1); s1.map = rbatch::MAP_COPY; s1.out = G;
    if (int rc = rbatch::sum(s1, st)) return rc;
    rbatch::SumJob s2{};   // region 2 -> dW2 (C, hid) transposed back, row hid -> db2
    s2.slab = p.slab + 2 * (int64_t)((hid + 3) / 4) * (C + 1); s2.nwg = (int)grid; s2.stride = p.slab_stride; s2.g4 = 1;
    s2.a2 = hid + 1; s2.b2 = C; s2.tot = ((hid + 4) / 4) * C; s2.map = rbatch::MAP_T; s2.out = dW2; s2.out2 = db2; s2.a = hid;
    if (int rc = rbatch::sum(s2, st)) return rc;
  }
  return wgrad_ln_finish_launch(G, W1, ln_w, ln_b, hid, C, 1.0f, dW1, db1, dln_w, dln_b, st);
}

extern "C" size_t rdst_mlp_fwd_workspace(int C, int hid) {
  if (C <= 0 || hid <= 0) return 16;
  return mlp3_pack_bytes(C, hid);
}
extern "C" int rdst_mlp_fwd_packable(int C, int hid, int dtype) {
  if (rdst_dtype(dtype, "rdst_mlp_fwd_packable")) return 0;
  return dtype == RDST_BF16 && mlp3_fwd_shape(C, hid);   // mlp3_mfma.hip
}

extern "C" int rdst_mlp_fwd(const void* X, int64_t ld_x, const float* ln_w, const float* ln_b, const float* W1, const float* b1,
                            const float* W2, const float* b2, void* Y, int64_t ld_y, float* stats, void* workspace,
                            size_t workspace_bytes, int64_t M, int C, int hid, int dtype, void* stream) {
  if (int rc = rdst_dtype(dtype, "rdst_mlp_fwd")) return rc;
  if (!X || !ln_w || !ln_b || !W1 || !W2 || !Y || !stats) return rdst_fail(RDST_EINVAL, "rdst_mlp_fwd: null pointer");
  if (M < 0 || C <= 0 || hid <= 0 || ld_x < C || ld_y < C) return rdst_fail(RDST_EINVAL, "rdst_mlp_fwd: bad dimensions");
  if (dtype != RDST_BF16 || !mlp_fused(C, hid)) return RDST_ENOTSUP;
  if (((uintptr_t)X & 3) || ((uintptr_t)Y & 3) || (ld_x & 1) || (ld_y & 1) || hid < 8) return RDST_ENOTSUP;
  if (M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  if (workspace && workspace_bytes >= rdst_mlp_fwd_workspace(C, hid)) {   // streaming kernel on pre-packed weights (mlp3_mfma.hip)
    const int rc = mlp3_fwd_bf16((const bf16*)X, ld_x, ln_w, ln_b, W1, b1, W2, b2, (bf16*)Y, ld_y, stats, M, C, hid, workspace,
                                 workspace_bytes == RDST_PREPACKED, st);
    if (rc != RDST_ENOTSUP) return rc;
  }
  const int nct = mlp_nct(C, hid);
  MlpFwdArgs p{};
  p.X = (const bf16*)X; p.ldx = ld_x; p.lnw = ln_w; p.lnb = ln_b; p.W1 = W1; p.b1 = b1; p.W2 = W2; p.b2 = b2;
  p.Y = (bf16*)Y; p.ldy = ld_y; p.stats = stats; p.M = M; p.C = C; p.hid = hid;
  p.ntiles = (M + 31) / 32;
  int64_t cap = nct == 2 ? 2 * kCUs : kCUs;   // the narrow layers fit two workgroups per CU (see rdst_mlp_bwd)
  { const char* e = rdst_dbg_getenv("RDST_MLP_GRID"); if (e && atoi(e) > 0) cap = atoi(e); }
  const int64_t grid = rdst_tile_grid(p.ntiles, cap, &p.tiles_per_wg);
  int rc = 0;
#define RDST_MLPF(NC)                                                                                                \
  {                                                                                                                  \
    auto kern = mlp_fwd_kernel<NC>;                                                                                  \
    const int smem = MlpFwdCfg<NC>::smem(hid, C);                                                                    \
    if (smem > 160 * 1024) return RDST_ENOTSUP;                                                                      \
    rc = rdst_launch(kern, dim3((unsigned)grid), dim3(128 * NC), smem, st, "mlp_fwd", p);                             \
  }
  p.stamps = rdst_stamps_begin("RDST_MLPF_STAMPS", grid, 16, st);
  if (nct == 2) RDST_MLPF(2) else if (nct == 3) RDST_MLPF(3) else RDST_MLPF(4)
#undef RDST_MLPF
  rdst_stamps_end(p.stamps, grid, 16, RDST_STAMPS_TICKS, st, "mlp_fwd C=%d hid=%d", C, hid);
  return rc;
}

