// K4/K5 for the E1 shapes: 3x3 / pad 1 convolution, forward and dgrad, with the WEIGHTS STATIONARY IN REGISTERS and the input
// rows rolling through LDS.  One kernel source, two arithmetics (the policy AR, first template argument):
//   C3Bf16 (conv3_mfma.hip)  : bf16 rows, one v_mfma_f32_32x32x16_bf16 per product;
//   C3X3   (conv3x_mfma.hip) : RDST_F32X3: fp32 rows, every matrix operand as two bf16 terms (hi = bf16(v), lo = bf16(v - hi)) and
//                              three MFMAs per product (lo.hi + hi.lo + hi.hi).
// The two translation units keep their policy, pack kernel, entry points and per-shape launch tables; everything a wave does is
// here, with `if constexpr (X3)` where the arithmetics differ.  THE BODY STAYS IN THE __global__ TEMPLATE: as a __device__
// function behind a thin wrapper it changed the code of every instantiation and the register counts of three.
//
// Why: the 150 -> 60 fusion conv of an RDSTB (rdst_variations.py:420-421) has 9 x 60 x 150 bf16 = 162 KB of weights —
// more than the 160 KB of LDS next to any pixel tile — so the stripe kernel of conv_mfma.hip ran two weight-chunk
// passes, re-staged (and converted, or split) the fp32 weights in every workgroup and spent most of a launch there (bf16: 110-140 us
// for 21 GFLOP; fp32x3: 226 us where this kernel's bf16 form takes 37).  A CU's register file is 512 KB.  Here a workgroup is
// 4 waves (one per SIMD, up to 512 VGPRs each): every wave keeps the A-operand fragments (32 output channels x 16 contraction
// channels per 32x32x16 MFMA) of ITS share of the weight tensor in registers for the whole kernel — loaded once, as plain 16-B
// loads, from an image that a tiny pack kernel lays out fragment-major (pack.h; fp32x3: hi / lo fragment pairs) — and LDS holds
// only input pixels:
//   * a workgroup owns a vertical strip, 32 pixels wide and SH rows high; the input rows (34 pixels with the halo,
//     K channels, pixel stride padded to an odd number of 16-B slots) roll through a ring of NR = 2 RPS + 2 row slots:
//     a step computes RPS output rows from RPS + 2 resident rows while the next RPS rows arrive by LDS-DMA in the other RPS
//     slots (no staging registers: pixels outside the image and pad slots are out-of-range offsets, which the hardware turns into
//     zeros), issued between the step's MFMAs and awaited behind them, one barrier per step.  No input row is read twice
//     inside a strip;
//   * fp32x3: the RAW fp32 pixels land in the ring; when a step's new rows have landed ONE conversion pass, shared by the four
//     waves, rewrites them in place as 64-byte groups [8 hi | 8 hi | 8 lo | 8 lo] of 16 channels; one more barrier per step;
//   * the B operand of a tap (ky, kx) is the SAME LDS image at a row / pixel offset: one ds_read_b128 (fp32x3: two) per
//     (tap, k-step) with an immediate offset, shared by the wave's NT output-channel tiles;
//   * accumulators are transposed (output channel in the registers, pixel on the lane): bias is the initial value, the scale
//     rides on the weights, residual (forward) / dX_add (dgrad) are applied to row chunks of 8 channels obtained with one
//     v_permlane32_swap per register pair, PixelShuffle(2) outputs leave as runs of 4 channels (common.py:125-136).
// Wave roles per shape (waves = CW x KSPLIT x PSLOTS = 4; a wave's share is at most 90 fragments = 360 registers):
//   bf16   150 -> 60 fwd        : CW 2 (one 32-channel tile each, 90 fragments), 2 pixel slots
//          60 -> 60 fwd / dgrad : CW 1, NT 2 (72 fragments), 4 pixel slots
//          60 -> 240 fwd + PS   : CW 4, NT 2 (72 fragments), every wave sees every pixel tile (B read once per 2 MFMAs)
//          60 -> 150 dgrad      : two launches: channels [0,128) as CW 4 x NT 1, channels [128,150) as 4 pixel slots
//          240 -> 60 dgrad      : the gradient of conv + PixelShuffle(2): contraction over k' = 60 q + c' (q = sub-pixel), read
//                                 straight from the shuffled dY (UNSHUF, no un-shuffle pass); CW 2 x KSPLIT 2 (72 / 63 fragments),
//                                 the two K halves exchange one accumulator tile each through LDS and finish one row each
//   fp32x3 150 -> 60 fwd        : CW 2 x KSPLIT 2 (hi + lo: 90 / 72 fragments)
//          60 -> 60 fwd / dgrad : CW 2, 2 pixel slots (72 fragments)
//          60 -> 240 fwd + PS   : two launches of four channel tiles, CW 4
//          60 -> 150 dgrad      : as bf16
//          240 -> 60 dgrad      : four launches of the 60 -> 60 form, one per sub-pixel, dY through a stride-2 pixel view
// Everything else (exact fp32, other channel counts, W % 32 != 0, input activation) stays on conv_mfma.hip.
#pragma once
#include "conv3_host.h"
#include "lds_dma.h"
#include "mfma.h"
#include "pack.h"

namespace {

// AR::In = { const T* A; int64_t lda; int a_bytes; } : input rows (UNSHUF: the shuffled dY (B, 2H, 2W, K/4)) and their extent in
// bytes (< 2^31): the buffer descriptor's range.  C3X3 adds the sub-pixel view ymul, yoff, xmul, xoff behind them; the kernarg
// offsets are part of the code, so the view is no member of the bf16 struct.
template <class AR>
struct C3Args : AR::In {
  const typename AR::WT* Wp;      // packed weights of this launch's channel tiles (tile 0 = channel n0)
  const float* bias;              // (N) or null
  const typename AR::T* R; int64_t ldr;   // forward residual / dgrad dX_add, output geometry; or null
  typename AR::T* Y; int64_t ldy;
  int B, H, W;                    // the conv's resolution
  int n0, N;                      // first output channel of this launch, total output channels (store mask)
  float s;
  int SH, nys, nstrips;           // strip height, strips per image column, total strips
  unsigned long long* stamps;     // debug build: [grid][8] cycle counters (AR::STAMPS), else null
};

template <class AR, int K, int CW, int NT, int KSPLIT, int PSLOTS, int RPS, bool UNSHUF, bool PSTORE>
struct C3Cfg {
  static constexpr bool X3 = AR::X3;
  static constexpr int EB = AR::EB;                        // bytes per row element
  static constexpr int KSTEPS = (K + 15) / 16;
  static constexpr int KSH = (KSTEPS + KSPLIT - 1) / KSPLIT;
  // a pixel: K bf16 channels; fp32x3: 64 bytes per 16 channels (raw fp32, then [8 hi | 8 hi | 8 lo | 8 lo])
  static constexpr int PSTRIDE = lds_odd_stride(X3 ? (K + 15) / 16 * 64 : 2 * K);
  static constexpr int SPP = PSTRIDE / 16;                 // 16-B slots per pixel
  static constexpr int RPIECES = (34 * SPP + 63) / 64;     // 1-KB LDS-DMA pieces per ring row
  static constexpr int ROWB = RPIECES * 1024;
  static constexpr int NR = 2 * RPS + 2;
  static constexpr int RPW = RPS / PSLOTS;                 // output rows per wave and step
  static constexpr int XBUF = KSPLIT > 1 ? 4 * NT * 4096 : 0;   // accumulator exchange, per wave NT tiles of 4 KB
  static constexpr int BIAS_OFF = NR * ROWB + 64;          // 64 B of zeroed slack behind the ring (k-step over-read)
  static constexpr int XBUF_OFF = BIAS_OFF + CW * NT * 32 * 4;
  static constexpr int SMEM = XBUF_OFF + XBUF;
  static constexpr int DSLOTS = (EB * K + 15) / 16;        // slots of a pixel that carry data
  static constexpr int NA_MAX = 60;                        // weight fragments kept in AGPRs (240 of the 256)
  static_assert(CW * KSPLIT * PSLOTS == 4, "4 waves");
  static_assert(RPS % PSLOTS == 0, "rows per step");
  static_assert(2 * RPS <= 16, "a strip of the smallest height is two steps");
  static_assert(!UNSHUF || !X3, "the un-shuffled dgrad of fp32 rows stays on conv_mfma.hip");
  static_assert(!UNSHUF || (K % 16 == 0), "un-shuffled rows: two sub-pixel pairs of K/2 channels, whole 16-B slots");
  static_assert(KSPLIT == 1 || RPW == 2, "the K halves exchange one row each");
};

template <class AR, int K, int CW, int NT, int KSPLIT, int PSLOTS, int RPS, bool UNSHUF, bool PSTORE>
__global__ void __launch_bounds__(256, 1) conv3_kernel(const C3Args<AR> p) {
  using CF = C3Cfg<AR, K, CW, NT, KSPLIT, PSLOTS, RPS, UNSHUF, PSTORE>;
  using T = typename AR::T;
  constexpr bool X3 = CF::X3;
  constexpr int EB = CF::EB, NP = X3 ? 2 : 1;   // NP: bf16 terms per operand
  constexpr int KSTEPS = CF::KSTEPS, KSH = CF::KSH, PSTRIDE = CF::PSTRIDE, ROWB = CF::ROWB, NR = CF::NR, RPW = CF::RPW;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = wave % CW, kh = (wave / CW) % KSPLIT, ps = wave / (CW * KSPLIT);
  const int H = p.H, W = p.W;
  RDST_PHASES_BEGIN(RDST_DBGV(p.stamps));
  // buffer descriptor of the input tensor (raw buffer, byte offsets, range = a_bytes: reads behind it return zeros), in SGPRs
  const u32x4s_t rsrc = dma_rsrc(p.A, (uint32_t)p.a_bytes);
  const uint32_t lds0 = lds_base(smem);

  lds_zero16(smem, CF::BIAS_OFF, tid, 256);
  float* biasL = reinterpret_cast<float*>(smem + CF::BIAS_OFF);
  for (int i = tid; i < CW * NT * 32; i += 256) biasL[i] = (p.bias && p.n0 + i < p.N) ? p.bias[p.n0 + i] * p.s : 0.f;
  __syncthreads();

  // ---- strips and their input rows -------------------------------------------------------------------------
  // rel row q of a strip = input row y0 - 1 + q, ring slot q % NR: the RPS + 2 rows of a step and the RPS rows of the next, which
  // land in slots no wave reads in this step.  A ring row is RPIECES LDS-DMA pieces of 1 KB
  // (buffer_load_dwordx4 ... lds: lane l of a piece fills 16-B slot l; the SOURCE address is per lane): slot -> (pixel,
  // 16-B chunk of its channel row); pad slots, pixels outside the image and the bytes behind the tensor's end are
  // out-of-range offsets of the buffer descriptor, which the hardware turns into zeros.  No staging registers, no
  // ds_write; the pieces of a row set are dealt round-robin to the 4 waves.
  const int nxs = W / 32;
  struct Strip { int b, y0, x0, nrows; };
  auto decode = [&](int strip) {
    const int xs = strip % nxs, tq = strip / nxs;
    const int ysg = tq % p.nys;
    Strip s;
    s.b = tq / p.nys; s.y0 = ysg * p.SH; s.x0 = xs * 32;
    s.nrows = (H - s.y0 < p.SH) ? H - s.y0 : p.SH;
    return s;
  };
  auto lane_off = [&](const Strip& sp, int pi) {   // byte offset of this lane's 16-B chunk inside an input row, < 0: zeros
    const int sidx = pi * 64 + lane;
    const int px = sidx / CF::SPP, sl = sidx - px * CF::SPP;
    const int x = sp.x0 - 1 + px;
    const bool ok = x >= 0 && x < W && px < 34 && sl < CF::DSLOTS;
    int off;
    if constexpr (X3) {                                  // pixel (y, x) = memory pixel (y ymul + yoff, x xmul + xoff): a sub-pixel view
      off = (x * p.xmul + p.xoff) * ((int)p.lda * 4) + sl * 16;
    } else if constexpr (UNSHUF) {
      constexpr int HS = CF::DSLOTS / 2;                 // slots per sub-pixel pair (i = 0 / 1)
      const int i2 = sl >= HS ? 1 : 0;
      off = (i2 * 2 * W + 2 * x) * ((int)p.lda * 2) + (sl - i2 * HS) * 16;
    } else {
      off = x * ((int)p.lda * 2) + sl * 16;
    }
    return ok ? off : -1;
  };
  auto dma = [&](const Strip& sp, int rel, int pi, int loff) {
    const int y = sp.y0 - 1 + rel;
    const bool rowok = y >= 0 && y < H;
    int rowbase;
    if constexpr (X3)
      rowbase = (int)((((int64_t)sp.b * (H * p.ymul) + (int64_t)y * p.ymul + p.yoff) * ((int64_t)W * p.xmul)) * (p.lda * 4));
    else
      rowbase = UNSHUF ? (int)((((int64_t)sp.b * (2 * H) + 2 * y) * (int64_t)(2 * W)) * (p.lda * 2))
                       : (int)((((int64_t)sp.b * H + y) * W) * (p.lda * 2));
    const int off = (rowok && loff >= 0) ? rowbase + loff : p.a_bytes;   // out of range -> the DMA writes zeros
    // (no wait follows: vmcnt(0) is placed by hand after a step's MFMAs, in front of the barrier that publishes the rows)
    lds_dma16(rsrc, __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)((rel % NR) * ROWB + pi * 1024)), off);
  };
  auto first_rows = [&](const Strip& sp) {           // rel rows 0 .. RPS + 1
    for (int q = wave; q < (RPS + 2) * CF::RPIECES; q += 4) {
      const int rr = q / CF::RPIECES, pi = q - rr * CF::RPIECES;
      dma(sp, rr, pi, lane_off(sp, pi));
    }
  };
  // fp32x3: the conversion pass of ring rows rel0 .. rel0 + nrel - 1 (landed, published by a barrier): raw fp32 -> hi / lo groups, in place
  [[maybe_unused]] auto convert_rows = [&](int rel0, int nrel) {
    for (int idx = tid; idx < nrel * 34 * KSTEPS; idx += 256) {
      const int rr = idx / (34 * KSTEPS), rem = idx - rr * (34 * KSTEPS), px = rem / KSTEPS, g = rem - px * KSTEPS;
      char* grp = smem + ((rel0 + rr) % NR) * ROWB + px * PSTRIDE + g * 64;
      float f[16];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(grp + 16 * q);
        // (channels past K: the tail of the pixel's last 16-byte slot belongs to the next channels of the same memory row)
        f[4 * q] = g * 16 + 4 * q < K ? v.x : 0.f; f[4 * q + 1] = g * 16 + 4 * q + 1 < K ? v.y : 0.f;
        f[4 * q + 2] = g * 16 + 4 * q + 2 < K ? v.z : 0.f; f[4 * q + 3] = g * 16 + 4 * q + 3 < K ? v.w : 0.f;
      }
      Pack16 h0, l0, h1, l1;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h0.w[e] = pack_bf16x2(f[2 * e], f[2 * e + 1]);
        l0.w[e] = pack_bf16x2(f[2 * e] - bf16lo(h0.w[e]), f[2 * e + 1] - bf16hi(h0.w[e]));
        h1.w[e] = pack_bf16x2(f[8 + 2 * e], f[9 + 2 * e]);
        l1.w[e] = pack_bf16x2(f[8 + 2 * e] - bf16lo(h1.w[e]), f[9 + 2 * e] - bf16hi(h1.w[e]));
      }
      Pack16* dst = reinterpret_cast<Pack16*>(grp);
      dst[0] = h0; dst[1] = h1; dst[2] = l0; dst[3] = l1;
    }
  };
  if ((int)blockIdx.x < p.nstrips) first_rows(decode(blockIdx.x));   // in flight together with the weight loads below

  // ---- this wave's weight fragments: registers for the whole kernel -------------------------------------------
  // The register file is 256 VGPRs + 256 AGPRs per lane; an MFMA takes its A operand from either.  Left alone, the
  // compiler keeps "spilling" fragments to AGPRs and copies each back (4 v_accvgpr_read per MFMA) under maximal
  // register pressure, which also serialises every ds_read with its MFMA.  So the first NA fragments are LOADED INTO
  // AGPRs by hand (inline asm, "=a": the value's register class is then the accumulator file and the MFMA reads it
  // there) and only the rest live in VGPRs.
  constexpr int NFR = NP * NT * 9 * KSH;   // the NP terms of every (tile, tap, k-step): f = NP * ((t * 9 + tap) * KSH + kk) + lo
  constexpr int NA = NFR < CF::NA_MAX ? NFR : CF::NA_MAX, NV = NFR - NA;
  u32x4v_t wfa[NA > 0 ? NA : 1];
  Pack16 wfv[NV > 0 ? NV : 1];
  auto wsrc = [&](int f2, bool& real) {
    const int f = X3 ? f2 >> 1 : f2, lo = X3 ? f2 & 1 : 0;
    const int t = f / (9 * KSH), rem = f - t * (9 * KSH), tap = rem / KSH, kk = rem - tap * KSH;
    const int ks = kh * KSH + kk;
    real = ks < KSTEPS;                      // the short K half pads with a zero fragment (its partner has KSH real ones)
    return reinterpret_cast<const char*>(p.Wp) + (((((int64_t)(cg * NT + t) * 9 + tap) * KSTEPS + (real ? ks : KSTEPS - 1)) * NP + lo) * 64 + lane) * 16;
  };
#pragma unroll
  for (int f = 0; f < NA; ++f) {
    bool real;
    const char* src = wsrc(f, real);
    frag_load_a(wfa[f], src);
  }
#pragma unroll
  for (int f = 0; f < NV; ++f) {
    bool real;
    const u32x4_a4 v = *reinterpret_cast<const u32x4_a4*>(wsrc(NA + f, real));
    wfv[f].w[0] = real ? v.x : 0u; wfv[f].w[1] = real ? v.y : 0u; wfv[f].w[2] = real ? v.z : 0u; wfv[f].w[3] = real ? v.w : 0u;
  }
  wait_vmcnt<0>();
#pragma unroll
  for (int f = 0; f < NA; ++f) {
    bool real;
    (void)wsrc(f, real);
    if (KSPLIT > 1 && !real) wfa[f] = u32x4v_t{0u, 0u, 0u, 0u};
    frag_pin_a(wfa[f]);         // ordered behind the wait: every use of the fragment depends on this
  }
  auto wfrag = [&](int t, int tap, int kk, int lo) {
    const int f = NP * ((t * 9 + tap) * KSH + kk) + lo;
    return f < NA ? __builtin_bit_cast(bf16x8_t, wfa[f < NA ? f : 0]) : __builtin_bit_cast(bf16x8_t, wfv[f < NA ? 0 : f - NA]);
  };
  __syncthreads();   // (the first strip's rows landed: the weight wait above covered them)
  if constexpr (X3) {
    if ((int)blockIdx.x < p.nstrips) convert_rows(0, RPS + 2);
    __syncthreads();
  }
  RDST_PHASE(RDST_DBGV(p.stamps), 0);
  for (int strip = blockIdx.x; strip < p.nstrips; strip += gridDim.x) {
    const Strip sp = decode(strip);
    const int b = sp.b, y0 = sp.y0, x0 = sp.x0, nrows = sp.nrows;
    const int nsteps = (nrows + RPS - 1) / RPS;
    if (strip != (int)blockIdx.x) {
      first_rows(sp);
      wait_vmcnt<0>();
      __syncthreads();
      if constexpr (X3) {
        convert_rows(0, RPS + 2);
        __syncthreads();
      }
    }
    // the pieces this wave loads in every step: fixed (row-in-step, piece) pairs -> their lane offsets are loop invariants
    constexpr int NPW = (RPS * CF::RPIECES + 3) / 4;
    int loff[NPW];
#pragma unroll
    for (int k = 0; k < NPW; ++k) loff[k] = lane_off(sp, (wave + 4 * k) % CF::RPIECES);
    RDST_PHASE(RDST_DBGV(p.stamps), 1);

    for (int j = 0; j < nsteps; ++j) {
      const bool more = j + 1 < nsteps;
      // residual / dX_add chunks of this step's outputs (8 channels: 16 or 32 bytes): in flight during the MFMAs
      constexpr int RFIN = KSPLIT == 2 ? 1 : RPW;           // rows this wave finishes per step
      uint32_t rpre[RFIN][NT][2][2 * EB];
      if constexpr (!PSTORE) {
        if (p.R) {
#pragma unroll
          for (int i = 0; i < RFIN; ++i) {
            const int yo = j * RPS + (KSPLIT == 2 ? kh : i) * PSLOTS + ps;
            const int yc = y0 + (yo < nrows ? yo : 0);
            const int pix = (b * H + yc) * W + x0 + r;
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
              for (int gp = 0; gp < 2; ++gp) {
                const int cb = p.n0 + (cg * NT + t) * 32 + 8 * (2 * gp + h);
                const int nv = p.N - cb;
                const T* rp = p.R + (pix * (int)p.ldr + (nv > 0 ? cb : 0));
                if constexpr (X3) {
                  if (nv >= 8) {
                    const u32x4_a4 q4 = *reinterpret_cast<const u32x4_a4*>(rp), q5 = *reinterpret_cast<const u32x4_a4*>(rp + 4);
                    rpre[i][t][gp][0] = q4.x; rpre[i][t][gp][1] = q4.y; rpre[i][t][gp][2] = q4.z; rpre[i][t][gp][3] = q4.w;
                    rpre[i][t][gp][4] = q5.x; rpre[i][t][gp][5] = q5.y; rpre[i][t][gp][6] = q5.z; rpre[i][t][gp][7] = q5.w;
                  } else {
#pragma unroll
                    for (int d = 0; d < 8; ++d) rpre[i][t][gp][d] = (d < nv) ? __float_as_uint(rp[d]) : 0u;
                  }
                } else {
                  if (nv >= 8) {
                    const u32x4_a4 q4 = *reinterpret_cast<const u32x4_a4*>(rp);
                    rpre[i][t][gp][0] = q4.x; rpre[i][t][gp][1] = q4.y; rpre[i][t][gp][2] = q4.z; rpre[i][t][gp][3] = q4.w;
                  } else {
#pragma unroll
                    for (int d = 0; d < 4; ++d) rpre[i][t][gp][d] = (2 * d + 2 <= nv) ? *reinterpret_cast<const uint32_t*>(rp + 2 * d) : 0u;
                  }
                }
              }
          }
        }
      }
      RDST_PHASE(RDST_DBGV(p.stamps), 2);

      f32x16 acc[RPW][NT];
      bool live[RPW];
#pragma unroll
      for (int i = 0; i < RPW; ++i) {
        const int yo = j * RPS + i * PSLOTS + ps;        // output row inside the strip
        live[i] = yo < nrows;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (kh == 0) {   // bias = initial accumulator: register group g4 holds channels 8 g4 + 4 h .. + 3
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const float4 bq = *reinterpret_cast<const float4*>(biasL + (cg * NT + t) * 32 + 8 * g4 + 4 * h);
              acc[i][t][4 * g4] = bq.x; acc[i][t][4 * g4 + 1] = bq.y; acc[i][t][4 * g4 + 2] = bq.z; acc[i][t][4 * g4 + 3] = bq.w;
            }
          } else {
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[i][t][v] = 0.f;
          }
        }
        if (live[i]) {
          // one B fragment (fp32x3: a hi and a lo pack) per (tap, k-step), read PD fragments ahead of the MFMA that consumes it (the
          // wave is alone on its SIMD: nothing else hides the LDS latency)
          constexpr int NSEQ = 9 * KSH, PD = (X3 && NFR > 80) ? 4 : 6, DSTEP = 3;
          const char* base[3];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky) base[ky] = smem + ((yo + ky) % NR) * ROWB + r * PSTRIDE + h * 16 + kh * (KSH * 16 * EB);
          auto rd = [&](int idx, int lo) {
            const int ky = idx / (3 * KSH), rem = idx - ky * (3 * KSH), kx = rem / KSH, kk = rem - kx * KSH;
            return *reinterpret_cast<const Pack16*>(base[ky] + kx * PSTRIDE + kk * (16 * EB) + 32 * lo);
          };
          Pack16 bq[PD], bql[X3 ? PD : 1];
#pragma unroll
          for (int u = 0; u < PD; ++u) {
            bq[u] = rd(u, 0);
            if constexpr (X3) bql[u] = rd(u, 1);
          }
#pragma unroll
          for (int idx = 0; idx < NSEQ; ++idx) {
            const int tap = idx / KSH, kk = idx - tap * KSH;
            const Pack16 cur = bq[idx % PD];
            if constexpr (X3) {
              const Pack16 curl = bql[idx % PD];
#pragma unroll
              for (int t = 0; t < NT; ++t) {
                acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag(t, tap, kk, 1), __builtin_bit_cast(bf16x8_t, cur), acc[i][t], 0, 0, 0);
                acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag(t, tap, kk, 0), __builtin_bit_cast(bf16x8_t, curl), acc[i][t], 0, 0, 0);
                acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag(t, tap, kk, 0), __builtin_bit_cast(bf16x8_t, cur), acc[i][t], 0, 0, 0);
              }
            } else {
#pragma unroll
              for (int t = 0; t < NT; ++t)
                acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wfrag(t, tap, kk, 0), __builtin_bit_cast(bf16x8_t, cur), acc[i][t], 0, 0, 0);
            }
            if (idx + PD < NSEQ) {
              bq[idx % PD] = rd(idx + PD, 0);
              if constexpr (X3) bql[idx % PD] = rd(idx + PD, 1);
            }
            // the next step's rows: one DMA piece every DSTEP MFMAs of the wave's first row, so that its issue (60-180 cycles
            // each) runs in the shadow of the matrix pipe
            if (i == 0 && idx % DSTEP == DSTEP - 1 && idx / DSTEP < NPW) {
              const int k = idx / DSTEP;
              const int q = wave + 4 * k;
              if (more && q < RPS * CF::RPIECES) {
                const int rr = q / CF::RPIECES, pi = q - rr * CF::RPIECES;
                dma(sp, (j + 1) * RPS + 2 + rr, pi, loff[k]);
              }
            }
            __builtin_amdgcn_sched_barrier(0);   // keep the read PD fragments ahead of its MFMA (the scheduler pairs them up otherwise)
          }
        }
      }

      wait_vmcnt<0>();   // the next step's rows have landed (issued >= half a step ago)
      RDST_PHASE(RDST_DBGV(p.stamps), 3);
      int fin = 0;                                        // the row (index into acc) this wave finishes
      if constexpr (KSPLIT == 2) {
        // the two K halves of a channel group hold partial sums of the same two rows: half kh gives away row 1 - kh
        // and finishes row kh
        float* xb = reinterpret_cast<float*>(smem + CF::XBUF_OFF);
        float* mine = xb + (size_t)wave * NT * 1024;
        const int partner = (ps * KSPLIT + (1 - kh)) * CW + cg;
        const float* theirs = xb + (size_t)partner * NT * 1024;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) mine[(t * 16 + v) * 64 + lane] = kh == 0 ? acc[1][t][v] : acc[0][t][v];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const float o = theirs[(t * 16 + v) * 64 + lane];
            acc[0][t][v] = (kh == 0 ? acc[0][t][v] : acc[1][t][v]) + o;
          }
        live[0] = kh == 0 ? live[0] : live[1];
        fin = kh;
      }

      RDST_PHASE(RDST_DBGV(p.stamps), 4);
      // ---- epilogue -------------------------------------------------------------------------------------------
#pragma unroll
      for (int i = 0; i < (KSPLIT == 2 ? 1 : RPW); ++i) {
        if (!live[i]) continue;
        const int yo = j * RPS + (KSPLIT == 2 ? fin : i) * PSLOTS + ps;
        const int y = y0 + yo, x = x0 + r;

#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const int cb0 = p.n0 + (cg * NT + t) * 32;      // first channel of the tile
          if constexpr (PSTORE) {
            // PixelShuffle(2): conv channel n = 4 c' + 2 i + j -> channel c' of output pixel (2y+i, 2x+j).  Register v
            // holds n = 8 (v>>2) + 4h + (v&3): for q = v & 3 the lane owns c' = 2 (v>>2) + h; one swap per register pair
            // gives each lane half 4 consecutive c' of that sub-pixel
            const int cq = cb0 / 4 + 4 * h;
            const int Co = p.N / 4;
            T* ybase = p.Y + (((b * (2 * H) + 2 * y) * (2 * W) + 2 * x) * (int)p.ldy + cq);   // (extent < 2^31 bytes)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const auto s0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][t][q]), __float_as_uint(acc[i][t][8 + q]), false, false);
              const auto s1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][t][4 + q]), __float_as_uint(acc[i][t][12 + q]), false, false);
              T* dst = ybase + ((q >> 1) * 2 * W + (q & 1)) * (int)p.ldy;
              if constexpr (X3) {
                if (cq + 4 <= Co) {
                  u32x4_a4 u;
                  u.x = s0[0]; u.y = s0[1]; u.z = s1[0]; u.w = s1[1];
                  *reinterpret_cast<u32x4_a4*>(dst) = u;
                } else if (cq + 2 <= Co) {
                  dst[0] = __uint_as_float(s0[0]); dst[1] = __uint_as_float(s0[1]);
                }
              } else {
                if (cq + 4 <= Co) {
                  u32x2_a4 u;
                  u.x = pack_bf16x2(__uint_as_float(s0[0]), __uint_as_float(s0[1]));
                  u.y = pack_bf16x2(__uint_as_float(s1[0]), __uint_as_float(s1[1]));
                  *reinterpret_cast<u32x2_a4*>(dst) = u;
                } else if (cq + 2 <= Co) {
                  *reinterpret_cast<uint32_t*>(dst) = pack_bf16x2(__uint_as_float(s0[0]), __uint_as_float(s0[1]));
                }
              }
            }
          } else {
            const int pix = (b * H + y) * W + x;   // (extents < 2^31 bytes: 32-bit element offsets)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
              float c8[8];
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[i][t][8 * gp + e]),
                                                                 __float_as_uint(acc[i][t][8 * gp + 4 + e]), false, false);
                c8[e] = __uint_as_float(sw[0]);
                c8[4 + e] = __uint_as_float(sw[1]);
              }
              const int cb = cb0 + 8 * (2 * gp + h);      // the lane's 8 consecutive channels
              const int nv = p.N - cb;                    // valid channels from cb on (N is even)
              if (nv <= 0) continue;
              if (p.R) {
                if constexpr (X3) {
#pragma unroll
                  for (int d = 0; d < 8; ++d) c8[d] += __uint_as_float(rpre[i][t][gp][d]);
                } else {
#pragma unroll
                  for (int d = 0; d < 4; ++d) { c8[2 * d] += bf16lo(rpre[i][t][gp][d]); c8[2 * d + 1] += bf16hi(rpre[i][t][gp][d]); }
                }
              }
              T* yp = p.Y + (pix * (int)p.ldy + cb);
              if constexpr (X3) {
                if (nv >= 8) {
                  u32x4_a4 u, u2;
                  u.x = __float_as_uint(c8[0]); u.y = __float_as_uint(c8[1]); u.z = __float_as_uint(c8[2]); u.w = __float_as_uint(c8[3]);
                  u2.x = __float_as_uint(c8[4]); u2.y = __float_as_uint(c8[5]); u2.z = __float_as_uint(c8[6]); u2.w = __float_as_uint(c8[7]);
                  *reinterpret_cast<u32x4_a4*>(yp) = u;
                  *reinterpret_cast<u32x4_a4*>(yp + 4) = u2;
                } else {
#pragma unroll
                  for (int d = 0; d < 8; ++d)
                    if (d < nv) yp[d] = c8[d];
                }
              } else {
                if (nv >= 8) {
                  u32x4_a4 u;
                  u.x = pack_bf16x2(c8[0], c8[1]); u.y = pack_bf16x2(c8[2], c8[3]);
                  u.z = pack_bf16x2(c8[4], c8[5]); u.w = pack_bf16x2(c8[6], c8[7]);
                  *reinterpret_cast<u32x4_a4*>(yp) = u;
                } else {
#pragma unroll
                  for (int d = 0; d < 3; ++d)
                    if (2 * d + 2 <= nv) *reinterpret_cast<uint32_t*>(yp + 2 * d) = pack_bf16x2(c8[2 * d], c8[2 * d + 1]);
                }
              }
            }
          }
        }
      }
      RDST_PHASE(RDST_DBGV(p.stamps), 5);
      __syncthreads();   // this step's reads are done; the next step's rows are published (every wave waited for its pieces above)
      if constexpr (X3) {
        if (more) {
          convert_rows((j + 1) * RPS + 2, RPS);
          __syncthreads();
        }
      }
      RDST_PHASE(RDST_DBGV(p.stamps), 6);
    }
  }
  RDST_PHASES_STORE(RDST_DBGV(p.stamps) && tid == 0, p.stamps, blockIdx.x);
}

// ctile0: the launch's first 32-channel tile (1 KB of packed weights per (tile, tap, k-step) and bf16 term)
template <class AR, int K, int CW, int NT, int KSPLIT, int PSLOTS, int RPS, bool UNSHUF, bool PSTORE>
int launch_c3(C3Args<AR>& p, int ctile0, hipStream_t st, const char* what) {
  using CF = C3Cfg<AR, K, CW, NT, KSPLIT, PSLOTS, RPS, UNSHUF, PSTORE>;
  p.Wp += (int64_t)ctile0 * 9 * CF::KSTEPS * (AR::X3 ? 2048 : 1024) / (int)sizeof(typename AR::WT);
  p.n0 = ctile0 * 32;
  Conv3Strips sp;   // (SH >= 2 RPS: C3Cfg asserts 2 RPS <= 16, so no clamp of SH to RPS is needed behind the plan)
  if (!conv3_strip_plan(p.B, p.H, p.W, 2 * RPS, 256, sp)) return RDST_ENOTSUP;
  p.SH = sp.SH; p.nys = sp.nys; p.nstrips = sp.nstrips;
  const int grid = sp.npg;
  auto kern = conv3_kernel<AR, K, CW, NT, KSPLIT, PSLOTS, RPS, UNSHUF, PSTORE>;
  p.stamps = rdst_stamps_begin(AR::STAMPS, grid, 8, st);
  const int rc = rdst_launch(kern, dim3((unsigned)grid), dim3(256), CF::SMEM, st, what, p);
  rdst_stamps_end(p.stamps, grid, 8, RDST_STAMPS_SUMS, st, "%s", what);   // 0 weights, 1 first rows, 2 dma issue, 3 mfma, 4 exchange, 5 epilogue, 6 barrier
  return rc;
}

// the larger of the forward image (K = Cin, N = Cout) and the dgrad image (K = Cout, N = Cin)
template <class AR>
size_t c3_pack_bytes(int Cin, int Cout) {
  const size_t frag = AR::X3 ? 2048 : 1024;
  const size_t f = (size_t)((Cout + 31) / 32) * 9 * ((Cin + 15) / 16) * frag;
  const size_t d = (size_t)((Cin + 31) / 32) * 9 * ((Cout + 15) / 16) * frag;
  return (f > d ? f : d) + 256;
}

inline int c3_fwd_shape(int Cin, int Cout, int ks, int r, bool has_res, int in_act) {
  if (ks != 3 || in_act) return 0;
  if (Cin == 150 && Cout == 60 && r == 1) return 1;
  if (Cin == 60 && Cout == 60 && r == 1) return 2;
  if (Cin == 60 && Cout == 240 && r == 2 && !has_res) return 3;
  return 0;
}

// The checks, the pack and the argument block both forward entry points share.  RDST_ENOTSUP = not one of the covered shapes (the
// caller falls back to conv_mfma.hip); shape = c3_fwd_shape's.
template <class AR>
int c3_fwd_args(C3Args<AR>& p, int& shape, const typename AR::T* X, int64_t ldx, int in_act, const float* Wc, const float* bias,
                const typename AR::T* R, int64_t ldr, typename AR::T* Y, int64_t ldy, const ConvGeom& g, float s, void* wpack,
                bool prepacked, hipStream_t st) {
  if (!wpack || g.pad != 1 || g.W % 32 || ((uintptr_t)wpack & 15)) return RDST_ENOTSUP;
  shape = c3_fwd_shape(g.Cin, g.Cout, g.ks, g.r, R != nullptr, in_act);
  if (!shape) return RDST_ENOTSUP;
  const int cy = g.Cout / (g.r * g.r);
  if (!conv3_rows_ok(X, ldx) || !conv3_rows_ok(Y, ldy) || (R && !conv3_rows_ok(R, ldr)) || (!AR::X3 && (cy & 1))) return RDST_ENOTSUP;
  const int64_t abytes = ((g.pixels() - 1) * ldx + g.Cin) * AR::EB;
  const int64_t opix = g.pixels() * g.r * g.r;
  if (abytes >= (1ll << 31) || opix * ldy * AR::EB >= (1ll << 31) || (R && opix * ldr * AR::EB >= (1ll << 31))) return RDST_ENOTSUP;
  typename AR::WT* wp = reinterpret_cast<typename AR::WT*>(wpack);
  if (!prepacked)
    if (int rc = AR::pack(Wc, wp, g.Cin, g.Cout, g.Cin, g.Cout, PK_FWD, s, st)) return rc;
  p.A = X; p.lda = ldx; p.a_bytes = (int)abytes; p.Wp = wp; p.bias = bias; p.R = R; p.ldr = ldr; p.Y = Y; p.ldy = ldy;
  p.B = g.B; p.H = g.H; p.W = g.W; p.N = g.Cout; p.s = s;
  return 0;
}

// ... and both dgrad entry points: dX = dX_add + s * conv^T(dY), dY in the OUTPUT geometry (pixel-shuffled when g.r == 2).  The
// caller packs the weights (the image depends on the shape).
template <class AR>
int c3_dgrad_args(C3Args<AR>& p, int& shape, const typename AR::T* dY, int64_t lddy, typename AR::T* dX, int64_t lddx,
                  const typename AR::T* acc, int64_t ldacc, int in_act, const ConvGeom& g, float s, void* wpack) {
  if (!conv3_bwd_geom_ok(g, in_act, wpack)) return RDST_ENOTSUP;
  if (!conv3_rows_ok(dY, lddy) || !conv3_rows_ok(dX, lddx) || (acc && !conv3_rows_ok(acc, ldacc))) return RDST_ENOTSUP;
  shape = conv3_bwd_shape(g.Cin, g.Cout, g.r);
  if (!shape) return RDST_ENOTSUP;
  const int64_t abytes = ((g.pixels() * g.r * g.r - 1) * lddy + g.Cout / (g.r * g.r)) * AR::EB;
  if (abytes >= (1ll << 31) || g.pixels() * lddx * AR::EB >= (1ll << 31) || (acc && g.pixels() * ldacc * AR::EB >= (1ll << 31)))
    return RDST_ENOTSUP;
  p.A = dY; p.lda = lddy; p.a_bytes = (int)abytes; p.Wp = reinterpret_cast<typename AR::WT*>(wpack); p.bias = nullptr;
  p.R = acc; p.ldr = ldacc; p.Y = dX; p.ldy = lddx;
  p.B = g.B; p.H = g.H; p.W = g.W; p.N = g.Cin; p.s = s;
  return 0;
}

}  // namespace
