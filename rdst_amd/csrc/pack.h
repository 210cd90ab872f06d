// Weight packing for the register-stationary kernels (lin3_mfma.hip, conv3_kernel.h): the device bodies, shared by the
// per-call pack kernels and by the batched one (pack_batch.hip: every layer of a network in a handful of launches).
#pragma once
#include "common.h"
#include "mfma.h"

constexpr int PK_FWD = 0, PK_DGRAD = 1, PK_DGRAD_UNSHUF = 2;

// ---- lane level: a thread packs the 8 values of lane (r, h) of one fragment: output n = 32 tile + r, contraction k = k0 + e,
// k0 = 16 ks + 8 h.  One gather per layer kind, one store per arithmetic. ----

// Linear: W[n][k] gamma[k] s (zeros for a pad row and for k >= K)
__device__ __forceinline__ void lin_pack_gather(float (&v)[8], const float* __restrict__ W, const float* __restrict__ gamma, int n,
                                                bool row, int k0, int K, float s) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    v[e] = (row && k < K) ? W[(int64_t)n * K + k] * (gamma ? gamma[k] : 1.f) * s : 0.f;
  }
}

// 3x3 convolution, tap = 3 ky + kx (zeros for n >= N and k >= K); out_scale rides on the weights: (conv(W) + bias) s = conv(s W) + s bias
//   PK_FWD          : Wc[n][k][tap]
//   PK_DGRAD        : Wc[cmul k + coff][n][8 - tap]           (contraction over co, mirrored tap; (cmul, coff) = (4, q): the
//                                                              sub-pixel slice q of conv + PixelShuffle(2))
//   PK_DGRAD_UNSHUF : Wc[4 c' + q][n][8 - tap], k = 60 q + c' (conv channel 4c'+q is sub-pixel q of channel c'); compiled only with
//                     UNSHUF (the bf16 image): without it every mode but PK_FWD is PK_DGRAD
template <bool UNSHUF>
__device__ __forceinline__ void conv_pack_gather(float (&v)[8], const float* __restrict__ Wc, int Cin, int Cout, int n, int N, int k0,
                                                 int K, int tap, int mode, float s, int cmul, int coff) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e;
    float x = 0.f;
    if (n < N && k < K) {
      if (mode == PK_FWD) x = Wc[((int64_t)n * Cin + k) * 9 + tap];
      else if (!UNSHUF || mode == PK_DGRAD) x = Wc[((int64_t)(cmul * k + coff) * Cin + n) * 9 + (8 - tap)];
      else {
        const int cq = Cout / 4, q = k / cq, c = k - q * cq;
        x = Wc[((int64_t)(4 * c + q) * Cin + n) * 9 + (8 - tap)];
      }
    }
    v[e] = x * s;
  }
}

// bf16 image: fragment f = 64 lanes x 8 bf16 (1 KB); i = 64 f + lane
__device__ __forceinline__ void pack_store_bf16(bf16* __restrict__ img, int64_t i, const float (&v)[8]) {
  u32x4_a4 o;
  o.x = pack_bf16x2(v[0], v[1]); o.y = pack_bf16x2(v[2], v[3]); o.z = pack_bf16x2(v[4], v[5]); o.w = pack_bf16x2(v[6], v[7]);
  *reinterpret_cast<u32x4_a4*>(img + i * 8) = o;
}
// RDST_F32X3 image: every value as TWO bf16 terms, hi = bf16(w), lo = bf16(w - hi); fragment f = [hi: 64 lanes x 8 bf16][lo: the same] (2 KB)
__device__ __forceinline__ void pack_store_hilo(uint32_t* __restrict__ img, int f, int lane, const float (&v)[8]) {
  u32x4_a4 hi, lo;
  uint32_t* ph = reinterpret_cast<uint32_t*>(&hi);
  uint32_t* pl = reinterpret_cast<uint32_t*>(&lo);
#pragma unroll
  for (int e2 = 0; e2 < 4; ++e2) {
    ph[e2] = pack_bf16x2(v[2 * e2], v[2 * e2 + 1]);
    pl[e2] = pack_bf16x2(v[2 * e2] - bf16lo(ph[e2]), v[2 * e2 + 1] - bf16hi(ph[e2]));
  }
  uint32_t* dst = img + ((int64_t)f * 128 + lane) * 4;
  *reinterpret_cast<u32x4_a4*>(dst) = hi;
  *reinterpret_cast<u32x4_a4*>(dst + 256) = lo;
}

// The row pass of a Linear image, one wave per output row n (coalesced row reads, fixed shuffle tree): S = sum_k of the rounded
// bf16 values (WITH_S: the bf16 kernels fold LayerNorm's mean through it), bb = b'[n] = (bias[n] + sum_k W[n][k] beta[k]) s; zeros
// for a pad row.
template <bool WITH_S>
__device__ __forceinline__ void lin_pack_row(const float* __restrict__ W, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             const float* __restrict__ bias, int n, bool row, int K, float s, float& S, float& bb) {
  const int lane = threadIdx.x & 63;
  S = 0.f;
  bb = 0.f;
  if (!row) return;
  if (WITH_S || beta)
    for (int k = lane; k < K; k += 64) {
      const float w = W[(int64_t)n * K + k];
      if (WITH_S) S += __bfloat162float(__float2bfloat16(w * (gamma ? gamma[k] : 1.f) * s));
      if (beta) bb = fmaf(w, beta[k], bb);
    }
  if (WITH_S) S = wave_sum(S);
  bb = wave_sum(bb);
  bb = (bb + (bias ? bias[n] : 0.f)) * s;
}

// ---- block level: the bodies of the pack kernels.  Blocks [0, nb1): one thread per (fragment, lane); Linear images: the blocks
// behind them run the row pass, 4 rows each. ----

// Linear, bf16: fragment (nt, ks).  sb[0][n] = S[n], sb[1][n] = b'[n].
__device__ __forceinline__ void lin3_pack_block(int bid, const float* __restrict__ W, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ bias,
                                                        bf16* __restrict__ wp, float* __restrict__ sb, int N, int K, int ksteps,
                                                        int ntiles, float s) {
  const int nfr = ntiles * ksteps * 64, nb1 = (nfr + 255) / 256;
  if (bid < nb1) {
    const int i = bid * 256 + threadIdx.x;
    if (i >= nfr) return;
    const int lane = i & 63, f = i >> 6;
    const int ks = f % ksteps, nt = f / ksteps;
    const int n = nt * 32 + (lane & 31);
    float v[8];
    lin_pack_gather(v, W, gamma, n, n < N, ks * 16 + (lane >> 5) * 8, K, s);
    pack_store_bf16(wp, i, v);
    return;
  }
  const int n = (bid - nb1) * 4 + (threadIdx.x >> 6);
  const int NP = ntiles * 32;
  if (n >= NP) return;
  float S, bb;
  lin_pack_row<true>(W, gamma, beta, bias, n, n < N, K, s, S, bb);
  if ((threadIdx.x & 63) == 0) {
    sb[n] = S;
    sb[NP + n] = bb;
  }
}


// The same image for a Linear whose N outputs are `nsec` equal SECTIONS (qkv: q | k | v, N = 3 C), each padded to whole
// 32-row tiles of its own: tile nt = sec * spt + j holds outputs sec * Cs + 32 j + r (zero rows where 32 j + r >= Cs), so a
// tile never straddles two sections and the consumer (swinattn_fwd.hip) writes each tile into one LDS section.
// sb[0][32 nt + r] = S, sb[1][32 nt + r] = b' of that output (0 for the pad rows).
__device__ __forceinline__ void lin3sec_pack_block(int bid, const float* __restrict__ W, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, const float* __restrict__ bias,
                                                   bf16* __restrict__ wp, float* __restrict__ sb, int N, int K, int nsec, float s) {
  const int Cs = N / nsec, spt = (Cs + 31) / 32, ntiles = nsec * spt, ksteps = (K + 15) / 16;
  const int nfr = ntiles * ksteps * 64, nb1 = (nfr + 255) / 256;
  if (bid < nb1) {
    const int i = bid * 256 + threadIdx.x;
    if (i >= nfr) return;
    const int lane = i & 63, f = i >> 6;
    const int ks = f % ksteps, nt = f / ksteps;
    const int sec = nt / spt, c = (nt - sec * spt) * 32 + (lane & 31);
    float v[8];
    lin_pack_gather(v, W, gamma, sec * Cs + c, c < Cs, ks * 16 + (lane >> 5) * 8, K, s);
    pack_store_bf16(wp, i, v);
    return;
  }
  const int np = (bid - nb1) * 4 + (threadIdx.x >> 6);   // padded output index
  const int NP = ntiles * 32;
  if (np >= NP) return;
  const int nt = np >> 5, sec = nt / spt, c = (nt - sec * spt) * 32 + (np & 31);
  float S, bb;
  lin_pack_row<true>(W, gamma, beta, bias, sec * Cs + c, c < Cs, K, s, S, bb);
  if ((threadIdx.x & 63) == 0) {
    sb[np] = S;
    sb[NP + np] = bb;
  }
}
static __host__ __device__ inline int lin3sec_tiles(int N, int nsec) { return nsec * ((N / nsec + 31) / 32); }
static inline int lin3sec_pack_blocks(int K, int N, int nsec) {
  const int nt = lin3sec_tiles(N, nsec), ks = (K + 15) / 16;
  return (nt * ks * 64 + 255) / 256 + (nt * 32 + 3) / 4;
}
static __host__ __device__ inline size_t lin3sec_pack_bytes(int K, int N, int nsec) {
  const int nt = lin3sec_tiles(N, nsec), ks = (K + 15) / 16;
  return (size_t)nt * ks * 1024 + (size_t)2 * nt * 32 * 4 + 256;
}


// Linear, RDST_F32X3 (lin3x_mfma.hip): fragment (nt, ks) as a hi / lo pair.  Behind the fragments: b'[32 nt + r] (fp32; 0 for the
// pad rows).  The kernels that read it normalise the rows BEFORE the product (x-hat = (x - mean) rstd, split into hi + lo), so
// no S[n] term exists.
__device__ __forceinline__ void lin3x_pack_block(int bid, const float* __restrict__ W, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, const float* __restrict__ bias, uint32_t* __restrict__ wp,
                                                 float* __restrict__ bp, int N, int K, int ksteps, int ntiles, float s) {
  const int nfr = ntiles * ksteps * 64, nb1 = (nfr + 255) / 256;
  if (bid < nb1) {
    const int i = bid * 256 + threadIdx.x;
    if (i >= nfr) return;
    const int lane = i & 63, f = i >> 6;
    const int ks = f % ksteps, nt = f / ksteps;
    const int n = nt * 32 + (lane & 31);
    float v[8];
    lin_pack_gather(v, W, gamma, n, n < N, ks * 16 + (lane >> 5) * 8, K, s);
    pack_store_hilo(wp, f, lane, v);
    return;
  }
  const int n = (bid - nb1) * 4 + (threadIdx.x >> 6);
  if (n >= ntiles * 32) return;
  float S, bb;
  lin_pack_row<false>(W, gamma, beta, bias, n, n < N, K, s, S, bb);
  if ((threadIdx.x & 63) == 0) bp[n] = bb;
}
static inline int lin3_pack_blocks(int K, int N) {
  const int nt = (N + 31) / 32, ks = (K + 15) / 16;
  return (nt * ks * 64 + 255) / 256 + (nt * 32 + 3) / 4;
}
static inline int lin3x_pack_blocks(int K, int N) { return lin3_pack_blocks(K, N); }
static __host__ __device__ inline size_t lin3x_pack_bytes(int K, int N) {
  const int nt = (N + 31) / 32, ks = (K + 15) / 16;
  return (size_t)nt * ks * 2048 + (size_t)nt * 32 * 4 + 256;
}


// 3x3 convolution (conv3_kernel.h): fragment (ct, tap, ks), bf16 with the three PK_ modes / as a hi / lo pair with PK_FWD and
// PK_DGRAD, the latter through conv_pack_gather's (cmul, coff).
__device__ __forceinline__ void conv3_pack_block(int bid, const float* __restrict__ Wc, bf16* __restrict__ out, int Cin,
                                                         int Cout, int K, int N, int ksteps, int ctiles, int mode, float s) {
  const int i = bid * 256 + threadIdx.x;
  if (i >= ctiles * 9 * ksteps * 64) return;
  const int lane = i & 63, f = i >> 6;
  const int ks = f % ksteps, tap = (f / ksteps) % 9, ct = f / (ksteps * 9);
  float v[8];
  conv_pack_gather<true>(v, Wc, Cin, Cout, ct * 32 + (lane & 31), N, ks * 16 + (lane >> 5) * 8, K, tap, mode, s, 1, 0);
  pack_store_bf16(out, i, v);
}
__device__ __forceinline__ void conv3x_pack_block(int bid, const float* __restrict__ Wc, uint32_t* __restrict__ out, int Cin, int Cout,
                                                  int K, int N, int ksteps, int ctiles, int mode, float s, int cmul = 1, int coff = 0) {
  const int i = bid * 256 + threadIdx.x;
  if (i >= ctiles * 9 * ksteps * 64) return;
  const int lane = i & 63, f = i >> 6;
  const int ks = f % ksteps, tap = (f / ksteps) % 9, ct = f / (ksteps * 9);
  float v[8];
  conv_pack_gather<false>(v, Wc, Cin, Cout, ct * 32 + (lane & 31), N, ks * 16 + (lane >> 5) * 8, K, tap, mode, s, cmul, coff);
  pack_store_hilo(out, f, lane, v);
}
static inline int conv3_pack_blocks(int K, int N) {
  const int ks = (K + 15) / 16, ct = (N + 31) / 32;
  return (ct * 9 * ks * 64 + 255) / 256;
}
static inline int conv3x_pack_blocks(int K, int N) { return conv3_pack_blocks(K, N); }
