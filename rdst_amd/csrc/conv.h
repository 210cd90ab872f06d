// Convolution geometry + hooks for the MFMA fast paths (conv_mfma.hip); a hook returns RDST_ENOTSUP
// when it does not cover the shape and conv.hip falls back to the generic functor GEMM.
#pragma once
#include "common.h"

struct ConvGeom {
  int B, H, W;    // input pixel grid (the conv runs at this resolution)
  int Cin, Cout;  // Cout counts channels BEFORE the pixel shuffle
  int ks, pad;
  int r;          // PixelShuffle factor folded into the output addressing (1 = none)
  __host__ __device__ __forceinline__ int64_t pixels() const { return (int64_t)B * H * W; }
  __device__ __forceinline__ void decode(int64_t p, int& b, int& y, int& x) const {
    const int hw = H * W;
    b = (int)(p / hw);
    const int q = (int)(p - (int64_t)b * hw);
    y = q / W;
    x = q - y * W;
  }
  // output row / channel of conv output channel `co` at input pixel (b,y,x):
  // nn.PixelShuffle(r): channel c*r*r + i*r + j -> channel c at (y*r+i, x*r+j)   (networks/common.py:132)
  __device__ __forceinline__ void out_rc(int b, int y, int x, int co, int64_t& row, int& c) const {
    if (r == 1) {
      row = ((int64_t)b * H + y) * W + x;
      c = co;
      return;
    }
    const int r2 = r * r;
    c = co / r2;
    const int rem = co - c * r2, i = rem / r, j = rem - i * r;
    row = ((int64_t)b * (H * r) + y * r + i) * (int64_t)(W * r) + x * r + j;
  }
};

template <typename T>
int conv_fwd_mfma(const T* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const T* R, int64_t ldr,
                  T* Y, int64_t ldy, const ConvGeom& g, float s, bool split, hipStream_t st);
// split (fp32 rows only): the RDST_F32X3 form of the kernels (common.h).
// The two backward hooks take dY as PLAIN rows (B*H*W, Cout): plain_dy() un-shuffles a pixel-shuffled
// dY into scratch once (or returns dY itself when r == 1).
template <typename T>
const T* plain_dy(const T* dY, int64_t lddy, const ConvGeom& g, void* scratch, int64_t& ld_out, hipStream_t st, int& rc);
template <typename T>
int conv_dgrad_mfma(const T* X, int64_t ldx, int in_act, const float* Wc, const T* dYp, int64_t lddyp, T* dX,
                    int64_t lddx, const T* acc, int64_t ldacc, const ConvGeom& g, float s, bool split, hipStream_t st);
template <typename T>
int conv_wgrad_mfma(const T* X, int64_t ldx, int in_act, const T* dYp, int64_t lddyp, float* dW, float* dbias,
                    const WsSlab& slab, const ConvGeom& g, float s, bool split, hipStream_t st);

// one-output-channel 3x3 conv (the tail conv) and the 1 -> 1 channel 1x1 conv (MeanShift), bf16: plain vector kernels
// (conv_c1.hip); RDST_ENOTSUP for other shapes
int conv_c1_fwd_bf16(const bf16* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const bf16* R, int64_t ldr, bf16* Y,
                     int64_t ldy, const ConvGeom& g, float s, hipStream_t st);
int conv_c1_bwd_bf16(const bf16* X, int64_t ldx, int in_act, const float* Wc, const bf16* dY, int64_t lddy, bf16* dX,
                     int64_t lddx, const bf16* acc, int64_t ldacc, float* dW, float* dbias, const WsSlab& slab, const ConvGeom& g,
                     float s, hipStream_t st, hipStream_t wst);
// the mirror shape, one INPUT channel -> Cout (the head conv on a single-channel image), bf16: forward and weight gradient
// on the same tile kernels; RDST_ENOTSUP for other shapes
int conv_in1_fwd_bf16(const bf16* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const bf16* R, int64_t ldr, bf16* Y,
                      int64_t ldy, const ConvGeom& g, float s, hipStream_t st);
int conv_in1_wgrad_bf16(const bf16* X, int64_t ldx, int in_act, const bf16* dY, int64_t lddy, float* dW, float* dbias, const WsSlab& slab,
                        const ConvGeom& g, float s, hipStream_t st);

// register-stationary 3x3 kernels for the E1 shapes, bf16 (conv3_kernel.h, entry points in conv3_mfma.hip); RDST_ENOTSUP for everything else.
// wpack: conv3_pack_bytes(Cin, Cout) bytes of 16-byte aligned device scratch (NULL -> RDST_ENOTSUP).
size_t conv3_pack_bytes(int Cin, int Cout);
int conv3_fwd_shape(int Cin, int Cout, int ks, int r, bool has_res, int in_act);   // 0 = not covered
int conv3_fwd_bf16(const bf16* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const bf16* R, int64_t ldr,
                   bf16* Y, int64_t ldy, const ConvGeom& g, float s, void* wpack, bool prepacked, hipStream_t st);
int conv3_dgrad_bf16(const float* Wc, const bf16* dY, int64_t lddy, bf16* dX, int64_t lddx, const bf16* acc, int64_t ldacc,
                     int in_act, const ConvGeom& g, float s, void* wpack, hipStream_t st);
size_t conv3_wgrad_slab_floats(int Cin, int Cout);   // per workgroup: the larger of the bf16 and the fp32x3 kernel's (conv3x_wgrad_slab_floats)
int conv3_wgrad_bf16(const bf16* X, int64_t ldx, int in_act, const bf16* dY, int64_t lddy, float* dW, float* dbias, const WsSlab& slab,
                     const ConvGeom& g, float s, hipStream_t st);

// the same kernel source on fp32 rows in the RDST_F32X3 arithmetic (entry points in conv3x_mfma.hip); wpack: conv3x_pack_bytes bytes
size_t conv3x_pack_bytes(int Cin, int Cout);
int conv3x_fwd_shape(int Cin, int Cout, int ks, int r, bool has_res, int in_act);   // 0 = not covered
int conv3x_fwd_f32(const float* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const float* R, int64_t ldr,
                   float* Y, int64_t ldy, const ConvGeom& g, float s, void* wpack, bool prepacked, hipStream_t st);
int conv3x_dgrad_f32(const float* Wc, const float* dY, int64_t lddy, float* dX, int64_t lddx, const float* acc, int64_t ldacc,
                     int in_act, const ConvGeom& g, float s, void* wpack, hipStream_t st);
int conv3x_wgrad_f32(const float* X, int64_t ldx, int in_act, const float* dY, int64_t lddy, float* dW, float* dbias, const WsSlab& slab,
                     const ConvGeom& g, float s, hipStream_t st);   // conv3x_wgrad.hip
size_t conv3x_wgrad_slab_floats(int shape);   // of conv3_bwd_shape() 1..3, 0 otherwise
// the one-channel 3x3 convolutions on fp32 rows (conv_c1x.hip: plain fp32 FMAs, both fp32 modes): tail conv wide -> 1 and head conv 1 -> wide
int conv_c1x_fwd_f32(const float* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const float* R, int64_t ldr, float* Y,
                     int64_t ldy, const ConvGeom& g, float s, hipStream_t st);
int conv_in1x_fwd_f32(const float* X, int64_t ldx, int in_act, const float* Wc, const float* bias, const float* R, int64_t ldr, float* Y,
                      int64_t ldy, const ConvGeom& g, float s, hipStream_t st);
int conv_c1x_bwd_f32(const float* X, int64_t ldx, int in_act, const float* Wc, const float* dY, int64_t lddy, float* dX, int64_t lddx,
                     const float* acc, int64_t ldacc, float* dW, float* dbias, const WsSlab& slab, const ConvGeom& g, float s, hipStream_t st);
int conv_in1x_wgrad_f32(const float* X, int64_t ldx, int in_act, const float* dY, int64_t lddy, float* dW, float* dbias, const WsSlab& slab,
                        const ConvGeom& g, float s, hipStream_t st);

// ---- the backward workspace (rdst_conv_bwd_workspace): [wpack][w3slab][slab][small][dYp][mslab][c1slab] -------------------------
// slab: every kernel above that writes one slab row per workgroup takes its region as a WsSlab of this layout, caps its grid
// by the region's rows and asks rdst_slab_fits() before it launches.
constexpr int kConvSplits = kCUs / 2;       // split-K slices of the generic weight-gradient GEMM
constexpr int kConvWgradRows = kCUs / 2;    // rows of mslab: pixel groups of conv_wgrad_mfma (x ks kernel rows in grid.y)
constexpr int kC1Rows = 4 * kCUs;           // partial rows of the one-channel kernels' slab (bf16; the fp32 ones write kCUs); + the reduced row
struct ConvBwdWs {
  void* wpack;      // the data gradient's packed weights (conv3_dgrad_bf16 / conv3x_dgrad_f32): room for the hi / lo image
  WsSlab w3slab;    // conv3_wgrad_bf16, conv3x_wgrad_f32 (3x3 only)
  WsSlab slab;      // [Cout][Cin][taps] slices of the generic split-K GEMM
  WsSlab small;     // colsum rows [Cout]
  void* dYp;        // dY as plain rows where the call has a PixelShuffle (plain_dy)
  WsSlab mslab;     // conv_wgrad_mfma: [ks][Cout][ks][CinP] per pixel group
  WsSlab c1slab;    // the one-channel kernels: rows of 9 Cin + 1 (tail conv) or 10 Cout (head conv) floats, fp32 rows one float wider
  size_t bytes;
};
// r: the call's PixelShuffle factor; the size query asks with r = 2 (room for an un-shuffled dY, bf16 or fp32)
inline ConvBwdWs conv_bwd_layout(void* base, int B, int H, int W, int Cin, int Cout, int ks, int r) {
  WsCarver c(base);
  ConvBwdWs w{};
  const int64_t taps = (int64_t)ks * ks, CinP = (Cin + 1 + 31) / 32 * 32;
  w.wpack = c.take<char>(conv3x_pack_bytes(Cin, Cout));
  w.w3slab = ws_take_slab(c, ks == 3 ? kCUs : 0, conv3_wgrad_slab_floats(Cin, Cout));
  c.take<float>(ks == 3 ? kWsSlackFloats : 0);
  w.slab = ws_take_slab(c, kConvSplits, taps * Cout * Cin);
  w.small = ws_take_slab(c, kSmallBlocks, Cout);
  c.take<float>(kWsSlackFloats);
  const size_t unsh = (size_t)B * H * W * Cout * 4;
  w.dYp = c.take<char>(r > 1 ? unsh : 0);
  w.mslab = ws_take_slab(c, kConvWgradRows, taps * Cout * CinP);
  c.take<float>(kWsSlackFloats);
  c.take<char>(r > 1 ? 0 : unsh);   // (without a shuffle mslab starts where dYp would: the room stays, the one-channel slab does not move)
  // two users: bf16 kernels (kC1Rows + 1 rows) and fp32 kernels (kCUs + 1 rows, one float wider): the larger need
  const int64_t wide = Cin == 1 ? Cout : Cin, row = Cin == 1 ? 10 * wide : 9 * wide + 1;
  const size_t need16 = (size_t)(kC1Rows + 1) * row, need32 = (size_t)(kCUs + 1) * (10 * wide + 1);
  w.c1slab = WsSlab{c.take<float>(need16 > need32 ? need16 : need32), kC1Rows + 1, row};
  w.bytes = c.bytes();
  return w;
}
