// LDS-DMA (buffer_load ... lds), hand-placed waits, compiler-invisible fragment loads and the LDS row-stride rules: the
// idioms the streaming kernels (lin3*, mlp3, lnlin3*, conv3*, swinattn_fwd, wattn_bwd_pair) share, written down once.
#pragma once
#include "common.h"

// ---- LDS-DMA ---------------------------------------------------------------------------------------------------------
// A piece is 1 KB: lane l of the issuing wave fills the 16-byte LDS slot l behind the (wave-uniform) destination from its OWN
// source offset.  The source is a raw buffer descriptor with byte offsets and range = `bytes`: an offset at or behind the
// range reads as zeros, which is how rows past the end, pad slots and halo pixels are filled without a branch.
typedef uint32_t u32x4s_t __attribute__((ext_vector_type(4)));   // a buffer descriptor: lives in SGPRs

__device__ __forceinline__ u32x4s_t dma_rsrc(const void* ptr, uint32_t bytes) {
  u32x4s_t q;
  q.x = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)ptr);
  q.y = __builtin_amdgcn_readfirstlane((uint32_t)((uintptr_t)ptr >> 32) & 0xffffu);
  q.z = __builtin_amdgcn_readfirstlane(bytes);
  q.w = 0x00020000u;
  return q;
}

// LDS byte address of a __shared__ pointer (what M0 / ds instructions take)
__device__ __forceinline__ uint32_t lds_base(const void* smem) {
  return (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
}

// One piece: 16 bytes per lane from byte offset `off` of `rs` to LDS slot lane of `lds_dst` (wave-uniform, in an SGPR:
// pass it through readfirstlane).
// Inline asm, not the builtin: the compiler orders every later ds_read behind a builtin LDS-DMA with s_waitcnt
// vmcnt(0) (it cannot tell that the slots differ), which exposes the whole HBM latency in every step.  The waits are
// placed by hand (wait_vmcnt below), in front of the barrier that publishes the piece.  The destination travels in M0,
// where the compiler may hold a value of its own: M0 is saved and restored around the load.
// RESCALAR: make the descriptor scalar again at the point of use (under SGPR pressure it otherwise arrives in vector
// registers, which the instruction cannot take).
template <bool RESCALAR = false>
__device__ __forceinline__ void lds_dma16(const u32x4s_t& rs0, uint32_t lds_dst, int off) {
  uint32_t keep;
  u32x4s_t rs = rs0;
  if constexpr (RESCALAR) {
    rs.x = __builtin_amdgcn_readfirstlane(rs0.x); rs.y = __builtin_amdgcn_readfirstlane(rs0.y);
    rs.z = __builtin_amdgcn_readfirstlane(rs0.z); rs.w = __builtin_amdgcn_readfirstlane(rs0.w);
  }
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(off), "s"(lds_dst), "s"(rs) : "memory");
}

// Counted wait: at most N of this wave's vector-memory operations (they retire in issue order) are still in flight.  The
// count is an instruction immediate (6 bits).
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- weight fragments the compiler must not see as loads -----------------------------------------------------------------
// A 16-byte fragment per lane from `src` (+ OFFSET, an instruction immediate; %c prints it in decimal), into a VGPR quad or straight into AGPRs (an
// MFMA reads its A operand from either file).  Were these plain loads, the compiler would drain the whole queue (vmcnt(0)) at
// the first use and with it every tile in flight; so the load is opaque, and after the hand-placed wait that covers it
// frag_pin / frag_pin_a makes every later use depend on a point behind that wait.
typedef uint32_t u32x4v_t __attribute__((ext_vector_type(4)));   // a fragment: 8 bf16 per lane

template <int OFFSET = 0>
__device__ __forceinline__ void frag_load(u32x4v_t& dst, const void* src) {
  if constexpr (OFFSET == 0) asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(dst) : "v"(src) : "memory");
  else asm volatile("global_load_dwordx4 %0, %1, off offset:%c2" : "=v"(dst) : "v"(src), "n"(OFFSET) : "memory");
}
__device__ __forceinline__ void frag_load_a(u32x4v_t& dst, const void* src) {
  asm volatile("global_load_dwordx4 %0, %1, off" : "=a"(dst) : "v"(src) : "memory");
}
template <typename T> __device__ __forceinline__ void frag_pin(T& a) { asm volatile("" : "+v"(a)); }
template <typename T> __device__ __forceinline__ void frag_pin(T& a, T& b) { asm volatile("" : "+v"(a), "+v"(b)); }
template <typename T> __device__ __forceinline__ void frag_pin_a(T& a) { asm volatile("" : "+a"(a)); }

// ---- LDS row strides (bytes) ------------------------------------------------------------------------------------------------
// Rows read with ds_read_b128 (one row per lane): >= bytes, a multiple of 16 with an ODD number of 16-byte slots, so that the
// 16 rows of a lane group land on distinct 16-byte slots of the 256-byte bank row.
__host__ __device__ constexpr int lds_odd_stride(int bytes) {
  int s = (bytes + 15) / 16 * 16;
  if (((s / 16) & 1) == 0) s += 16;
  return s;
}
// Rows of K bf16 read in whole 32-byte k-steps: the stride covers every k-step, so no read leaves the row.
__host__ __device__ constexpr int lds_kstep_stride(int K) { return lds_odd_stride((K + 15) / 16 * 32); }
// Rows read transposed (ds_read_b64_tr_b16): >= bytes, = 64 or 192 (mod 256), so that the four rows of a transposed read fall
// on the four 64-byte quarters of the bank row.
__host__ __device__ constexpr int lds_tr_stride(int bytes) {
  int s = (bytes + 63) / 64 * 64;
  while ((s % 256) != 64 && (s % 256) != 192) s += 64;
  return s;
}
// Planes of `cols` bf16 that are written in 8-byte row slices and read transposed (lnlin3 / lnlin3x): the row plus one pad
// slot, an odd 16-byte slot count, not 16..47 (mod 256).
__host__ __device__ constexpr int lds_plane_stride(int cols) {
  const int b = cols * 2 + 16;
  return (b & 255) < 48 ? b + 64 : b;
}
__host__ __device__ constexpr int ce_gcd(int a, int b) { return b == 0 ? a : ce_gcd(b, a % b); }
