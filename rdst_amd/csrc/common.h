// Shared helpers for the gfx950 kernels of librdst_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <initializer_list>
#include "../../include/rdst_hip.h"
#include "workspace.h"

typedef __hip_bfloat16 bf16;

// One workgroup per CU on this part (MI355X: 256 CUs): the unit of every persistent grid cap and of every per-workgroup slab
// region's row count.  Nothing queries the device; a port to another part changes the grids here and nowhere else.
constexpr int kCUs = 256;
// rows of the `small` regions of the Linear and conv backward workspaces (column sums, LayerNorm d(gamma) / d(beta) partials)
constexpr int kSmallBlocks = 2 * kCUs;
// floats kept free behind some regions of the backward workspaces: no kernel writes them, the totals have always held them
constexpr int kWsSlackFloats = 64;

// Ablation switches, in-kernel cycle stamps and environment overrides exist only in a -DRDST_DEBUG build
// (RDST_BUILD_DEBUG=1 python -m rdst_amd.build; tools/ use it).  In the shipped library RDST_DBGV(x) is the
// constant 0 and rdst_dbg_getenv() a constant null pointer, so every `if (RDST_DBGV(p.dbg) & 2)` /
// `if (RDST_DBGV(p.stamps) && ...)` branch and every `e ? atoi(e) : dflt` folds away at compile time: no
// getenv, hipMalloc or host sync in a launcher, no ablation test inside a kernel loop.
enum { RDST_STAMPS_SUMS = 0, RDST_STAMPS_TICKS = 1 };   // what a kernel keeps in its stamp slots: rdst_stamps_end()
#ifdef RDST_DEBUG
#include <stdlib.h>
#define RDST_DBGV(x) (x)
static inline const char* rdst_dbg_getenv(const char* name) { return getenv(name); }
// per-workgroup cycle counters of a kernel (debug build only): while `env` is set to a positive number every launch is
// armed; the launcher passes the returned device buffer ([grid][n] u64, zeroed) to the kernel and calls rdst_stamps_end()
// after the launch, which synchronises and prints one summary over the workgroups, headed by the printf-style tag.
//   RDST_STAMPS_SUMS   the kernel ACCUMULATES cycles in its slots (RDST_PHASES_*): the mean of every slot
//   RDST_STAMPS_TICKS  the kernel writes the cycle counter itself into slot after slot (0 = never reached): per slot, over
//                      the workgroups that reached it, the mean distance to the slot before it and to slot 0
static inline unsigned long long* rdst_stamps_begin(const char* env, int64_t grid, int n, hipStream_t st) {
  const char* e = getenv(env);
  if (!e || atoi(e) <= 0) return nullptr;
  unsigned long long* d = nullptr;
  if (hipMalloc((void**)&d, (size_t)grid * n * 8) != hipSuccess) return nullptr;
  (void)hipMemsetAsync(d, 0, (size_t)grid * n * 8, st);
  return d;
}
template <class... A>
static inline void rdst_stamps_end(unsigned long long* d, int64_t grid, int n, int mode, hipStream_t st, const char* tag, const A&... a) {
  if (!d) return;
  (void)hipStreamSynchronize(st);
  unsigned long long* h = (unsigned long long*)malloc((size_t)grid * n * 8);
  (void)hipMemcpy(h, d, (size_t)grid * n * 8, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  fprintf(stderr, "[stamps ");
  fprintf(stderr, tag, a...);
  fprintf(stderr, " grid=%lld] %s\n", (long long)grid,
          mode == RDST_STAMPS_TICKS ? "mean ticks since the stamp before / since stamp 0 (n workgroups)" : "mean cycles per workgroup");
  for (int k = 0; k < n; ++k) {
    double sum = 0, sum0 = 0;
    int cnt = 0;
    for (int64_t w = 0; w < grid; ++w) {
      const unsigned long long* s = h + (size_t)w * n;
      if (mode == RDST_STAMPS_TICKS && !s[k]) continue;
      sum += (double)(mode == RDST_STAMPS_TICKS ? s[k] - s[k ? k - 1 : 0] : s[k]);
      sum0 += (double)(s[k] - s[0]);
      cnt++;
    }
    if (!cnt) continue;
    if (mode == RDST_STAMPS_TICKS) fprintf(stderr, "  %2d: %9.0f %9.0f (n=%d)\n", k, sum / cnt, sum0 / cnt, cnt);
    else fprintf(stderr, "  %2d: %9.0f\n", k, sum / cnt);
  }
  free(h);
}
#else
#define RDST_DBGV(x) 0
static inline constexpr const char* rdst_dbg_getenv(const char*) { return nullptr; }
static inline unsigned long long* rdst_stamps_begin(const char*, int64_t, int, hipStream_t) { return nullptr; }
template <class... A>
static inline void rdst_stamps_end(unsigned long long*, int64_t, int, int, hipStream_t, const char*, const A&...) {}
#endif
// RDST_DISABLE_MFMA=1 (debug build): every matrix-core launcher passes and the generic kernels serve
static inline bool mfma_disabled() {
  const char* e = rdst_dbg_getenv("RDST_DISABLE_MFMA");
  return e && e[0] == '1';
}

// The kernel side of the stamps: where a kernel's time goes, phase by phase.  Both fold to nothing when they are off.
// RDST_PHASES_BEGIN(on) declares 8 cycle counters; RDST_PHASE(on, k) adds the cycles since the previous RDST_PHASE to counter k;
// RDST_PHASES_STORE(cond, buf, row) writes them to row `row` of the buffer of rdst_stamps_begin().  `on` is RDST_DBGV(p.stamps)
// (the constant 0 in the shipped library) or a constant set by a -D switch of the file.  (Macros, not a struct with methods:
// the register-saturated kernels allocate differently around a struct, and a diagnostic build has to measure the shipped code.)
#define RDST_PHASES_BEGIN(on)                                              \
  unsigned long long tprev_ = (on) ? __builtin_readcyclecounter() : 0ull; \
  unsigned long long tacc_[8] = {0, 0, 0, 0, 0, 0, 0, 0}
#define RDST_PHASE(on, k)                                          \
  if (on) {                                                        \
    const unsigned long long tn_ = __builtin_readcyclecounter();   \
    tacc_[k] += tn_ - tprev_;                                      \
    tprev_ = tn_;                                                  \
  }
#define RDST_PHASES_STORE(cond, buf, row) \
  if (cond)                               \
    for (int k_ = 0; k_ < 8; ++k_) (buf)[(size_t)(row) * 8 + k_] = tacc_[k_]
// WaveTicks<ON>: 8 counters per wave in clock64() ticks, without a buffer: lane 0 of every wave of workgroup 0 prints its 8 slots,
// `legend` naming them.  ON is a -D switch of the file (tools/abl_build.sh); the kernel calls print() once, at its end.
template <bool ON>
struct WaveTicks {
  long long tk[8], tl;
  __device__ __forceinline__ WaveTicks() {
    if constexpr (ON) {
      for (int k = 0; k < 8; ++k) tk[k] = 0;
      tl = clock64();
    }
  }
  __device__ __forceinline__ void add(int k) {
    if constexpr (ON) {
      const long long n = clock64();
      tk[k] += n - tl;
      tl = n;
    }
  }
  __device__ __forceinline__ void print(int wave, int lane, const char* role, const char* legend) const {
    if constexpr (ON) {
      if (blockIdx.x == 0 && lane == 0)
        printf("wave %d %s [%s]: %lld %lld %lld %lld %lld %lld %lld %lld\n", wave, role, legend, tk[0], tk[1], tk[2], tk[3], tk[4],
               tk[5], tk[6], tk[7]);
    }
  }
};

// thread-local last-error text behind rdst_last_error()
extern thread_local char g_rdst_err[256];
static inline int rdst_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_rdst_err, sizeof(g_rdst_err), fmt, ap);
  va_end(ap);
  return code;
}
static inline int rdst_launch_status(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rdst_fail(-(int)e, "%s: %s", what, hipGetErrorString(e));
  return 0;
}

// Launch `kern` with `smem` bytes of dynamic LDS and report the launch's status.  More than 64 KB of dynamic LDS has to be allowed per
// kernel first, and that is done on EVERY launch: the attribute is per DEVICE, a process-wide "done" flag would leave a second GPU
// without it.  At 64 KB or less the call is skipped — the limit it would set is the one every kernel starts with, so nothing the
// runtime can observe changes (some kernels ask for less in their small instantiations).
template <class K, class... A>
static inline int rdst_launch(K kern, dim3 grid, dim3 threads, size_t smem, hipStream_t st, const char* what, const A&... args) {
  if (smem > 64 * 1024) (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  hipLaunchKernelGGL(kern, grid, threads, smem, st, args...);
  return rdst_launch_status(what);
}

// Every pointer and every leading dimension (in BYTES) is a multiple of the granule `gran` (a kernel's chunk size).
static inline bool rdst_aligned(int gran, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> ld_bytes) {
  for (const void* q : ptrs)
    if ((uintptr_t)q % gran) return false;
  for (int64_t l : ld_bytes)
    if (l % gran) return false;
  return true;
}

// The persistent grid plan: `ntiles` tiles over at most `cap` workgroups, each taking *tiles_per_wg consecutive tiles, and
// no more workgroups than that leaves with work.  Returns the grid.
static inline int64_t rdst_tile_grid(int64_t ntiles, int64_t cap, int* tiles_per_wg) {
  const int64_t grid = ntiles < cap ? ntiles : cap;
  *tiles_per_wg = (int)((ntiles + grid - 1) / grid);
  return (ntiles + *tiles_per_wg - 1) / *tiles_per_wg;
}

// In front of every launch that writes one slab row per workgroup: `grid` rows of `stride` floats fit the workspace region.
// The caps come from the same region (WsSlab::cap), so this never fires unless a layout and a launcher stop agreeing.
static inline int rdst_slab_fits(const WsSlab& r, int64_t grid, int64_t stride, const char* what) {
  if (r.fits(grid, stride)) return 0;
  return rdst_fail(RDST_EINVAL, "%s: %lld slab rows of %lld floats do not fit the workspace region (%lld x %lld)", what,
                   (long long)grid, (long long)stride, (long long)r.rows, (long long)r.stride);
}

// The compute mode of an entry point's dtype, decoded first thing: `dtype` becomes the element type of the rows (RDST_BF16 or
// RDST_F32) and `split` says whether the GEMMs run in the split arithmetic of mfma.h (RDST_F32X3: fp32 rows, Mma<float, true>).
// The launchers take `split` as an argument and pick their <..., true> instantiation from it; kernels without a split form run
// exact fp32.  Unknown values are refused.
static inline int rdst_dtype(int& dtype, bool& split, const char* who) {
  if (dtype != RDST_BF16 && dtype != RDST_F32 && dtype != RDST_F32X3) return rdst_fail(RDST_EINVAL, "%s: bad dtype %d", who, dtype);
  split = dtype == RDST_F32X3;
  if (split) dtype = RDST_F32;
  return 0;
}
static inline int rdst_dtype(int& dtype, const char* who) {   // (an entry point without split kernels)
  bool split;
  return rdst_dtype(dtype, split, who);
}

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16>(bf16 v) { return __bfloat162float(v); }
template <typename T> __device__ __forceinline__ T from_f32(float v);
template <> __device__ __forceinline__ float from_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 from_f32<bf16>(float v) { return __float2bfloat16(v); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_erf_grad(float x) {
  // d/dx [0.5 x (1+erf(x/sqrt2))] = 0.5(1+erf(x/sqrt2)) + x * exp(-x^2/2)/sqrt(2pi)
  return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.39894228040143267794f * expf(-0.5f * x * x);
}
// GELU(erf) for the bf16 throughput mode: erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far below
// bf16 resolution) on the hardware exp2 / rcp — ~14 vector instructions instead of erff's ~40; the
// Linear kernels around a GELU were vector-issue bound on it (measured).  The fp32 parity mode keeps erff.
__device__ __forceinline__ void erf_as(float z, float& erfz, float& expmz2) {
  const float az = fabsf(z);
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, az, 1.0f));
  float pl = fmaf(1.061405429f, t, -1.453152027f);
  pl = fmaf(pl, t, 1.421413741f);
  pl = fmaf(pl, t, -0.284496736f);
  pl = fmaf(pl, t, 0.254829592f);
  pl *= t;
  expmz2 = __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);   // exp(-z^2)
  erfz = copysignf(fmaf(-pl, expmz2, 1.0f), z);
}
__device__ __forceinline__ float gelu_fast(float x) {
  float e, g;
  erf_as(x * 0.70710678118654752440f, e, g);
  return 0.5f * x * (1.0f + e);
}
__device__ __forceinline__ float gelu_grad_fast(float x) {
  float e, g;
  erf_as(x * 0.70710678118654752440f, e, g);                       // g = exp(-x^2/2)
  return fmaf(x * 0.39894228040143267794f, g, 0.5f * (1.0f + e));
}
// GELU through a table in LDS (bf16 throughput mode, the fused Mlp kernels): 512 entries of four fp16 over [-8, 8),
//   entry i = (Phi(u_i), Phi(u_i+1) - Phi(u_i), g(u_i), g(u_i+1) - g(u_i)),  u_i = -8 + i/32,  g = GELU' = Phi + u phi,
// read with ONE ds_read_b64 and interpolated linearly by v_fma_mix_f32 (fp32 weight x fp16 slope + fp16 value, fp32
// result): interpolation error <= 3e-5 in Phi, 1e-4 in GELU', fp16 storage 2.4e-4 / 4.9e-4 — the results are then
// rounded to bf16 (2e-3) anyway — for ~8 vector instructions per element where the erf / exp2 / rcp form takes ~27:
// those kernels' GELU phases run at the vector-issue floor.  Outside [-8, 8) the clamped index
// gives 0 / 1.
#define RDST_GELU_TAB_BYTES 4096
__device__ __forceinline__ void gelu_tab_fill(char* tab, int tid, int nt) {
  for (int i = tid; i < 512; i += nt) {
    const float u0 = -8.f + (float)i * 0.03125f, u1 = u0 + 0.03125f;
    const float c0 = 0.5f * erfcf(-u0 * 0.70710678118654752440f), c1 = 0.5f * erfcf(-u1 * 0.70710678118654752440f);
    const float g0 = fmaf(u0 * 0.39894228040143267794f, expf(-0.5f * u0 * u0), c0);
    const float g1 = fmaf(u1 * 0.39894228040143267794f, expf(-0.5f * u1 * u1), c1);
    const _Float16 h0 = (_Float16)c0, h2 = (_Float16)g0;
    const _Float16 h1 = (_Float16)(c1 - (float)h0), h3 = (_Float16)(g1 - (float)h2);   // slopes from the ROUNDED values
    uint2 w;
    w.x = (uint32_t)__builtin_bit_cast(uint16_t, h0) | ((uint32_t)__builtin_bit_cast(uint16_t, h1) << 16);
    w.y = (uint32_t)__builtin_bit_cast(uint16_t, h2) | ((uint32_t)__builtin_bit_cast(uint16_t, h3) << 16);
    reinterpret_cast<uint2*>(tab)[i] = w;
  }
}
// forward only: (Phi, slope) pairs alone, 4 bytes per entry (a b32 read of random entries spreads over all 64 banks)
#define RDST_GELU_TAB4_BYTES 2048
__device__ __forceinline__ void gelu_tab4_fill(char* tab, int tid, int nt) {
  for (int i = tid; i < 512; i += nt) {
    const float u0 = -8.f + (float)i * 0.03125f, u1 = u0 + 0.03125f;
    const float c0 = 0.5f * erfcf(-u0 * 0.70710678118654752440f), c1 = 0.5f * erfcf(-u1 * 0.70710678118654752440f);
    const _Float16 h0 = (_Float16)c0, h1 = (_Float16)(c1 - (float)h0);
    reinterpret_cast<uint32_t*>(tab)[i] = (uint32_t)__builtin_bit_cast(uint16_t, h0) | ((uint32_t)__builtin_bit_cast(uint16_t, h1) << 16);
  }
}
// (interpolation weight, byte offset of the entry)
__device__ __forceinline__ float gelu_tab_index(float u, uint32_t& off) {
  const float t = __builtin_amdgcn_fmed3f(fmaf(u, 32.f, 256.f), 0.f, 511.99f);
  off = (uint32_t)t << 3;
  return __builtin_amdgcn_fractf(t);
}
__device__ __forceinline__ float gelu_tab4_index(float u, uint32_t& off) {
  const float t = __builtin_amdgcn_fmed3f(fmaf(u, 32.f, 256.f), 0.f, 511.99f);
  off = (uint32_t)t << 2;
  return __builtin_amdgcn_fractf(t);
}
// value + weight * slope of one packed (value = low half, slope = high half) fp16 pair
__device__ __forceinline__ float gelu_tab_lerp(float w, uint32_t pair) {
  float r;
  asm("v_fma_mix_f32 %0, %1, %2, %2 op_sel:[0,1,0] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(w), "v"(pair));
  return r;
}
template <bool FAST = false>
__device__ __forceinline__ float apply_act(float x, int act) {
  if (act == RDST_ACT_GELU) return FAST ? gelu_fast(x) : gelu_erf(x);
  if (act == RDST_ACT_LEAKY02) return x > 0.f ? x : 0.2f * x;
  if (act == RDST_ACT_LEAKY001) return x > 0.f ? x : 0.01f * x;
  return x;
}
template <bool FAST = false>
__device__ __forceinline__ float act_grad(float xpre, int act) {
  if (act == RDST_ACT_GELU) return FAST ? gelu_grad_fast(xpre) : gelu_erf_grad(xpre);
  if (act == RDST_ACT_LEAKY02) return xpre > 0.f ? 1.f : 0.2f;
  if (act == RDST_ACT_LEAKY001) return xpre > 0.f ? 1.f : 0.01f;
  return 1.f;
}
