// The K-tap chain of the degradation kernels (resample.hip, consistency.hip): one output value from the taps of one table
// row.  acc = w[0] * v[0] rounded, then one explicit fmaf per tap in ascending order, so every kernel that forms a value
// through tapk() from the same samples under the same table gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// one output value from the 4 * K4 taps of one table row: v(j) is the sample at (unclamped) source index j
template <class F>
__device__ __forceinline__ float tapk(const int4* __restrict__ it, const f4* __restrict__ wt, int K4, F v) {
  int4 j = it[0];
  f4 w = wt[0];
  float acc = __fmul_rn(w.x, v(j.x));
  acc = fmaf(w.y, v(j.y), acc);
  acc = fmaf(w.z, v(j.z), acc);
  acc = fmaf(w.w, v(j.w), acc);
  int q = 1;
  // long rows, four table entries at a time: their eight loads and sixteen samples are in flight together (a wave forms one
  // chain per lane and nothing else hides the tables' latency); the order of the sums is the same
  // (and the next four entries are loaded before the current sixteen taps are summed)
  int4 jn[4];
  f4 wn[4];
  if (q + 4 <= K4) {
#pragma unroll
    for (int s = 0; s < 4; ++s) jn[s] = it[q + s], wn[s] = wt[q + s];
  }
  for (; q + 4 <= K4; q += 4) {
    int4 jj[4];
    f4 ww[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) jj[s] = jn[s], ww[s] = wn[s];
    if (q + 8 <= K4) {
#pragma unroll
      for (int s = 0; s < 4; ++s) jn[s] = it[q + 4 + s], wn[s] = wt[q + 4 + s];
    }
    float vv[16];
#pragma unroll
    for (int s = 0; s < 4; ++s) vv[4 * s] = v(jj[s].x), vv[4 * s + 1] = v(jj[s].y), vv[4 * s + 2] = v(jj[s].z), vv[4 * s + 3] = v(jj[s].w);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc = fmaf(ww[s].x, vv[4 * s], acc);
      acc = fmaf(ww[s].y, vv[4 * s + 1], acc);
      acc = fmaf(ww[s].z, vv[4 * s + 2], acc);
      acc = fmaf(ww[s].w, vv[4 * s + 3], acc);
    }
  }
  for (; q < K4; ++q) {
    j = it[q];
    w = wt[q];
    acc = fmaf(w.x, v(j.x), acc);
    acc = fmaf(w.y, v(j.y), acc);
    acc = fmaf(w.z, v(j.z), acc);
    acc = fmaf(w.w, v(j.w), acc);
  }
  return acc;
}

}  // namespace
