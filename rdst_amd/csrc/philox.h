// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 library's
// philox4x32): a counter-based generator without state.  The four output words are a pure function of the 128-bit counter
// and the 64-bit key, so a value that is keyed by its own position comes out the same whatever thread, workgroup or kernel
// forms it.  Plain integer arithmetic: two 32 x 32 -> 64 multiplies per round (the low halves and __umulhi), ten rounds, the
// key bumped by the Weyl constants between them.  tests/noise_reference.py restates it in exact integers and holds the
// Random123 known-answer vectors.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;   // the round multipliers
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;   // the key increments

struct PhiloxWords {
  uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ PhiloxWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                     uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return {c0, c1, c2, c3};
}

// the words of pixel (y, x) of plane `plane` under `seed`: key = the seed's halves, counter = (x, y, plane, stream tag 0)
__device__ __forceinline__ PhiloxWords philox_pixel(unsigned long long seed, uint32_t plane, uint32_t y, uint32_t x) {
  return philox4x32_10(x, y, plane, 0u, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32));
}

}  // namespace
