// The counter-based draw idiom of the device samplers (espi_params.hip states the same three functions for the fake-ESPI
// stream; augment_params.hip takes them from here): a 32-bit mixer, a draw = mix of (key, draw index), and an integer in a
// closed range by multiply-shift.  The recipes built from them are in include/spnet_hip.h beside the prototypes.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned rng_mix(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}
// draw k of a key
__device__ __forceinline__ unsigned rng_draw(unsigned key, unsigned k) {
  return rng_mix(key ^ (k * 0x85ebca6bu + 0xc2b2ae35u));
}
// integer in [lo, hi] by multiply-shift; an empty range gives lo
__device__ __forceinline__ int rng_randint(unsigned u, int lo, int hi) {
  const int n = max(hi - lo + 1, 1);
  return lo + (int)(((unsigned long long)u * (unsigned long long)(unsigned)n) >> 32);
}
