// The counter-based draw idiom of every device sampler, stated once: a 32-bit mixer, a draw = mix of (key, draw index), an
// integer in a closed range by multiply-shift, and the 24-bit uniform in [0, 1).  The KEY recipes differ by design and stay
// in the kernels (espi_params.hip's espi_key and frame chain, augment_params.hip's sample chain, the per-pixel
// pix * 0x9e3779b9 + seed chain of espi.hip and augment.hip); they are written down in include/spnet_hip.h beside the
// prototypes.  Integer-only apart from the exact * 2^-24, so it is included above a file's fp-contract pragma.
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
// the top 24 bits as a uniform in [0, 1): exact in float, and the same value in double
__device__ __forceinline__ float rng_u01(unsigned h) { return (float)(h >> 8) * (1.f / 16777216.f); }
__device__ __forceinline__ double rng_u01_double(unsigned h) { return (double)(h >> 8) * (1.0 / 16777216.0); }
