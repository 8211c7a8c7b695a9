// Shared device/host helpers for the SPNet gfx950 kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// The C ABI: every extern "C" definition is compiled against its prototype, so a definition that drifts from the header
// (a type, the order or the number of arguments) is a `conflicting types` error, not a wrong pointer at run time.
#include "spnet_hip.h"

#define SPNET_WAVE 64

static inline int spnet_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// A batch on grid y or z: those dimensions end at 65,535, so a batch of n goes out as launch(base, count) per chunk.
constexpr int SPNET_GRID_YZ_MAX = 65535;
template <class Launch>
static inline void spnet_for_grid_chunks(int n, Launch&& launch) {
  for (int base = 0; base < n; base += SPNET_GRID_YZ_MAX) launch(base, n - base < SPNET_GRID_YZ_MAX ? n - base : SPNET_GRID_YZ_MAX);
}

// Every extern "C" entry point returns 0 on success or the hipError_t of the failed launch.
#define SPNET_RETURN_LAUNCH_STATUS()            \
  do {                                          \
    hipError_t e__ = hipGetLastError();         \
    return (int)e__;                            \
  } while (0)

// Output extent of a VALID window of k taps at stride s over `in` elements: floor((in - k) / s) + 1, 0 when the window
// is longer than the input.  (C++ division truncates toward zero: in = k - 1 at stride 2 would give (-1)/2 + 1 = 1.)
static inline int spnet_valid_out(int in, int k, int s) { return in < k ? 0 : (in - k) / s + 1; }

// Memory-bound elementwise kernels: cap the grid and grid-stride the rest (256 CUs x 8 blocks).
static inline int spnet_ew_grid(long n_items, int block) {
  long g = (n_items + block - 1) / block;
  if (g > 2048 * 4) g = 2048 * 4;
  if (g < 1) g = 1;
  return (int)g;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
  return v;
}

// Input codec: uint8 grey level -> the network's float32 input, x = (v / 255 - 0.5) * 2 with every step rounded as numpy
// rounds it on float32 (spnet/utils.py:340-342), so a pixel converted on the device has the host conversion's bits.
__device__ __forceinline__ float spnet_u8_to_input_f(unsigned v) {
  return __fmul_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), 0.5f), 2.f);
}

// Keras' moving-statistics update, moving*momentum + value*(1 - momentum), with every product and the sum rounded on
// its own (no fused multiply-add): the same bits from every kernel that performs it.  (__fmul_rn / __fadd_rn are plain
// operators in this toolchain's headers; the pragma is what keeps the compiler from contracting them.)
__device__ __forceinline__ float bn_moving_update(float moving, float momentum, float value) {
#pragma clang fp contract(off)
  return __fadd_rn(__fmul_rn(momentum, moving), __fmul_rn(1.f - momentum, value));
}

// shift = beta - mean*scale of the BatchNorm affine as ONE fused multiply-add, written out: __fmul_rn / __fsub_rn are
// plain operators in this toolchain's headers and the compiler contracted the pair wherever it liked (it did, in every
// kernel -- tests/test_batchnorm_gpu.py found the bits); an explicit fmaf is the same in every kernel by construction.
__device__ __forceinline__ float bn_shift(float beta, float mean, float scale) {
  return fmaf(-mean, scale, beta);
}

// Batch statistics of one channel from its column sums (sum, sum of squares over M values) and everything the BatchNorm
// forward derives from them.  Three kernels perform this step (bn_fwd_finalize_kernel, and the consumers it is folded
// into: bn_fwd_fused_vec_kernel, dw3x3_tile_fwd_kernel) and must produce the same bits: the variance is ONE double
// fma, q/M - mean*mean rounded once (as above: written out, not left to contraction); tests/helpers/bn_ref.py's
// finalize_bits restates the whole step rounding by rounding.
struct BnChannelStats {
  float mean, invstd, scale, shift, unbiased_var;
};
__device__ __forceinline__ BnChannelStats bn_channel_stats(double s, double q, long M, float gamma, float beta, float eps) {
  BnChannelStats r;
  const double mean = s / (double)M;
  double var = fma(-mean, mean, q / (double)M);
  if (var < 0.0) var = 0.0;
  r.mean = (float)mean;
  r.invstd = (float)(1.0 / sqrt(__dadd_rn(var, (double)eps)));
  r.scale = __fmul_rn(gamma, r.invstd);
  r.shift = bn_shift(beta, r.mean, r.scale);
  r.unbiased_var = (float)((M > 1) ? __dmul_rn(var, (double)M / (double)(M - 1)) : var);
  return r;
}

// XCD-aware block remap (bijective for any grid size): blocks that the dispatcher deals to the same
// XCD (b % 8) get a contiguous range of logical ids, so neighbouring tiles share that XCD's L2.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int nx = 8;
  int q = nblk / nx, r = nblk % nx;
  int x = bid % nx, i = bid / nx;
  int base = (x < r) ? x * (q + 1) : r * (q + 1) + (x - r) * q;
  return base + i;
}
