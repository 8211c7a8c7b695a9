// The store of a uint8 tile that sits in LDS, shared by resize.hip and warp.hip: lanes own ALIGNED groups of 4 output elements
// in memory, one dword of a uint8 output or one float4 of a network-input output per lane, whatever the alignment of the
// output's rows.  For workgroups of 256 threads.
#pragma once
#include "common.h"

// RAW4 (diagnostic builds only): the float4 store converts int -> float plainly instead of spnet_u8_to_input_f
template <bool RAW4 = false>
__device__ __forceinline__ void put4(unsigned char* p, unsigned v0, unsigned v1, unsigned v2, unsigned v3) {
  *reinterpret_cast<unsigned*>(p) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
}
template <bool RAW4 = false>
__device__ __forceinline__ void put4(float* p, unsigned v0, unsigned v1, unsigned v2, unsigned v3) {
  if (RAW4) { *reinterpret_cast<float4*>(p) = make_float4((float)v0, (float)v1, (float)v2, (float)v3); return; }
  *reinterpret_cast<float4*>(p) = make_float4(spnet_u8_to_input_f(v0), spnet_u8_to_input_f(v1), spnet_u8_to_input_f(v2),
                                              spnet_u8_to_input_f(v3));
}
__device__ __forceinline__ void put1(unsigned char* p, unsigned v) { *p = (unsigned char)v; }
__device__ __forceinline__ void put1(float* p, unsigned v) { *p = spnet_u8_to_input_f(v); }

// nro rows of tw bytes (LDS, pitch bytes apart) -> out[row0 + row * OW + 0 .. tw), nq = groups per row (tile dwords + 1):
// groups of 4 elements that start where (address / sizeof(T)) % 4 == 0 are one vector store, the clipped groups at a row's
// ends go element by element
template <class T, bool RAW4 = false>
__device__ __forceinline__ void store_tile(T* __restrict__ out, const unsigned char* __restrict__ so, int pitch, long row0,
                                           int OW, int nro, int tw, int nq, int tid) {
  const long sh = (long)(((uintptr_t)out / sizeof(T)) & 3);
  for (int i = tid; i < nro * nq; i += 256) {
    const int row = i / nq, q = i - row * nq;
    const long e0 = row0 + (long)row * OW;                                // the row's first element
    const long e = ((((e0 + sh) >> 2) + q) << 2) - sh;
    const int rel = (int)(e - e0);                                        // -3 .. tw + 3
    if (rel >= tw) continue;
    const unsigned char* p = so + (size_t)row * pitch;
    if (rel >= 0 && rel + 4 <= tw) {
      put4<RAW4>(out + e, p[rel], p[rel + 1], p[rel + 2], p[rel + 3]);
    } else {
      for (int k = 0; k < 4; ++k)
        if (rel + k >= 0 && rel + k < tw) put1(out + e + k, p[rel + k]);
    }
  }
}
