// What the two PNG packers (png.hip: literals only; png_lz.hip: literals and matches) state alike, once: the limits, how
// bits reach the zeroed output, a code table's entry, how a frame's zlib stream begins, and how the filtered stream (filter
// type 0 on every row: H rows of 1 + rb bytes) is walked.  png_decode.hip takes the Adler modulus, the stream limit and the
// wave sum.  Everything is inlined into the one kernel that calls it; nothing here owns LDS.
// NOT here, on purpose: the workgroup scan of the bit offsets, the 64-bit register accumulator and the end-of-block / Adler
// tail.  Each of them, moved into a function or struct of this header, changed the packers' instruction streams (and, in
// one form of the scan, took png_pack_kernel from 74 to 83 VGPRs and png_lz_kernel<true> to scratch); measured, the LZ
// packer was 1-3 % slower.  They stay written out in png.hip and png_lz.hip, whose kernels compile as they always did.
#pragma once
#include "common.h"

constexpr unsigned ADLER_MOD = 65521u;
constexpr long PNG_MAX_STREAM = (1L << 27);  // bytes of a filtered stream: 15 bits per symbol stay inside 31-bit counts

inline bool png_shape_ok(int N, int H, int W, int channels) {
  if (N < 0 || H < 1 || W < 1 || channels < 1 || channels > 4) return false;
  return (long)H * ((long)W * channels + 1) <= PNG_MAX_STREAM;
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
  return v;
}

// nb (1..32) bits of v at bit position pos of the output, which fills every byte from its least significant bit (the
// buffer is little-endian words, so bit pos of the stream is bit pos % 32 of word pos / 32).  Dropped past `limit`.
__device__ __forceinline__ void or_bits(uint32_t* out, unsigned long long pos, unsigned long long limit, uint32_t v, int nb) {
  if (pos + (unsigned)nb > limit) return;
  const unsigned sh = (unsigned)(pos & 31);
  atomicOr(out + (pos >> 5), v << sh);
  if (sh + (unsigned)nb > 32u) atomicOr(out + (pos >> 5) + 1, v >> (32u - sh));
}

// a canonical code of the host (code | length << 16) as the packers keep it in LDS: length << 16 | code, bit-reversed
// (first code bit in bit 0)
__device__ __forceinline__ uint32_t code_table_entry(uint32_t c) {
  const unsigned len = (c >> 16) & 15u;
  const unsigned code = c & ((1u << len) - 1u);
  return (len << 16) | (len ? (__brev(code) >> (32u - len)) : 0u);
}
// zlib header (deflate, 32 KiB window, no preset dictionary, level 0: 0x78 0x01) at byte o0, then the hb bits of the block
// header (`header`: the frame's HDR_WORDS words).  Returns the bit position of the first symbol.
template <int HDR_WORDS>
__device__ __forceinline__ unsigned long long write_stream_head(uint32_t* out, long long o0, unsigned long long limit,
                                                                const uint32_t* header, int hb, int tid) {
  const unsigned long long base = ((unsigned long long)o0 + 2ull) * 8ull;
  if (tid == HDR_WORDS) or_bits(out, (unsigned long long)o0 * 8ull, limit, 0x78u, 8);
  if (tid == HDR_WORDS + 1) or_bits(out, (unsigned long long)o0 * 8ull + 8ull, limit, 0x01u, 8);
  if (tid < HDR_WORDS) {
    const int nb = min(hb - 32 * tid, 32);
    if (nb > 0) {
      uint32_t w = header[tid];
      if (nb < 32) w &= (1u << nb) - 1u;
      or_bits(out, base + 32ull * tid, limit, w, nb);
    }
  }
  return base + (unsigned)hb;
}

// Index tid + T m (m = 0, 1, ...) of a sequence of rows of `period` bytes as (row, column), carried from step to step
// instead of divided out again.
template <int T>
struct RowCursor {
  long row;
  int col;
  int period, qstep, rstep;
  __device__ __forceinline__ RowCursor(int tid, int period_) {
    row = tid / period_;
    col = tid % period_;
    period = period_;
    qstep = T / period_;
    rstep = T % period_;
  }
  __device__ __forceinline__ void step() {
    row += qstep;
    col += rstep;
    const bool wrap = col >= period;
    col -= wrap ? period : 0;
    row += wrap ? 1 : 0;
  }
};
// the filtered stream's byte under a cursor over rows of rb + 1: the filter type 0 first, then the row's rb pixel bytes
template <int T>
__device__ __forceinline__ unsigned char stream_byte(const unsigned char* __restrict__ src, int rb, const RowCursor<T>& c,
                                                     bool inside) {
  return (inside && c.col > 0) ? src[c.row * rb + (c.col - 1)] : (unsigned char)0;
}
