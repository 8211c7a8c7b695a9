// PNG decoding of N files whose bytes sit in device memory: the inverse of png.hip's spnet_png_pack, but general -- the
// files this project reads were written by cv2.imwrite, Pillow and png.hip, so every deflate block type, LZ77 matches up
// to 32 KiB back and all five filter types occur.  Replaces the decoder behind Image.open(...).convert("RGB")
// (spnet/utils.py:325-345); the container (signature, chunks, CRCs) stays on the host (spnet_amd/png.py).
//
//   spnet_png_inflate   one wave (one 64-thread workgroup) per file.  Inflate is serial in its symbols, so the decode state
//                       of inflate_core.h is wave-uniform: every lane runs the same state machine on the same bits and
//                       holds the same values (redundant LDS writes of tables and literals carry one value to one address).
//                       The lanes divide what is parallel inside a stream: staging 1 KiB of compressed bytes in LDS, match
//                       copies inside the 32 KiB history window (which lives in LDS: a match never re-reads global bytes),
//                       flushing finished output to HBM in pieces of >= 16 KiB with consecutive lanes on consecutive
//                       bytes, and the Adler-32 sums of each piece.  LDS per workgroup: 32768 (window) + 3584 (tables) +
//                       1028 (input stage) = 37380 bytes, four workgroups per CU.  Nothing waits on another workgroup.
//                       Bounds: compressed bytes are fetched through the stage only, which reads zero beyond the file's
//                       extent; window indices are masked; the core checks op < L before every put and copy, and
//                       dist <= op; the flush writes bytes below op <= L of the file's own slot.
//   spnet_png_unfilter  one wave per file, rows in order (a row needs the row above), two rows in LDS.  None / Up: parallel
//                       over bytes.  Sub: a prefix sum modulo 256 per channel (a segment per lane, a wave scan of the
//                       segment sums).  Average / Paeth: serial along the row, one lane per channel (the chains of the bpp
//                       channels are independent).
#include "common.h"
#include "deflate_bits.h"
#include "inflate_core.h"

namespace {

constexpr int PD_T = SPNET_WAVE;            // one wave per file
constexpr int PD_WINDOW = 32768;
constexpr int PD_WMASK = PD_WINDOW - 1;
constexpr int PD_STAGE = 1024;              // compressed bytes staged at a time (+ 4 so that in32 reads whole words)
constexpr int PD_FLUSH = 16384;             // flush once this much is unflushed: 16384 + 258 < 32768 - 258
constexpr int PD_MAX_ROW = 32768;           // W * channels of spnet_png_unfilter: two rows in LDS

struct LdsIO {
  const unsigned char* src;     // the file's zlib stream
  int in_len;
  unsigned char* dst;           // the file's output slot
  unsigned char* win;           // [PD_WINDOW]
  uint32_t* stage;              // [PD_STAGE / 4 + 1]
  int stage_base;               // first staged byte, -1: nothing staged
  int flushed;                  // output bytes already in HBM (and in the Adler sums)
  unsigned a, b;                // Adler-32 of the flushed bytes
  int lane;

  __device__ void restage(int pos) {
    __syncthreads();                                                       // every lane is done with the old stage
    unsigned char* sb = reinterpret_cast<unsigned char*>(stage);
    for (int i = lane; i < PD_STAGE + 4; i += PD_T) {
      const int p = pos + i;                                               // pos < in_len < 2^31 - PD_STAGE - 4 (launcher)
      sb[i] = (p < in_len) ? src[p] : (unsigned char)0;
    }
    stage_base = pos;
    __syncthreads();
  }
  __device__ uint32_t in32(int pos) {
    if (stage_base < 0 || pos < stage_base || pos + 4 > stage_base + PD_STAGE) restage(pos);
    const int i = pos - stage_base;                                        // 0 .. PD_STAGE - 4
    const uint32_t w0 = stage[i >> 2], w1 = stage[(i >> 2) + 1];           // word index <= PD_STAGE / 4
    return (uint32_t)((((uint64_t)w1 << 32) | w0) >> (8 * (i & 3)));
  }
  __device__ void put(int op, unsigned byte) { win[op & PD_WMASK] = (unsigned char)byte; }
  __device__ void copy(int op, int dist, int len) {
    // Every source byte lies below op, so no lane needs a byte this copy produces.  In the ring, though, a destination
    // can land on the SLOT of a source: for dist > 32768 - len, destination byte k has the slot of source byte
    // k - (32768 - dist), which another lane reads (dist == 32768: the same lane).  That source index is not above k, so it
    // is read in the same turn of this loop or an earlier one than the write to its slot -- and within a turn all 64
    // lanes read before any writes, because the workgroup is ONE wave executing in lockstep (asserted below).
    static_assert(PD_T == SPNET_WAVE, "LdsIO::copy relies on a workgroup of exactly one wave");
    for (int k = lane; k < len; k += PD_T) {
      const int s = op - dist + (dist >= len ? k : k % dist);
      win[(op + k) & PD_WMASK] = win[s & PD_WMASK];
    }
    __syncthreads();                                                       // other lanes read these bytes from here on
  }
  __device__ void flush(int op) {
    const int n = op - flushed;                                            // <= PD_FLUSH + 258 + 255
    unsigned long long sa = 0, sb = 0;
    for (int i = lane; i < n; i += PD_T) {
      const unsigned d = win[(flushed + i) & PD_WMASK];
      dst[flushed + i] = (unsigned char)d;
      sa += d;
      sb += (unsigned long long)d * (unsigned)(n - i);
    }
    const unsigned ta = wave_sum_u32((unsigned)(sa % ADLER_MOD));           // 64 values below 2^16
    const unsigned tb = wave_sum_u32((unsigned)(sb % ADLER_MOD));
    b = (unsigned)((b + (unsigned long long)n * a + tb) % ADLER_MOD);
    a = (a + ta) % ADLER_MOD;
    flushed = op;
    __syncthreads();
  }
  __device__ void produced(int op) {
    if (op - flushed >= PD_FLUSH) flush(op);
  }
  __device__ uint32_t finish(int op) {
    if (op > flushed) flush(op);
    return (b << 16) | a;
  }
};

__global__ __launch_bounds__(PD_T) void png_inflate_kernel(const unsigned char* __restrict__ blob, long blob_bytes,
                                                           const long long* __restrict__ offsets, int L, long out_stride,
                                                           unsigned char* __restrict__ out, int* __restrict__ status) {
  __shared__ __align__(16) unsigned char s_win[PD_WINDOW];
  __shared__ inflate::Tables s_tab;
  __shared__ uint32_t s_stage[PD_STAGE / 4 + 1];
  const long n = blockIdx.x;
  const long long o0 = offsets[n], o1 = offsets[n + 1];
  int st;
  if (o0 < 0 || o1 < o0 || o1 > (long long)blob_bytes || o1 - o0 > (long long)(1 << 30)) {     // (uniform)
    st = inflate::BAD_ARGS;
  } else {
    LdsIO io;
    io.src = blob + o0;
    io.in_len = (int)(o1 - o0);
    io.dst = out + n * out_stride;
    io.win = s_win;
    io.stage = s_stage;
    io.stage_base = -1;
    io.flushed = 0;
    io.a = 1u;
    io.b = 0u;
    io.lane = threadIdx.x;
    st = inflate::run(io, s_tab, io.in_len, L);
  }
  if (threadIdx.x == 0) status[n] = st;
}

__device__ __forceinline__ unsigned pd_paeth(int a, int b, int c) {
  const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
  return (unsigned)((pa <= pb && pa <= pc) ? a : (pb <= pc) ? b : c);
}

__global__ __launch_bounds__(PD_T) void png_unfilter_kernel(const unsigned char* __restrict__ in, long in_stride, int H, int W,
                                                            int bpp, int rbp, unsigned char* __restrict__ first,
                                                            unsigned char* __restrict__ all, int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char s_rows[];                   // [2][rbp]
  const int lane = threadIdx.x;
  const long n = blockIdx.x;
  if (status[n] != 0) return;                                              // (uniform) not inflated: nothing to unfilter
  const int rb = W * bpp;
  unsigned char* prev = s_rows;
  unsigned char* cur = s_rows + rbp;
  for (int i = lane; i < rb; i += PD_T) prev[i] = 0;
  __syncthreads();
  const unsigned char* src = in + n * in_stride;
  for (int y = 0; y < H; ++y, src += rb + 1) {
    const int ft = src[0];
    if (ft > 4) {                                                          // (uniform)
      if (lane == 0) status[n] = inflate::BAD_FILTER;
      return;
    }
    for (int i = lane; i < rb; i += PD_T) cur[i] = src[1 + i];
    __syncthreads();
    if (ft == 2) {
      for (int i = lane; i < rb; i += PD_T) cur[i] = (unsigned char)(cur[i] + prev[i]);
    } else if (ft == 1) {
      const int seg = (W + PD_T - 1) / PD_T;
      const int p0 = min(lane * seg, W), p1 = min(p0 + seg, W);
      for (int c = 0; c < bpp; ++c) {
        unsigned s = 0;
        for (int p = p0; p < p1; ++p) {
          s += cur[p * bpp + c];
          cur[p * bpp + c] = (unsigned char)s;
        }
        unsigned incl = s & 255u;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const unsigned t = (unsigned)__shfl_up((int)incl, off, 64);
          if (lane >= off) incl += t;
        }
        const unsigned excl = incl - (s & 255u);
        for (int p = p0; p < p1; ++p) cur[p * bpp + c] = (unsigned char)(cur[p * bpp + c] + excl);
      }
    } else if (ft >= 3 && lane < bpp) {
      unsigned a = 0, c = 0;                                               // left and upper-left: zero before the first pixel
      for (int i = lane; i < rb; i += bpp) {
        const unsigned b = prev[i];
        const unsigned pred = (ft == 3) ? ((a + b) >> 1) : pd_paeth((int)a, (int)b, (int)c);
        a = (cur[i] + pred) & 255u;
        cur[i] = (unsigned char)a;
        c = b;
      }
    }
    __syncthreads();
    const long row = n * H + y;
    if (all)
      for (int i = lane; i < rb; i += PD_T) all[row * rb + i] = cur[i];
    if (first)
      for (int x = lane; x < W; x += PD_T) first[row * W + x] = cur[x * bpp];
    unsigned char* t = prev;
    prev = cur;
    cur = t;
    __syncthreads();                                                       // cur (the old prev) is rewritten by the next row
  }
}

}  // namespace

extern "C" int spnet_png_inflate(const unsigned char* blob, long blob_bytes, const long long* offsets, int N, long L,
                                 long out_stride, unsigned char* out, int* status, void* stream) {
  if (N < 0 || L < 1 || L > PNG_MAX_STREAM || out_stride < L || blob_bytes < 0) return (int)hipErrorInvalidValue;
  if (!blob || !offsets || !out || !status) return (int)hipErrorInvalidValue;
  if (((uintptr_t)offsets & 7) || ((uintptr_t)status & 3)) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)N), dim3(PD_T), 0, (hipStream_t)stream, blob, blob_bytes, offsets,
                     (int)L, out_stride, out, status);
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_png_unfilter(const unsigned char* inflated, long in_stride, int N, int H, int W, int channels,
                                  unsigned char* first, unsigned char* all, int* status, void* stream) {
  if (N < 0 || H < 1 || W < 1 || channels < 1 || channels > 4) return (int)hipErrorInvalidValue;
  const long rb = (long)W * channels, L = (long)H * (rb + 1);
  if (rb > PD_MAX_ROW || L > PNG_MAX_STREAM || in_stride < L) return (int)hipErrorInvalidValue;
  if (!inflated || !status || (!first && !all) || ((uintptr_t)status & 3)) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  const int rbp = (int)((rb + 15) / 16 * 16);
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)N), dim3(PD_T), (size_t)(2 * rbp), (hipStream_t)stream, inflated,
                     in_stride, H, W, channels, rbp, first, all, status);
  SPNET_RETURN_LAUNCH_STATUS();
}
