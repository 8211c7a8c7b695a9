// PNG encoding of N uint8 frames that sit in device memory: the zlib stream of each frame, written by the GPU as ONE final
// dynamic-Huffman deflate block that holds nothing but literals (no LZ77 matches; ESPI frames are sensor noise, what zlib
// gains on them it gains in its Huffman stage).  Replaces the encoder behind cv2.imwrite (gen_fake_espi.py:274-275,
// augment_preproc.py:99, spnet/utils.py:132); the container (signature, IHDR, IDAT, IEND and their CRCs) stays on the host.
//
// The filtered stream of a frame is PNG's scanline stream with filter type 0 on every row: H rows of 1 + rb bytes,
// rb = W * channels, L = H * (rb + 1) bytes in all.
//
//   spnet_png_hist   one workgroup per frame: the 256-bin histogram of the stream (per-wave LDS bins, summed at the end; the
//                    H filter bytes are added to bin 0) and its Adler-32.  A pixel d at stream index i adds d to the low sum
//                    and d * (L - i) to the high sum, so the sums are formed per thread in 64 bits, reduced modulo 65521
//                    ONCE per thread and added up across the workgroup as values below 2^16: no 32-bit sum can overflow.
//   spnet_png_pack   one workgroup per frame walks the stream in tiles of 1024 threads x 16 symbols.  A tile is staged in LDS
//                    with coalesced byte loads; a thread then owns 16 consecutive symbols, counts their code bits, takes its
//                    bit offset from a workgroup scan (the offset carried from tile to tile is uniform in the workgroup) and
//                    appends its codes to a 64-bit register, least significant bit first, 32 bits at a time.  The first and
//                    the last word a thread touches may be shared with its neighbours (or with the next frame): those are
//                    merged with atomicOr into the zeroed output; the words in between are the thread's alone and are
//                    stored.  OR is commutative, so the bytes do not depend on the order in which threads arrive.  Nothing
//                    waits on another workgroup.  Every write is checked against the end of the frame's slot.
#include "common.h"
#include "deflate_bits.h"

namespace {

constexpr int PNG_T = 1024;                 // threads per workgroup (16 waves)
constexpr int PNG_WAVES = PNG_T / SPNET_WAVE;
constexpr int PNG_SPT = 16;                 // symbols per thread per tile: one 16-byte LDS read
constexpr int PNG_TILE = PNG_T * PNG_SPT;
constexpr int PNG_NSYM = 257;               // 256 literals + end of block
constexpr int PNG_HDR_WORDS = 64;           // 2048 bits: 3 + 14 + 19 * 3 + 258 * 7 = 1880 is the longest header

__global__ __launch_bounds__(PNG_T) void png_hist_kernel(const unsigned char* __restrict__ src, int H, int rb,
                                                         uint32_t* __restrict__ hist, uint32_t* __restrict__ adler) {
  __shared__ unsigned s_h[PNG_WAVES][256];
  __shared__ unsigned s_a[PNG_WAVES], s_b[PNG_WAVES];
  const int tid = threadIdx.x, wave = tid >> 6;
  const long n = blockIdx.x;
  for (int i = tid; i < PNG_WAVES * 256; i += PNG_T) (&s_h[0][0])[i] = 0u;
  __syncthreads();

  const long nsrc = (long)H * rb, L = nsrc + H;
  const unsigned char* p = src + n * nsrc;
  unsigned* h = s_h[wave];
  // pixel byte j sits in row j / rb, at stream index j + row + 1; the row is carried, not divided out again (written out:
  // RowCursor gives this kernel other code)
  long row = tid / rb;
  int col = tid % rb;
  const int qstep = PNG_T / rb, rstep = PNG_T % rb;
  unsigned long long sa = 0, sb = 0;
  for (long j = tid; j < nsrc; j += PNG_T) {
    const unsigned d = p[j];
    atomicAdd(&h[d], 1u);
    sa += d;
    sb += (unsigned long long)d * (unsigned long long)(L - (j + row + 1));
    row += qstep;
    col += rstep;
    if (col >= rb) { col -= rb; ++row; }
  }
  const unsigned a = wave_sum_u32((unsigned)(sa % ADLER_MOD));     // 64 values below 2^16
  const unsigned b = wave_sum_u32((unsigned)(sb % ADLER_MOD));
  if ((tid & 63) == 0) { s_a[wave] = a; s_b[wave] = b; }
  __syncthreads();
  if (tid < 256) {
    unsigned c = (tid == 0) ? (unsigned)H : 0u;                     // the filter-type bytes
    for (int w = 0; w < PNG_WAVES; ++w) c += s_h[w][tid];
    hist[n * 256 + tid] = c;
  }
  if (tid == 0) {
    unsigned A = 1u, B = (unsigned)(L % ADLER_MOD);                 // the initial 1 is added to the high sum L times
    for (int w = 0; w < PNG_WAVES; ++w) { A += s_a[w]; B += s_b[w]; }     // 1024 values below 2^16 each: below 2^27
    adler[n] = ((B % ADLER_MOD) << 16) | (A % ADLER_MOD);
  }
}

struct PackArgs {
  const unsigned char* src;
  const uint32_t* codes;
  const uint32_t* header;
  const int* header_bits;
  const long long* offsets;
  const uint32_t* adler;
  uint32_t* out;
  long out_bytes;
  int H, rb;
};

__global__ __launch_bounds__(PNG_T) void png_pack_kernel(const PackArgs a) {
  __shared__ uint32_t s_code[PNG_NSYM];                   // length << 16 | code, bit-reversed: first code bit in bit 0
  __shared__ __align__(16) unsigned char s_sym[PNG_TILE];
  __shared__ unsigned s_wtot[PNG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long n = blockIdx.x;
  const long long o0 = a.offsets[n], o1 = a.offsets[n + 1];
  if (o0 < 0 || o1 < o0 || o1 > (long long)a.out_bytes) return;          // (uniform) a slot outside the buffer: not written
  const unsigned long long limit = (unsigned long long)o1 * 8ull;
  uint32_t* out = a.out;

  for (int s = tid; s < PNG_NSYM; s += PNG_T) {
    const uint32_t c = a.codes[n * PNG_NSYM + s];
    s_code[s] = code_table_entry(c);
  }

  const int hb = min(max(a.header_bits[n], 0), PNG_HDR_WORDS * 32);
  // bit position of the tile's first symbol
  unsigned long long carry = write_stream_head<PNG_HDR_WORDS>(out, o0, limit, a.header + n * PNG_HDR_WORDS, hb, tid);

  const int rb = a.rb, rb1 = rb + 1;
  const long nsrc = (long)a.H * rb, L = nsrc + a.H;
  const unsigned char* p = a.src + n * nsrc;
  // stream index tid + 1024 m of the m-th staging step: row / column carried across steps and tiles
  RowCursor<PNG_T> c(tid, rb1);
  __syncthreads();

  for (long tile = 0; tile < L; tile += PNG_TILE) {
#pragma unroll
    for (int k = 0; k < PNG_SPT; ++k) {
      const long i = tile + (long)k * PNG_T + tid;
      s_sym[k * PNG_T + tid] = stream_byte(p, rb, c, i < L);
      c.step();
    }
    __syncthreads();

    const long first = tile + (long)tid * PNG_SPT;
    const int cnt = (int)min(max(L - first, 0L), (long)PNG_SPT);
    const uint4 q = *reinterpret_cast<const uint4*>(s_sym + tid * PNG_SPT);
    const unsigned wq[4] = {q.x, q.y, q.z, q.w};
    uint32_t cv[PNG_SPT];
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < PNG_SPT; ++k) {
      cv[k] = (k < cnt) ? s_code[(wq[k >> 2] >> ((k & 3) * 8)) & 255u] : 0u;
      bits += cv[k] >> 16;
    }
    unsigned incl = bits;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = (unsigned)__shfl_up((int)incl, off, 64);
      if (lane >= off) incl += t;
    }
    if (lane == 63) s_wtot[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (int w = 0; w < PNG_WAVES; ++w) {
      const unsigned t = s_wtot[w];
      before += (w < wave) ? t : 0u;
      total += t;
    }
    const unsigned long long pos = carry + before + (incl - bits);
    if (bits > 0 && pos + bits <= limit) {
      uint32_t* wp = out + (pos >> 5);
      unsigned long long acc = 0;
      unsigned nacc = (unsigned)(pos & 31);                                // the bits below belong to the neighbour
      bool shared = true;                                                  // the first word may hold a neighbour's bits
#pragma unroll
      for (int k = 0; k < PNG_SPT; ++k) {
        acc |= (unsigned long long)(cv[k] & 0xffffu) << nacc;
        nacc += cv[k] >> 16;
        if (nacc >= 32u) {
          if (shared) atomicOr(wp, (uint32_t)acc);
          else *wp = (uint32_t)acc;
          shared = false;
          ++wp;
          acc >>= 32;
          nacc -= 32u;
        }
      }
      if (nacc > 0u) atomicOr(wp, (uint32_t)acc);
    }
    carry += total;
    __syncthreads();                                                       // s_sym and s_wtot are rewritten by the next tile
  }

  // end of block, zero bits up to the next byte (the buffer arrives zeroed), Adler-32 most significant byte first
  const uint32_t eob = s_code[256];
  if (tid == 0 && (eob >> 16)) or_bits(out, carry, limit, eob & 0xffffu, (int)(eob >> 16));
  const unsigned long long tail = ((carry + (eob >> 16) + 7ull) >> 3) * 8ull;
  if (tid >= 64 && tid < 68) {
    const int k = tid - 64;
    or_bits(out, tail + 8ull * k, limit, (a.adler[n] >> (24 - 8 * k)) & 255u, 8);
  }
}

}  // namespace

extern "C" int spnet_png_hist(const unsigned char* src, int N, int H, int W, int channels, uint32_t* hist, uint32_t* adler,
                              void* stream) {
  if (!png_shape_ok(N, H, W, channels) || !src || !hist || !adler) return (int)hipErrorInvalidValue;
  if (((uintptr_t)hist | (uintptr_t)adler) & 3) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipLaunchKernelGGL(png_hist_kernel, dim3((unsigned)N), dim3(PNG_T), 0, (hipStream_t)stream, src, H, W * channels, hist,
                     adler);
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_png_pack(const unsigned char* src, int N, int H, int W, int channels, const uint32_t* codes,
                              const uint32_t* header, const int* header_bits, const long long* offsets,
                              const uint32_t* adler, unsigned char* out, long out_bytes, void* stream) {
  if (!png_shape_ok(N, H, W, channels) || !src || !codes || !header || !header_bits || !offsets || !adler || !out)
    return (int)hipErrorInvalidValue;
  if (out_bytes < 0 || (out_bytes & 3)) return (int)hipErrorInvalidValue;            // whole 32-bit words
  if (((uintptr_t)codes | (uintptr_t)header | (uintptr_t)header_bits | (uintptr_t)adler | (uintptr_t)out) & 3)
    return (int)hipErrorInvalidValue;
  if ((uintptr_t)offsets & 7) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  PackArgs a;
  a.src = src; a.codes = codes; a.header = header; a.header_bits = header_bits; a.offsets = offsets; a.adler = adler;
  a.out = reinterpret_cast<uint32_t*>(out); a.out_bytes = out_bytes; a.H = H; a.rb = W * channels;
  hipLaunchKernelGGL(png_pack_kernel, dim3((unsigned)N), dim3(PNG_T), 0, (hipStream_t)stream, a);
  SPNET_RETURN_LAUNCH_STATUS();
}
