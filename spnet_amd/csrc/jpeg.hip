// Baseline JPEG encoding of N uint8 frames that sit in device memory: the entropy-coded scan of each frame (restart
// intervals, byte stuffing, RST markers), written by the GPU; the header segments and EOI stay on the host
// (spnet_amd/jpeg.py).  The arithmetic is integer only and is specified beside the prototypes in include/spnet_hip.h;
// tests/helpers/jpeg_ref.py restates it in numpy and the bytes are equal.
//
// One kernel, two forms.  A workgroup is ONE wave and owns ONE restart interval of one frame (at most 64 MCUs); a lane owns
// one MCU, that is one 8 x 8 block of every component.
//   1  per component: colour transform, both DCT passes in registers (fully unrolled: p[8][8] stays in VGPRs), quantisation;
//      the coefficients go to LDS in zigzag order, [component][k][lane] (a lane reads only its own column: no bank conflict,
//      no barrier).  The DC difference is the DC minus the left neighbour lane's (lane 0: minus 0) and replaces the DC.
//   2  every lane walks its coefficients and COUNTS its bits; a wave scan gives its bit offset in the interval.
//   3  the words of the staging buffer the interval needs are zeroed; every lane walks its coefficients again and appends its
//      codes, most significant bit first, to a 64-bit register that is flushed 32 bits at a time with ds atomic OR (the first
//      and the last word of a lane are shared with its neighbours; OR is commutative, so the bytes do not depend on the order
//      lanes arrive in); lane 0 sets the 1-bits that pad the last byte.
//   4  the staged bytes are read 64 at a time; a ballot counts the 0xFF bytes below each lane, which gives every byte its
//      place after stuffing.  spnet_jpeg_scan only counts (bytes + 0xFF bytes = the interval's size); spnet_jpeg_pack stores
//      every byte, and a 0x00 behind every 0xFF, with plain byte stores -- intervals are byte aligned, so every output byte
//      has exactly one writer and nothing in HBM is merged -- and then the RST marker.  The interval's place in the frame is
//      the sum of the sizes before it (read from the scan's array) plus 2 per marker.
// The packer RECOMPUTES steps 1 and 2: there is no coefficient workspace in HBM (as png_lz.hip keeps none for its tokens).
//
// LDS: the staging buffer holds the worst case of an interval, 64 lanes x channels x (27 + 63 * 26) bits (a DC code of at
// most 16 + 11 bits and 63 AC codes of at most 16 + 10): 13,324 bytes grey, 39,964 bytes colour; plus the coefficients
// (8 KiB per component) and the quantisation entries.  Colour comes to 65,056 of the 65,536 bytes a workgroup may declare
// statically.  Writes into the staging buffer are bounds-checked all the same.
#include "common.h"

namespace {

constexpr int JPEG_MAX_DIM = 65535;          // SOF0 holds 16-bit sizes
constexpr int JPEG_RI = 64;                  // MCUs of a restart interval at most: one lane each
constexpr int JPEG_BLOCK_BITS = 27 + 63 * 26;

// K[u][x] = rint(2^12 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u > 0) = 1/2
__device__ const int JPEG_K[8][8] = {
    {1448, 1448, 1448, 1448, 1448, 1448, 1448, 1448},   {2009, 1703, 1138, 400, -400, -1138, -1703, -2009},
    {1892, 784, -784, -1892, -1892, -784, 784, 1892},   {1703, -400, -2009, -1138, 1138, 2009, 400, -1703},
    {1448, -1448, -1448, 1448, 1448, -1448, -1448, 1448}, {1138, -2009, 400, 1703, -1703, -400, 2009, -1138},
    {784, -1892, 1892, -784, -784, 1892, -1892, 784},   {400, -1138, 1703, -2009, 2009, -1703, 1138, -400}};

// position in the zigzag sequence of the coefficient at natural index v * 8 + u
__device__ const unsigned char JPEG_ZZ_OF[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42,
                                                 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                                 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60,
                                                 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// The four Annex K "typical" Huffman tables (ITU-T T.81 K.3 - K.6) as BITS (codes of length 1 .. 16) and HUFFVAL (symbols
// in code order), turned into length << 16 | code per symbol at compile time (T.81 Annex C).
struct HuffCodes {
  uint32_t e[256];
};
constexpr HuffCodes make_codes(const unsigned char* bits, const unsigned char* vals) {
  HuffCodes t{};
  unsigned code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int j = 0; j < bits[len - 1]; ++j) t.e[vals[k++]] = ((unsigned)len << 16) | code++;
    code <<= 1;
  }
  return t;
}
constexpr unsigned char DC_LUM_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned char DC_CHR_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr unsigned char DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr unsigned char AC_LUM_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr unsigned char AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr unsigned char AC_CHR_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr unsigned char AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr HuffCodes DC_LUM = make_codes(DC_LUM_BITS, DC_VALS), DC_CHR = make_codes(DC_CHR_BITS, DC_VALS);
constexpr HuffCodes AC_LUM = make_codes(AC_LUM_BITS, AC_LUM_VALS), AC_CHR = make_codes(AC_CHR_BITS, AC_CHR_VALS);
static_assert(DC_LUM.e[0] == 0x20000u && DC_LUM.e[11] == 0x901feu && DC_CHR.e[11] == 0xb07feu, "Annex K DC codes");
static_assert(AC_LUM.e[0x00] == 0x4000au && AC_LUM.e[0xf0] == 0xb07f9u && AC_LUM.e[0xfa] == 0x10fffeu, "Annex K AC codes");
static_assert(AC_CHR.e[0x00] == 0x20000u && AC_CHR.e[0xf0] == 0xa03fau && AC_CHR.e[0xfa] == 0x10fffeu, "Annex K AC codes");
// [0] luminance, [1] chrominance; the DC tables are read with a size category 0 .. 15 (11 is the largest that occurs)
__device__ const HuffCodes JPEG_DC[2] = {DC_LUM, DC_CHR};
__device__ const HuffCodes JPEG_AC[2] = {AC_LUM, AC_CHR};

inline long jpeg_restart_interval(int W) { return (W + 7) / 8 < JPEG_RI ? (W + 7) / 8 : JPEG_RI; }
inline long jpeg_intervals(int H, int W) {
  const long mcus = (long)((H + 7) / 8) * ((W + 7) / 8), ri = jpeg_restart_interval(W);
  return (mcus + ri - 1) / ri;
}
inline bool jpeg_shape_ok(int N, int H, int W, int channels) {
  if (N < 0 || H < 1 || W < 1 || H > JPEG_MAX_DIM || W > JPEG_MAX_DIM) return false;
  if (channels != 1 && channels != 3) return false;
  return (long)N * jpeg_intervals(H, W) <= 0x7fffffffL;             // one workgroup per interval
}

struct JpegArgs {
  const unsigned char* src;
  const uint16_t* qt;
  uint32_t* sizes_out;          // scan
  const uint32_t* sizes_in;     // pack
  const long long* offsets;
  unsigned char* out;
  long out_bytes;
  int H, W, mcu_w, mcus, ri, n_int;
};

// One component of one block: colour transform, rows, columns, quantisation; coefficient k of the zigzag sequence goes to
// coef[k][lane].  qm: the component's 64 entries Q << 24 | ceil(2^24 / 2Q), natural order.
template <int C>
__device__ __forceinline__ void jpeg_block(const unsigned char* __restrict__ frame, int H, int W, int y0, int x0, int comp,
                                           const uint32_t* qm, short (*coef)[64], int lane) {
  // component = (cr R + cg G + cb B + add) >> 16: JFIF's RGB -> YCbCr in 16-bit fixed point, Y rounded half up, Cb / Cr
  // with 128.5 - 2^-16 added (the constants sum to 2^16 for Y and to 0 for Cb / Cr)
  const int cr = comp == 0 ? 19595 : comp == 1 ? -11059 : 32768;
  const int cg = comp == 0 ? 38470 : comp == 1 ? -21709 : -27439;
  const int cb = comp == 0 ? 7471 : comp == 1 ? 32768 : -5329;
  const int add = comp == 0 ? 32768 : (128 << 16) + 32767;
  int xo[8];
#pragma unroll
  for (int x = 0; x < 8; ++x) xo[x] = min(x0 + x, W - 1) * C;      // the last column is replicated
  int p[8][8];
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const unsigned char* row = frame + (long)min(y0 + y, H - 1) * W * C;      // the last row is replicated
    int s[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) {
      int v;
      if (C == 1) {
        v = row[xo[x]];
      } else {
        v = (cr * (int)row[xo[x]] + cg * (int)row[xo[x] + 1] + cb * (int)row[xo[x] + 2] + add) >> 16;
        v = min(max(v, 0), 255);
      }
      s[x] = v - 128;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int acc = 0;                                                  // |acc| <= 11584 * 128 < 2^21
#pragma unroll
      for (int x = 0; x < 8; ++x) acc += JPEG_K[u][x] * s[x];
      p[y][u] = (acc + 256) >> 9;                                   // 3 fractional bits, |p| <= 2896
    }
  }
#pragma unroll
  for (int v = 0; v < 8; ++v) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int q = 0;                                                    // 15 fractional bits, |q| <= 11584 * 2896 < 2^25
#pragma unroll
      for (int y = 0; y < 8; ++y) q += JPEG_K[v][y] * p[y][u];
      const uint32_t e = qm[v * 8 + u];
      // (|q| + (Q << 14)) / (Q << 15) = ((|q| >> 14) + Q) / 2Q, the division as a multiplication: exact for every
      // numerator below 2^14 and Q = 1 .. 255 (tests/test_jpeg_cpu.py runs through all of them)
      const unsigned n = ((unsigned)abs(q) >> 14) + (e >> 24);
      const int c = (int)__umulhi(n << 8, e & 0xffffffu);
      coef[JPEG_ZZ_OF[v * 8 + u]][lane] = (short)(q < 0 ? -c : c);
    }
  }
}

// The staging buffer's bit writer: most significant bit first, words flushed with atomic OR.
struct BitSink {
  unsigned long long acc;
  unsigned nacc;
  uint32_t *wp, *wend;
  __device__ __forceinline__ void start(uint32_t* stage, uint32_t* end, unsigned pos) {
    acc = 0ull;
    nacc = pos & 31u;            // the bits before pos in its word are a neighbour's: zeros here
    wp = stage + (pos >> 5);
    wend = end;
  }
  __device__ __forceinline__ void put(uint32_t v, unsigned n) {      // n <= 27
    acc = (acc << n) | v;
    nacc += n;
    if (nacc >= 32u) {
      nacc -= 32u;
      if (wp < wend) atomicOr(wp, (uint32_t)(acc >> nacc));
      ++wp;
    }
  }
  __device__ __forceinline__ void finish() {
    if (nacc > 0u && wp < wend) atomicOr(wp, (uint32_t)acc << (32u - nacc));
  }
};

__device__ __forceinline__ unsigned jpeg_category(int v) { return 32u - (unsigned)__clz(abs(v)); }      // 0 for 0

// The codes of one block whose coefficients (the DC already a difference) are coef[k][lane]; returns their bit count.
template <bool EMIT>
__device__ __forceinline__ unsigned jpeg_walk(const short (*coef)[64], int lane, const uint32_t* __restrict__ dct,
                                              const uint32_t* __restrict__ act, BitSink& sink) {
  unsigned bits = 0;
  auto emit = [&](uint32_t entry, int value, unsigned s) {
    const unsigned n = (entry >> 16) + s;
    bits += n;
    // a negative value is sent as value - 1 in s bits
    if (EMIT) sink.put(((entry & 0xffffu) << s) | ((unsigned)(value + (value >> 31)) & ((1u << s) - 1u)), n);
  };
  const int diff = coef[0][lane];
  const unsigned sd = min(jpeg_category(diff), 15u);
  emit(dct[sd], diff, sd);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    const int c = coef[k][lane];
    if (c == 0) {
      ++run;
      continue;
    }
    while (run >= 16) {
      emit(act[0xf0], 0, 0u);           // ZRL
      run -= 16;
    }
    const unsigned s = jpeg_category(c);       // <= 15 for an int16
    emit(act[(run << 4) | s], c, s);
    run = 0;
  }
  if (run > 0) emit(act[0x00], 0, 0u);  // EOB
  return bits;
}

template <int C, bool PACK>
__global__ __launch_bounds__(SPNET_WAVE) void jpeg_kernel(const JpegArgs a) {
  constexpr int STAGE_WORDS = (SPNET_WAVE * C * JPEG_BLOCK_BITS + 31) / 32;
  constexpr int NT = C == 1 ? 1 : 2;
  __shared__ uint32_t s_stage[STAGE_WORDS];
  __shared__ short s_coef[C][64][SPNET_WAVE];
  __shared__ uint32_t s_qm[NT][64];
  const int lane = threadIdx.x;
  const long n = blockIdx.x / (unsigned)a.n_int;
  const int i = (int)(blockIdx.x % (unsigned)a.n_int);

  long long o0 = 0, o1 = 0;
  if (PACK) {
    o0 = a.offsets[n];
    o1 = a.offsets[n + 1];
    if (o0 < 0 || o1 < o0 || o1 > (long long)a.out_bytes) return;        // (uniform) a slot outside the buffer: not written
  }

#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const unsigned Q = min(max((unsigned)a.qt[t * 64 + lane], 1u), 255u);
    s_qm[t][lane] = (Q << 24) | (0xffffffu / (2u * Q) + 1u);               // ceil(2^24 / 2Q)
  }
  __syncthreads();

  const int m0 = i * a.ri;
  const int cnt = min(a.ri, a.mcus - m0);                                  // >= 1
  const bool active = lane < cnt;
  const int mcu = m0 + min(lane, cnt - 1);                                 // idle lanes redo the last MCU and keep nothing
  const int y0 = (mcu / a.mcu_w) * 8, x0 = (mcu % a.mcu_w) * 8;
  const unsigned char* frame = a.src + n * ((long)a.H * a.W * C);
  BitSink sink;

  unsigned bits = 0;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    const int t = c == 0 ? 0 : 1;
    jpeg_block<C>(frame, a.H, a.W, y0, x0, c, s_qm[NT == 1 ? 0 : t], s_coef[c], lane);
    const int dc = s_coef[c][0][lane];
    const int left = __shfl_up(dc, 1, SPNET_WAVE);
    s_coef[c][0][lane] = (short)(dc - (lane == 0 ? 0 : left));             // the predictor starts at 0 in every interval
    bits += jpeg_walk<false>(s_coef[c], lane, JPEG_DC[t].e, JPEG_AC[t].e, sink);
  }
  if (!active) bits = 0;
  unsigned incl = bits;
#pragma unroll
  for (int off = 1; off < SPNET_WAVE; off <<= 1) {
    const unsigned v = (unsigned)__shfl_up((int)incl, off, SPNET_WAVE);
    if (lane >= off) incl += v;
  }
  const unsigned total = (unsigned)__shfl((int)incl, SPNET_WAVE - 1, SPNET_WAVE);          // <= 64 * C * 1665 bits

  const int nwords = min((int)((total + 31u) >> 5), STAGE_WORDS);
  for (int w = lane; w < nwords; w += SPNET_WAVE) s_stage[w] = 0u;
  __syncthreads();
  if (active) {
    sink.start(s_stage, s_stage + STAGE_WORDS, incl - bits);
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
      const int t = c == 0 ? 0 : 1;
      jpeg_walk<true>(s_coef[c], lane, JPEG_DC[t].e, JPEG_AC[t].e, sink);
    }
    sink.finish();
  }
  if (lane == 0 && (total & 7u) && (int)(total >> 5) < STAGE_WORDS) {      // 1-bits up to the byte boundary
    const unsigned npad = 8u - (total & 7u);
    atomicOr(&s_stage[total >> 5], ((1u << npad) - 1u) << (32u - (total & 31u) - npad));
  }
  __syncthreads();

  const int nbytes = min((int)((total + 7u) >> 3), STAGE_WORDS * 4);
  unsigned long long at = 0;                                               // of the interval's first byte in `out`
  if (PACK) {
    unsigned long long before = 0;
    for (int k = lane; k < i; k += SPNET_WAVE) before += a.sizes_in[n * a.n_int + k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, SPNET_WAVE);
    at = (unsigned long long)o0 + before + 2ull * (unsigned)i;
  }
  unsigned stuffed = 0;
  for (int base = 0; base < nbytes; base += SPNET_WAVE) {
    const int j = base + lane;
    const unsigned b = j < nbytes ? (s_stage[j >> 2] >> (24 - 8 * (j & 3))) & 255u : 0u;
    const bool ff = b == 255u;
    const unsigned long long mask = __ballot(ff);
    if (PACK && j < nbytes) {
      const unsigned long long dst = at + (unsigned)j + stuffed + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
      if (dst < (unsigned long long)o1) a.out[dst] = (unsigned char)b;
      if (ff && dst + 1ull < (unsigned long long)o1) a.out[dst + 1ull] = 0;
    }
    stuffed += (unsigned)__popcll(mask);
  }
  const unsigned size = (unsigned)nbytes + stuffed;
  if (!PACK) {
    if (lane == 0) a.sizes_out[n * a.n_int + i] = size;
  } else if (i < a.n_int - 1 && lane < 2) {                                // RSTm, m = i mod 8; none after the last interval
    const unsigned long long dst = at + size + (unsigned)lane;
    if (dst < (unsigned long long)o1) a.out[dst] = lane == 0 ? (unsigned char)0xff : (unsigned char)(0xd0 + (i & 7));
  }
}

template <bool PACK>
int jpeg_launch(const JpegArgs& a, int N, int channels, void* stream) {
  const dim3 grid((unsigned)((long)N * a.n_int)), block(SPNET_WAVE);
  if (channels == 1) hipLaunchKernelGGL((jpeg_kernel<1, PACK>), grid, block, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL((jpeg_kernel<3, PACK>), grid, block, 0, (hipStream_t)stream, a);
  SPNET_RETURN_LAUNCH_STATUS();
}

JpegArgs jpeg_args(const unsigned char* src, int H, int W, const uint16_t* qt) {
  JpegArgs a = {};
  a.src = src; a.qt = qt; a.H = H; a.W = W;
  a.mcu_w = (W + 7) / 8; a.mcus = a.mcu_w * ((H + 7) / 8);
  a.ri = (int)jpeg_restart_interval(W); a.n_int = (int)jpeg_intervals(H, W);
  return a;
}

}  // namespace

extern "C" long spnet_jpeg_restart_interval(int W, int channels) {
  if (W < 1 || W > JPEG_MAX_DIM || (channels != 1 && channels != 3)) return -1;
  return jpeg_restart_interval(W);
}

extern "C" long spnet_jpeg_intervals(int H, int W, int channels) {
  if (!jpeg_shape_ok(0, H, W, channels)) return -1;
  return jpeg_intervals(H, W);
}

extern "C" int spnet_jpeg_scan(const unsigned char* src, int N, int H, int W, int channels, const uint16_t* qtables,
                               uint32_t* sizes, void* stream) {
  if (!jpeg_shape_ok(N, H, W, channels) || !src || !qtables || !sizes) return (int)hipErrorInvalidValue;
  if (((uintptr_t)qtables & 1) || ((uintptr_t)sizes & 3)) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  JpegArgs a = jpeg_args(src, H, W, qtables);
  a.sizes_out = sizes;
  return jpeg_launch<false>(a, N, channels, stream);
}

extern "C" int spnet_jpeg_pack(const unsigned char* src, int N, int H, int W, int channels, const uint16_t* qtables,
                               const uint32_t* sizes, const long long* offsets, unsigned char* out, long out_bytes,
                               void* stream) {
  if (!jpeg_shape_ok(N, H, W, channels) || !src || !qtables || !sizes || !offsets || !out) return (int)hipErrorInvalidValue;
  if (((uintptr_t)qtables & 1) || ((uintptr_t)sizes & 3) || ((uintptr_t)offsets & 7) || out_bytes < 0)
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  JpegArgs a = jpeg_args(src, H, W, qtables);
  a.sizes_in = sizes; a.offsets = offsets; a.out = out; a.out_bytes = out_bytes;
  return jpeg_launch<true>(a, N, channels, stream);
}
