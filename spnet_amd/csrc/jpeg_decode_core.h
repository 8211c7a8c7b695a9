// The baseline JPEG decoder (ITU-T T.81) as code that uses nothing device-specific: the Huffman decoding of one restart
// interval with every bounds and rejection rule, the "islow" inverse DCT of one block, and the upsampling and colour rule of
// one pixel are written here once.
//   csrc/jpeg_decode.hip             runs them on the GPU: a lane per interval, a thread per block, a thread per 4 pixels
//   tools/jpeg_decode_host_check.cpp runs them over plain arrays of exact size, so that the bounds rules can be proven
//                                    with host sanitizers before anything malformed is handed to a GPU
// The arithmetic is specified beside the prototypes in include/spnet_hip.h; tests/helpers/jpeg_decode_ref.py restates it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEGDEC_FN __host__ __device__ inline
#else
#define JPEGDEC_FN inline
#endif

namespace jpegdec {

enum Status : int {
  OK = 0,
  BAD_CODE = 1,          // a bit pattern that is no code of the table
  BAD_INDEX = 2,         // a run that carries the coefficient index past 63
  BAD_CATEGORY = 3,      // a magnitude category above 11 (DC) or 10 (AC)
  INPUT_EXHAUSTED = 4,   // bits missing before the interval's MCUs are done
  TRAILING_BYTES = 5,    // a whole byte or more left over after the interval's MCUs
  BAD_ARGS = 6           // an entry of the interval / file tables that points outside the launch's arrays
};

// One Huffman table, as spnet_amd/jpeg.py's device_table lays it out (226 words); a table set is DC 0, AC 0, DC 1, AC 1.
struct Table {
  uint16_t look[256];    // length << 8 | symbol of every code of up to 8 bits, indexed by the next 8 bits; 0: longer / none
  int32_t maxcode[17];   // the largest code of each length 1 .. 16, -1: none; [0] unused
  int32_t valoff[17];    // index of the length's first symbol minus its first code
  uint8_t vals[256];
};
struct TableSet {
  Table t[4];
};
constexpr int TABLE_WORDS = 226;
static_assert(sizeof(Table) == 4 * TABLE_WORDS && sizeof(TableSet) == 16 * TABLE_WORDS, "the host builds this layout");

constexpr long JPEG_MAX_BLOB = (1L << 31) - 1024;       // bytes of a launch's blob: positions are 32-bit
constexpr long JPEG_MAX_BLOCKS = (1L << 31) / 64 - 1;    // blocks of a launch's workspace: fewer than 2^31 coefficients

constexpr int INTERVAL_INTS = 8;  // first byte, end byte, file, first MCU, MCUs, 0, 0, 0
constexpr int FILE_INTS = 16;      // components, hs, vs, MCU columns, MCU rows, table set, first block, 0,
                                   // (DC table | AC table << 4) x 3, quantisation table x 3, 0, 0
enum FileField { F_COMPONENTS = 0, F_HS, F_VS, F_MCU_W, F_MCU_H, F_TABLE_SET, F_BLOCK0, F_TABLES = 8, F_QUANT = 11 };

// natural index (row v, column u: v * 8 + u) of the k-th coefficient of the zigzag sequence
#if defined(__HIPCC__)
__device__
#endif
    const unsigned char NATURAL_OF[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                          41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                          30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// What a file record must satisfy before anything is read or written for it.  total_blocks: of the workspace.
JPEGDEC_FN bool file_ok(const int* f, int n_sets, long total_blocks) {
  const int nc = f[F_COMPONENTS], hs = f[F_HS], vs = f[F_VS], mw = f[F_MCU_W], mh = f[F_MCU_H];
  if (nc != 1 && nc != 3) return false;
  if (!((hs == 1 && vs == 1) || (nc == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
  if (mw < 1 || mh < 1 || mw > 8192 || mh > 8192) return false;                         // 65,535 / 8
  if (f[F_TABLE_SET] < 0 || f[F_TABLE_SET] >= n_sets) return false;
  const long blocks = (long)mw * mh * (hs * vs + (nc == 3 ? 2 : 0));
  if (f[F_BLOCK0] < 0 || (long)f[F_BLOCK0] + blocks > total_blocks) return false;
  for (int c = 0; c < 3; ++c)
    if (f[F_TABLES + c] & ~0x11) return false;
  return true;
}

// The bits of one interval: bytes lo .. hi - 1 of the blob, most significant bit first, in a left-aligned 64-bit buffer.
// FF 00 is the byte FF; an FF followed by anything else (or by the interval's end) ends the data.  No byte at or after hi
// is read; cnt counts REAL bits only, the buffer reads as zeros below them.
struct Bits {
  const unsigned char* p;
  int pos, end;
  uint64_t buf;
  int cnt;
};
JPEGDEC_FN void refill(Bits& b) {
#pragma unroll 1
  for (int i = 0; i < 8 && b.cnt <= 56 && b.pos < b.end; ++i) {
    const unsigned v = b.p[b.pos];
    if (v == 0xFFu) {
      if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) {
        ++b.pos;
      } else {
        b.end = b.pos;       // a marker, or FF as the last byte: nothing more is data (pos stays below the interval's end)
        return;
      }
    }
    ++b.pos;
    b.buf |= (uint64_t)v << (56 - b.cnt);
    b.cnt += 8;
  }
}
JPEGDEC_FN void skip(Bits& b, int n) {       // 1 <= n <= 16, n <= cnt
  b.buf <<= n;
  b.cnt -= n;
}

// The next symbol of table t, or -status.  Needs a refill before it (at least 16 bits in the buffer where the data has them).
JPEGDEC_FN int symbol(Bits& b, const Table& t) {
  const unsigned peek = (unsigned)(b.buf >> 48);
  const unsigned e = t.look[peek >> 8];
  int len, sym;
  if (e) {
    len = (int)(e >> 8);
    sym = (int)(e & 255u);
  } else {
    sym = -1;
    for (len = 9; len <= 16; ++len) {
      const int code = (int)(peek >> (16 - len));
      if (code <= t.maxcode[len]) {
        sym = t.vals[(t.valoff[len] + code) & 255];
        break;
      }
    }
    if (sym < 0) return -BAD_CODE;
  }
  if (len > b.cnt) return -INPUT_EXHAUSTED;
  skip(b, len);
  return sym;
}

// s magnitude bits (1 <= s <= 11) as the signed value they stand for (T.81 F.2.2.1 EXTEND), or INT32_MIN: bits missing.
JPEGDEC_FN int receive_extend(Bits& b, int s) {
  if (s > b.cnt) return INT32_MIN;
  const int v = (int)(b.buf >> (64 - s));
  skip(b, s);
  return (v >> (s - 1)) ? v : v - (1 << s) + 1;
}

// One block: coefficient k of the zigzag sequence to coef[NATURAL_OF[k]] (coef: 64 int16 that are ZERO on entry).  pred: the
// component's DC predictor.  Returns a Status.  Every pass of the AC loop raises k by at least 1.
JPEGDEC_FN int decode_block(Bits& b, const Table& dc, const Table& ac, int& pred, int16_t* coef) {
  refill(b);
  int s = symbol(b, dc);
  if (s < 0) return -s;
  if (s > 11) return BAD_CATEGORY;
  if (s) {
    const int d = receive_extend(b, s);
    if (d == INT32_MIN) return INPUT_EXHAUSTED;
    pred = (int)((unsigned)pred + (unsigned)d);      // (modulo 2^32: a damaged stream may add for ever)
  }
  coef[0] = (int16_t)(uint16_t)(unsigned)pred;
  for (int k = 1; k < 64;) {
    refill(b);
    const int rs = symbol(b, ac);
    if (rs < 0) return -rs;
    const int run = rs >> 4;
    s = rs & 15;
    if (s == 0) {
      if (run != 15) break;      // EOB
      k += 16;                   // ZRL
      if (k > 64) return BAD_INDEX;
      continue;
    }
    if (s > 10) return BAD_CATEGORY;
    k += run;
    if (k > 63) return BAD_INDEX;
    const int v = receive_extend(b, s);
    if (v == INT32_MIN) return INPUT_EXHAUSTED;
    coef[NATURAL_OF[k]] = (int16_t)v;
    ++k;
  }
  return OK;
}

// One restart interval.  iv: its INTERVAL_INTS; files: the file records (n_files of them); set: the table set of the
// interval's file (the caller holds it wherever it likes); coef: the whole workspace of total_blocks blocks, zeroed.
// Blocks of a component lie in raster order of its block grid (MCU columns * h wide), the components one after another.
// Reads blob[iv[0] .. iv[1]) only and writes only blocks of the interval's own MCUs.
JPEGDEC_FN int decode_interval(const unsigned char* blob, long blob_bytes, const int* iv, const int* files, int n_files,
                               int n_sets, const TableSet& set, int16_t* coef, long total_blocks) {
  const int fi = iv[2];
  if (fi < 0 || fi >= n_files) return BAD_ARGS;
  const int* f = files + (long)fi * FILE_INTS;
  if (!file_ok(f, n_sets, total_blocks)) return BAD_ARGS;
  const int nc = f[F_COMPONENTS], hs = f[F_HS], vs = f[F_VS], mw = f[F_MCU_W], mh = f[F_MCU_H];
  const int m0 = iv[3], mn = iv[4];
  if (iv[0] < 0 || iv[1] < iv[0] || (long)iv[1] > blob_bytes) return BAD_ARGS;
  if (m0 < 0 || mn < 0 || (long)m0 + mn > (long)mw * mh) return BAD_ARGS;
  if (mn == 0) return OK;
  Bits b;
  b.p = blob;
  b.pos = iv[0];
  b.end = iv[1];
  b.buf = 0;
  b.cnt = 0;
  int pred[3] = {0, 0, 0};
  const long luma_blocks = (long)mw * mh * hs * vs, chroma_blocks = (long)mw * mh;
  for (int m = m0; m < m0 + mn; ++m) {
    const int my = m / mw, mx = m - my * mw;
    for (int c = 0; c < nc; ++c) {
      const Table& dc = set.t[(f[F_TABLES + c] & 1) * 2];
      const Table& ac = set.t[((f[F_TABLES + c] >> 4) & 1) * 2 + 1];
      const int h = c == 0 ? hs : 1, v = c == 0 ? vs : 1;
      const long base = (long)f[F_BLOCK0] + (c == 0 ? 0 : luma_blocks + (c - 1) * chroma_blocks);
      for (int j = 0; j < h * v; ++j) {
        const int by = my * v + j / h, bx = mx * h + j % h;
        const long blk = base + (long)by * (mw * h) + bx;           // inside the file's blocks: file_ok, m < mw * mh
        const int st = decode_block(b, dc, ac, pred[c], coef + blk * 64);
        if (st != OK) return st;
      }
    }
  }
  refill(b);
  if (b.pos < iv[1] || b.cnt >= 8) return TRAILING_BYTES;
  return OK;
}

// ---- pixels
// libjpeg's jidctint.c ("islow"): CONST_BITS 13, PASS1_BITS 2; one pass over 8 values, descaled by `shift` (11 for the
// column pass, 18 for the row pass).  The sums are formed modulo 2^32 (unsigned: the same bits as libjpeg's on every
// stream an encoder can write, and defined behaviour on the absurd coefficients of a damaged one).
JPEGDEC_FN void idct_1d(const int* x, int* o, int shift) {
  typedef uint32_t U;
  const U x0 = (U)x[0], x1 = (U)x[1], x2 = (U)x[2], x3 = (U)x[3], x4 = (U)x[4], x5 = (U)x[5], x6 = (U)x[6], x7 = (U)x[7];
  U z1 = (x2 + x6) * 4433u;
  U tmp2 = z1 - x6 * 15137u;
  U tmp3 = z1 + x2 * 6270u;
  U tmp0 = (x0 + x4) << 13;
  U tmp1 = (x0 - x4) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  z1 = x7 + x1;
  U z2 = x5 + x3, z3 = x7 + x3, z4 = x5 + x1;
  const U z5 = (z3 + z4) * 9633u;
  tmp0 = x7 * 2446u;
  tmp1 = x5 * 16819u;
  tmp2 = x3 * 25172u;
  tmp3 = x1 * 12299u;
  z1 *= (U)-7373;
  z2 *= (U)-20995;
  z3 = z3 * (U)-16069 + z5;
  z4 = z4 * (U)-3196 + z5;
  tmp0 += z1 + z3;
  tmp1 += z2 + z4;
  tmp2 += z2 + z3;
  tmp3 += z1 + z4;
  const U r = (U)1 << (shift - 1);
  o[0] = (int)(tmp10 + tmp3 + r) >> shift;
  o[7] = (int)(tmp10 - tmp3 + r) >> shift;
  o[1] = (int)(tmp11 + tmp2 + r) >> shift;
  o[6] = (int)(tmp11 - tmp2 + r) >> shift;
  o[2] = (int)(tmp12 + tmp1 + r) >> shift;
  o[5] = (int)(tmp12 - tmp1 + r) >> shift;
  o[3] = (int)(tmp13 + tmp0 + r) >> shift;
  o[4] = (int)(tmp13 - tmp0 + r) >> shift;
}

JPEGDEC_FN int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// The chroma sample of pixel (y, x) from the component's own samples, fetch(row, column) over its dh x dw TRUE samples
// (dw = ceil(W / hs), dh = ceil(H / vs)): libjpeg's "fancy" (triangle) upsampling with the edges replicated.
template <class Fetch>
JPEGDEC_FN int chroma_at(Fetch fetch, int hs, int vs, int y, int x, int dh, int dw) {
  if (hs == 1) return fetch(y, x);
  const int i = x >> 1, odd = x & 1;
  int j = odd ? i + 1 : i - 1;
  j = j < 0 ? 0 : j > dw - 1 ? dw - 1 : j;
  if (vs == 1) return (3 * fetch(y, i) + fetch(y, j) + 1 + odd) >> 2;
  const int r = y >> 1;
  int rn = (y & 1) ? r + 1 : r - 1;
  rn = rn < 0 ? 0 : rn > dh - 1 ? dh - 1 : rn;
  const int here = 3 * fetch(r, i) + fetch(rn, i), next = 3 * fetch(r, j) + fetch(rn, j);
  return (3 * here + next + 8 - odd) >> 4;
}

// libjpeg's YCbCr -> RGB in 16-bit fixed point (jdcolor.c); cb, cr: the samples minus 128.
JPEGDEC_FN int red_of(int y, int cr) { return clamp255(y + ((91881 * cr + 32768) >> 16)); }
JPEGDEC_FN int green_of(int y, int cb, int cr) { return clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16)); }
JPEGDEC_FN int blue_of(int y, int cb) { return clamp255(y + ((116130 * cb + 32768) >> 16)); }

}  // namespace jpegdec
