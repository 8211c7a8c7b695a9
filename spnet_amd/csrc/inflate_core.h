// The zlib / deflate decoder (RFC 1950, RFC 1951) as ONE bit-level state machine that uses nothing device-specific: block
// headers, table construction, symbol decode, length / distance arithmetic and every bounds rule are written here once.
// How compressed bytes are fetched and how output bytes are put, copied and summed is left to an IO policy:
//   csrc/png_decode.hip           instantiates it over LDS (staged input, 32 KiB history window, lanes copy and flush)
//   tools/inflate_host_check.cpp  instantiates it over plain arrays, so that the bounds rules can be proven with host
//                                 sanitizers before anything malformed is handed to a GPU
//
// IO policy (all positions are 32-bit: a stream is shorter than 2^31 bytes, an output at most 2^27):
//   uint32_t in32(int pos)                 compressed bytes pos .. pos + 3, little-endian; the core only asks for
//                                          0 <= pos < in_len and ignores the bytes at or beyond in_len
//   void put(int op, unsigned byte)        output byte op (op < out_len is checked here)
//   void copy(int op, int dist, int len)   output bytes op .. op + len - 1 = the bytes dist back, in order (dist < len:
//                                          the pattern repeats); 1 <= dist <= op, dist <= 32768, op + len <= out_len
//   void produced(int op)                  op bytes are final (after every symbol): a window may flush here
//   uint32_t finish(int op)                the Adler-32 of the op bytes produced
//
// What is accepted is what zlib's inflate accepts: an over-subscribed code is an error, an incomplete one too unless it
// is a literal/length or distance code with a single 1-bit code (or no code at all: using it is then the error).
//
// Decode tables: a first-level table of LUT_BITS = 9 bits ((symbol << 4) | length, 0 = not here) answers every code of
// up to 9 bits in one lookup; longer codes (and unused patterns) fall back to the canonical walk over count[] / sym[].
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define INFLATE_FN __host__ __device__ inline
#else
#define INFLATE_FN inline
#endif

namespace inflate {

enum Status : int {
  OK = 0,
  BAD_HEADER = 1,        // zlib header: method, window size, preset dictionary, header check
  BAD_BLOCK_TYPE = 2,    // BTYPE 3
  BAD_STORED_LEN = 3,    // LEN / NLEN mismatch
  BAD_CODE = 4,          // over-subscribed or incomplete code, too many codes, bad repeat, no end-of-block code
  BAD_SYMBOL = 5,        // a bit pattern that is no code, or a length / distance symbol that does not exist
  BAD_DISTANCE = 6,      // a match that starts before the output does
  INPUT_EXHAUSTED = 7,
  OUTPUT_OVERFLOW = 8,   // more than out_len bytes
  OUTPUT_SHORT = 9,      // fewer than out_len bytes
  BAD_ADLER = 10,
  BAD_FILTER = 11,       // (png_decode.hip) PNG filter type above 4
  BAD_ARGS = 12          // (png_decode.hip) an extent outside the blob
};

constexpr int LUT_BITS = 9;
constexpr int LUT_SIZE = 1 << LUT_BITS;
constexpr int MAX_BITS = 15;
constexpr int MAX_LIT = 288;
constexpr int MAX_LENS = 320;     // 286 + 30, rounded up

struct Code {
  uint16_t lut[LUT_SIZE];         // (symbol << 4) | code length, 0: longer than LUT_BITS, or no code
  uint16_t count[MAX_BITS + 1];   // codes of each length
  uint16_t sym[MAX_LIT];          // symbols in canonical order
};

struct Tables {
  Code lit, dist;                 // dist also holds the code-length code while a dynamic header is read
  uint8_t len[MAX_LENS];
};

struct Bits {
  uint64_t buf;
  int cnt;                        // valid bits in buf
  int pos, end;                   // next compressed byte, number of compressed bytes
};

template <class IO>
INFLATE_FN void refill(IO& io, Bits& b) {
  if (b.cnt >= 32 || b.pos >= b.end) return;
  const int n = (b.end - b.pos < 4) ? (b.end - b.pos) : 4;
  uint32_t v = io.in32(b.pos);
  if (n < 4) v &= (1u << (8 * n)) - 1u;
  b.buf |= (uint64_t)v << b.cnt;
  b.cnt += 8 * n;
  b.pos += n;
}

INFLATE_FN uint32_t take(Bits& b, int n) {      // the caller has checked n <= b.cnt; n <= 16
  const uint32_t v = (uint32_t)b.buf & ((1u << n) - 1u);
  b.buf >>= n;
  b.cnt -= n;
  return v;
}

INFLATE_FN uint32_t reverse_bits(uint32_t code, int n) {
  uint32_t r = 0;
  for (int i = 0; i < n; ++i) {
    r = (r << 1) | (code & 1u);
    code >>= 1;
  }
  return r;
}

// The tables of the prefix code with lengths len[0 .. n).  must_complete: the code-length code (zlib's CODES).
INFLATE_FN int build(Code& c, const uint8_t* len, int n, bool must_complete) {
  for (int l = 0; l <= MAX_BITS; ++l) c.count[l] = 0;
  for (int s = 0; s < n; ++s) c.count[len[s] & 15] = (uint16_t)(c.count[len[s] & 15] + 1);
  for (int i = 0; i < LUT_SIZE; ++i) c.lut[i] = 0;
  int left = 1, maxl = 0;
  for (int l = 1; l <= MAX_BITS; ++l) {
    left <<= 1;
    left -= (int)c.count[l];
    if (left < 0) return BAD_CODE;                             // over-subscribed
    if (c.count[l]) maxl = l;
  }
  if (maxl == 0) return OK;                                    // no code: using it is the error
  if (left > 0 && (must_complete || maxl != 1)) return BAD_CODE;
  int offs[MAX_BITS + 2];
  offs[1] = 0;
  for (int l = 1; l <= MAX_BITS; ++l) offs[l + 1] = offs[l] + (int)c.count[l];
  for (int s = 0; s < n; ++s) {
    const int l = len[s] & 15;
    if (l) c.sym[offs[l]++] = (uint16_t)s;                     // offs[l] < offs[16] <= n <= MAX_LIT
  }
  uint32_t code = 0;
  int idx = 0;
  for (int l = 1; l <= LUT_BITS; ++l) {
    for (int k = 0; k < (int)c.count[l]; ++k) {
      const uint16_t e = (uint16_t)((c.sym[idx++] << 4) | l);
      for (uint32_t j = reverse_bits(code, l); j < (uint32_t)LUT_SIZE; j += (1u << l)) c.lut[j] = e;
      ++code;
    }
    code <<= 1;
  }
  return OK;
}

// The next symbol of code c, or -(status).  The caller has refilled: b.cnt >= 15 unless the input ends.
INFLATE_FN int decode(const Code& c, Bits& b) {
  const uint32_t e = c.lut[(uint32_t)b.buf & (LUT_SIZE - 1)];
  if (e) {
    const int l = (int)(e & 15u);
    if (l > b.cnt) return -INPUT_EXHAUSTED;
    b.buf >>= l;
    b.cnt -= l;
    return (int)(e >> 4);
  }
  int code = 0, first = 0, index = 0;
  for (int l = 1; l <= MAX_BITS; ++l) {
    if (l > b.cnt) return -INPUT_EXHAUSTED;
    code |= (int)((b.buf >> (l - 1)) & 1u);
    const int count = (int)c.count[l];
    if (code - count < first) {
      b.buf >>= l;
      b.cnt -= l;
      return (int)c.sym[index + (code - first)];               // index + code - first < index + count <= n
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -BAD_SYMBOL;
}

INFLATE_FN int fixed_tables(Tables& t) {
  for (int s = 0; s < 288; ++s) t.len[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
  for (int s = 0; s < 32; ++s) t.len[288 + s] = 5;
  const int st = build(t.lit, t.len, 288, false);              // complete; 286 and 287 are rejected as length symbols
  if (st) return st;
  return build(t.dist, t.len + 288, 32, false);                // complete; 30 and 31 are rejected as distance symbols
}

template <class IO>
INFLATE_FN int dynamic_tables(IO& io, Bits& b, Tables& t) {
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  refill(io, b);
  if (b.cnt < 14) return INPUT_EXHAUSTED;
  const int hlit = (int)take(b, 5) + 257, hdist = (int)take(b, 5) + 1, hclen = (int)take(b, 4) + 4;
  if (hlit > 286 || hdist > 30) return BAD_CODE;
  for (int i = 0; i < 19; ++i) t.len[i] = 0;
  for (int i = 0; i < hclen; ++i) {
    refill(io, b);
    if (b.cnt < 3) return INPUT_EXHAUSTED;
    t.len[order[i]] = (uint8_t)take(b, 3);
  }
  int st = build(t.dist, t.len, 19, true);
  if (st) return st;
  const int total = hlit + hdist;                              // <= 316 < MAX_LENS
  int i = 0;
  while (i < total) {                                          // every turn consumes a code or fails
    refill(io, b);
    const int s = decode(t.dist, b);
    if (s < 0) return -s;
    if (s < 16) {
      t.len[i++] = (uint8_t)s;
      continue;
    }
    const int nextra = (s == 16) ? 2 : (s == 17) ? 3 : 7;
    if (b.cnt < nextra) return INPUT_EXHAUSTED;
    const int rep = (int)take(b, nextra) + ((s == 18) ? 11 : 3);
    if (s == 16 && i == 0) return BAD_CODE;                    // nothing to repeat
    if (i + rep > total) return BAD_CODE;                      // (a run may cross from the literal lengths into the distance lengths)
    const uint8_t v = (s == 16) ? t.len[i - 1] : (uint8_t)0;
    for (int k = 0; k < rep; ++k) t.len[i++] = v;
  }
  if (t.len[256] == 0) return BAD_CODE;                        // no end-of-block code
  st = build(t.lit, t.len, hlit, false);
  if (st) return st;
  return build(t.dist, t.len + hlit, hdist, false);
}

// One zlib stream of in_len bytes into exactly out_len bytes.  Every loop consumes input or ends: a stored block is
// bounded by its 16-bit length, the symbol loop reads at least one bit per turn of a stream of finite length.
template <class IO>
INFLATE_FN int run(IO& io, Tables& t, int in_len, int out_len) {
  if (in_len < 0 || out_len < 0) return BAD_ARGS;
  Bits b;
  b.buf = 0;
  b.cnt = 0;
  b.pos = 0;
  b.end = in_len;
  int op = 0;

  refill(io, b);
  if (b.cnt < 16) return INPUT_EXHAUSTED;
  const uint32_t cmf = take(b, 8), flg = take(b, 8);
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) return BAD_HEADER;

  bool last = false, have_fixed = false;
  while (!last) {
    refill(io, b);
    if (b.cnt < 3) return INPUT_EXHAUSTED;
    last = take(b, 1) != 0u;
    const uint32_t type = take(b, 2);
    if (type == 3u) return BAD_BLOCK_TYPE;
    if (type == 0u) {
      take(b, b.cnt & 7);                                      // to the byte boundary
      refill(io, b);
      if (b.cnt < 32) return INPUT_EXHAUSTED;
      const uint32_t len = take(b, 16), nlen = take(b, 16);
      if ((len ^ 0xffffu) != nlen) return BAD_STORED_LEN;
      for (uint32_t k = 0; k < len; ++k) {
        refill(io, b);
        if (b.cnt < 8) return INPUT_EXHAUSTED;
        if (op >= out_len) return OUTPUT_OVERFLOW;
        io.put(op++, take(b, 8));
        if ((k & 255u) == 255u) io.produced(op);
      }
      io.produced(op);
      continue;
    }
    if (type == 1u) {
      if (!have_fixed) {
        const int st = fixed_tables(t);
        if (st) return st;
        have_fixed = true;
      }
    } else {
      have_fixed = false;
      const int st = dynamic_tables(io, b, t);
      if (st) return st;
    }
    for (;;) {
      refill(io, b);
      int s = decode(t.lit, b);
      if (s < 0) return -s;
      if (s < 256) {
        if (op >= out_len) return OUTPUT_OVERFLOW;
        io.put(op++, (unsigned)s);
      } else if (s == 256) {
        break;
      } else {
        s -= 257;
        if (s >= 29) return BAD_SYMBOL;
        int len, nextra;                                       // RFC 1951 3.2.5, computed: 3 .. 258
        if (s < 8) {
          len = 3 + s;
          nextra = 0;
        } else if (s == 28) {
          len = 258;
          nextra = 0;
        } else {
          nextra = (s - 4) >> 2;
          len = 3 + ((4 + (s & 3)) << nextra);
        }
        if (b.cnt < nextra) return INPUT_EXHAUSTED;
        len += (int)take(b, nextra);
        refill(io, b);
        const int d = decode(t.dist, b);
        if (d < 0) return -d;
        if (d >= 30) return BAD_SYMBOL;
        int dist, dextra;                                      // 1 .. 32768
        if (d < 4) {
          dist = 1 + d;
          dextra = 0;
        } else {
          dextra = (d >> 1) - 1;
          dist = 1 + ((2 + (d & 1)) << dextra);
        }
        if (b.cnt < dextra) return INPUT_EXHAUSTED;
        dist += (int)take(b, dextra);
        if (dist > op) return BAD_DISTANCE;
        if (len > out_len - op) return OUTPUT_OVERFLOW;
        io.copy(op, dist, len);
        op += len;
      }
      io.produced(op);
    }
  }
  if (op < out_len) return OUTPUT_SHORT;
  take(b, b.cnt & 7);
  refill(io, b);
  if (b.cnt < 32) return INPUT_EXHAUSTED;
  uint32_t want = 0;
  for (int k = 0; k < 4; ++k) want = (want << 8) | take(b, 8);
  return io.finish(op) == want ? OK : BAD_ADLER;
}

}  // namespace inflate
