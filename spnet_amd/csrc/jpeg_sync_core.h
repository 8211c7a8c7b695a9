// Huffman decoding of ONE restart interval by many lanes (self-synchronising decode), as code that uses nothing
// device-specific.  jpeg_decode_core.h decodes an interval serially; a file without restart markers is one interval, and
// this header cuts such an interval into segments that are decoded independently and then chained until the result IS
// the serial one.
//   csrc/jpeg_decode_sync.hip        runs it on the GPU: a workgroup per interval, a lane per segment
//   tools/jpeg_sync_host_check.cpp   runs the same functions with the lanes in a loop, over plain arrays of exact size
//
// SEGMENTS.  The interval's bytes [lo, hi) are cut into segments of seg_bytes (a multiple of 4, at least 4).  A segment
// OWNS every symbol (Huffman code and magnitude bits) whose FIRST BIT lies in one of its bytes; the last segment also owns
// whatever starts at or after hi (the symbol that finds the data exhausted).
// STATE between two symbols (SyncState): the position of the next symbol's first bit (byte in the blob, bit in the
// byte), the block's index inside the MCU (which selects the component and so the tables) and the zigzag position k (0:
// a DC symbol is next).  Positions are CANONICAL: a position at a byte boundary names the next DATA byte, never the 00
// stuffed behind an FF, so two states are the same decoder state exactly when their words are equal.
// ERRORS (BAD_CODE, BAD_INDEX, BAD_CATEGORY, INPUT_EXHAUSTED) end a lane's decode: nothing behind an error of the TRUE
// decode is written or reported, as in decode_interval.  For the chain an error is a CUT, not a state that is handed on:
// the lane's exit is then the guess of the next segment, so the lanes behind it keep what they found on their own.  (Most
// errors belong to a lane that started from a wrong guess; an error state handed from lane to lane would wipe out every
// synchronised lane behind it, one per round, and the chain would be serial.)  Whether a lane's decode ended in an
// error is counted beside its blocks, and the prefix sum tells every lane whether the true decode failed before it.
// FF 00.  The reader is jpeg_decode_core.h's (FF 00 is the byte FF, FF before anything else ends the data), bounded by the
// interval's end, not the segment's.  A segment whose first byte is the 00 stuffed behind the previous segment's FF
// guesses its start one byte later: a symbol cannot start inside that 00, and nobody owns one that would.
// EXACTNESS.  Segment 0 starts in the true state (bit 0 of lo, block 0, k 0), every other segment first from a guess (its
// first bit, block 0, k 0).  Then rounds: segment i takes segment i - 1's latest exit state as its entry state and
// decodes again only if that differs from the entry it last used; the rounds stop when nobody decoded again.  After round
// r segments 0 .. r have true entries (induction: segment 0 is true from the start, and a true entry gives a true exit),
// so the fixed point is the serial decode and there are at most as many rounds as segments.  States are compared WHOLE;
// a match of the bit position alone in another block phase is not a match.
// Every loop is bounded: a decode step consumes at least one bit or ends in an error, and the step count is capped by
// the bits the interval has left.
#pragma once
#include "jpeg_decode_core.h"

namespace jpegdec {

constexpr int SYNC_MIN_SEG = 4;
constexpr int SYNC_MAX_SEG = 4096;
// A lane reads fewer than this many bytes past the end of its segment: a symbol starts before the end, the refill
// before it takes at most 8 data bytes (16 with stuffing) and looks one byte ahead.
constexpr int SYNC_READ_AHEAD = 32;
constexpr int32_t SYNC_NOWHERE = INT32_MAX;      // own_end of an interval's last segment

struct SyncState {
  int32_t pos;       // byte of the blob that holds the next symbol's first bit
  uint32_t meta;     // bit in that byte (0: the most significant) | block in the MCU << 3 | k << 8
};
JPEGDEC_FN SyncState sync_state(int pos, int bit, int blk, int k) {
  SyncState s;
  s.pos = pos;
  s.meta = (uint32_t)bit | (uint32_t)blk << 3 | (uint32_t)k << 8;
  return s;
}
JPEGDEC_FN bool sync_same(SyncState a, SyncState b) { return a.pos == b.pos && a.meta == b.meta; }

// jpeg_decode_core.h's reader over p[0 ..], where p[x - org] is byte x of the blob (org 0: p is the blob; the kernel
// reads a copy of a window of the blob), and which of the bytes it took were FF: that is what it takes to name the blob
// position of the next bit.
struct SyncBits {
  Bits b;            // b.pos, b.end: relative to org
  uint32_t ff;       // bit j: the j-th last byte taken was an FF (and its stuffed 00 was passed over)
  int org;
};
JPEGDEC_FN void sync_refill(SyncBits& r) {       // refill(), byte for byte
  Bits& b = r.b;
#pragma unroll 1
  for (int i = 0; i < 8 && b.cnt <= 56 && b.pos < b.end; ++i) {
    const unsigned v = b.p[b.pos];
    if (v == 0xFFu) {
      if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) {
        ++b.pos;
      } else {
        b.end = b.pos;
        return;
      }
    }
    ++b.pos;
    b.buf |= (uint64_t)v << (56 - b.cnt);
    b.cnt += 8;
    r.ff = r.ff << 1 | (v == 0xFFu ? 1u : 0u);
  }
}
// The blob position of the byte that holds the next bit: the buffer holds (part of) the last nb bytes taken, each one
// blob byte, or two where it was an FF.  With an empty buffer that is the next byte to take: canonical in both cases.
JPEGDEC_FN int sync_byte(const SyncBits& r) {
  const int nb = (r.b.cnt + 7) >> 3;             // <= 8
  return r.org + r.b.pos - nb - __builtin_popcount(r.ff & ((1u << nb) - 1u));
}
JPEGDEC_FN int sync_bit(const SyncBits& r) { return (8 - (r.b.cnt & 7)) & 7; }

// The reader at state s.  false: the state names bits the data does not have (no state this header forms does).
JPEGDEC_FN bool sync_open(SyncBits& r, const unsigned char* p, int org, int hi, SyncState s) {
  r.b.p = p;
  r.b.pos = s.pos - org;
  r.b.end = hi - org;
  r.b.buf = 0;
  r.b.cnt = 0;
  r.ff = 0;
  r.org = org;
  sync_refill(r);
  const int bit = (int)(s.meta & 7u);
  if (bit > r.b.cnt) return false;
  if (bit) skip(r.b, bit);
  return true;
}

// Where a lane that knows nothing starts the segment whose first byte is `first` (> lo): its first bit, or one byte on
// where that byte is the 00 stuffed behind an FF; at or past the interval's end: the end.
JPEGDEC_FN SyncState sync_guess(const unsigned char* p, int org, int hi, int first) {
  if (first >= hi) return sync_state(hi, 0, 0, 0);
  const bool stuffed = p[first - 1 - org] == 0xFFu && p[first - org] == 0;
  return sync_state(stuffed ? first + 1 : first, 0, 0, 0);
}

JPEGDEC_FN int sync_blocks_per_mcu(const int* f) { return f[F_HS] * f[F_VS] + (f[F_COMPONENTS] == 3 ? 2 : 0); }
JPEGDEC_FN int sync_component(const int* f, int blk) {      // of block blk (< blocks per MCU) of an MCU
  const int luma = f[F_HS] * f[F_VS];
  return blk < luma ? 0 : blk - luma + 1;
}

// One symbol of the block in state (blk, k), with decode_block's rules in decode_block's order.  sink.dc(component,
// difference) / sink.ac(k, value) receive what it read; done: the symbol ended its block.  Returns a Status; k is then
// not a state.
template <class Sink>
JPEGDEC_FN int sync_symbol(SyncBits& r, const TableSet& set, const int* f, int blk, int& k, bool& done, Sink& sink) {
  const int c = sync_component(f, blk);
  done = false;
  sync_refill(r);
  if (k == 0) {
    const int s = symbol(r.b, set.t[(f[F_TABLES + c] & 1) * 2]);
    if (s < 0) return -s;
    if (s > 11) return BAD_CATEGORY;
    int d = 0;
    if (s) {
      d = receive_extend(r.b, s);
      if (d == INT32_MIN) return INPUT_EXHAUSTED;
    }
    sink.dc(c, d);
    k = 1;
    return OK;
  }
  const int rs = symbol(r.b, set.t[((f[F_TABLES + c] >> 4) & 1) * 2 + 1]);
  if (rs < 0) return -rs;
  const int run = rs >> 4, s = rs & 15;
  if (s == 0) {
    if (run != 15) {             // EOB
      done = true;
      return OK;
    }
    k += 16;                     // ZRL
    if (k > 64) return BAD_INDEX;
    done = k == 64;
    return OK;
  }
  if (s > 10) return BAD_CATEGORY;
  k += run;
  if (k > 63) return BAD_INDEX;
  const int v = receive_extend(r.b, s);
  if (v == INT32_MIN) return INPUT_EXHAUSTED;
  sink.ac(k, v);
  ++k;
  done = k == 64;
  return OK;
}

// What decode_interval checks before it reads anything: OK or BAD_ARGS (fi: iv[2], already known to be a file).
JPEGDEC_FN int sync_interval_ok(long blob_bytes, const int* iv, const int* f, int n_sets, long total_blocks) {
  if (!file_ok(f, n_sets, total_blocks)) return BAD_ARGS;
  if (iv[0] < 0 || iv[1] < iv[0] || (long)iv[1] > blob_bytes) return BAD_ARGS;
  if (iv[3] < 0 || iv[4] < 0 || (long)iv[3] + iv[4] > (long)f[F_MCU_W] * f[F_MCU_H]) return BAD_ARGS;
  return OK;
}
JPEGDEC_FN int sync_segments(const int* iv, int seg_bytes) {          // at least one: an empty interval is exhausted at once
  const int n = (int)(((long)iv[1] - iv[0] + seg_bytes - 1) / seg_bytes);
  return n < 1 ? 1 : n;
}
// Steps a lane can take from byte `pos` on: every step that is no error consumes a bit.
JPEGDEC_FN long sync_step_cap(int hi, int pos) { return pos < hi ? 8L * (hi - pos) + 2 : 2; }

struct SegScan {
  SyncState exit;
  int status;                    // the error that ended the lane's decode, or OK
  uint32_t blocks;               // blocks that FINISH in the segment
  uint32_t dc[3];                // per component: the sum of the DC differences read in it, modulo 2^32
};
// (the three sums are picked by comparisons, not indexed: an array indexed by c would live in scratch memory on the GPU)
JPEGDEC_FN void sync_add(uint32_t* sums, int c, int d) {
  sums[0] += c == 0 ? (uint32_t)d : 0u;
  sums[1] += c == 1 ? (uint32_t)d : 0u;
  sums[2] += c == 2 ? (uint32_t)d : 0u;
}
struct ScanSink {
  uint32_t* sums;
  JPEGDEC_FN void dc(int c, int d) { sync_add(sums, c, d); }
  JPEGDEC_FN void ac(int, int) {}
};

// The symbols that segment [.., own_end) owns when it is entered in state `in` (own_end SYNC_NOWHERE: the interval's last
// segment).  f: the file's record (file_ok); set: its table set.  Reads bytes of [in.pos, hi) only; writes nothing.
JPEGDEC_FN SegScan scan_segment(const unsigned char* p, int org, int hi, int own_end, const int* f, const TableSet& set,
                                SyncState in) {
  SegScan out;
  out.exit = in;
  out.status = OK;
  out.blocks = 0;
  out.dc[0] = out.dc[1] = out.dc[2] = 0;
  if (in.pos >= own_end) return out;                                    // nothing of this segment's
  out.status = INPUT_EXHAUSTED;                                         // (also what a spent step cap would mean)
  out.exit = sync_guess(p, org, hi, own_end);                           // an error cuts the chain
  SyncBits r;
  if (!sync_open(r, p, org, hi, in)) return out;
  const int bpm = sync_blocks_per_mcu(f);
  int blk = (int)(in.meta >> 3 & 31u), k = (int)(in.meta >> 8 & 127u);
  ScanSink sink = {out.dc};
#pragma unroll 1
  for (long n = sync_step_cap(hi, in.pos); n > 0; --n) {
    const int at = sync_byte(r);
    if (at >= own_end) {
      out.exit = sync_state(at, sync_bit(r), blk, k);
      out.status = OK;
      break;
    }
    bool done;
    const int st = sync_symbol(r, set, f, blk, k, done, sink);
    if (st != OK) {
      out.status = st;
      break;
    }
    if (done) {
      ++out.blocks;
      blk = blk + 1 == bpm ? 0 : blk + 1;
      k = 0;
    }
  }
  return out;
}

// The block with ordinal ord (0 <= ord < MCUs * blocks per MCU) of interval iv, as decode_interval places it.
JPEGDEC_FN long sync_block_of(const int* iv, const int* f, long ord) {
  const int hs = f[F_HS], vs = f[F_VS], mw = f[F_MCU_W], mh = f[F_MCU_H];
  const int bpm = sync_blocks_per_mcu(f);
  const long m = iv[3] + ord / bpm;
  const int j = (int)(ord % bpm);
  const int my = (int)(m / mw), mx = (int)(m - (long)my * mw);
  const int c = sync_component(f, j);
  if (c == 0) return (long)f[F_BLOCK0] + (long)(my * vs + j / hs) * (mw * hs) + mx * hs + j % hs;
  return (long)f[F_BLOCK0] + (long)mw * mh * hs * vs + (long)(c - 1) * mw * mh + (long)my * mw + mx;
}

struct WriteSink {
  int16_t* cur;                  // the block in progress
  uint32_t pred[3];
  JPEGDEC_FN void dc(int c, int d) {
    sync_add(pred, c, d);
    cur[0] = (int16_t)(uint16_t)(c == 0 ? pred[0] : c == 1 ? pred[1] : pred[2]);
  }
  JPEGDEC_FN void ac(int k, int v) { cur[NATURAL_OF[k]] = (int16_t)v; }
};

// The same symbols again, from the TRUE entry state `in`, into the workspace (zeroed; natural order; decode_interval's
// layout; DC values predicted).  ord: the ordinal of the block in progress at entry (blocks that finished in earlier
// segments); pred: the three predictors at entry (the DC differences of earlier segments, summed).  Not to be called for
// a lane behind an error of the true decode (a prefix sum over SegScan::status tells).  iv has passed sync_interval_ok.  A block that straddles segments is written by several lanes at disjoint k.  A block whose ordinal is
// at or beyond MCUs * blocks per MCU is never decoded or written: the lane that finishes the LAST block applies
// decode_interval's trailing-bytes rule and stops, which is what reports data left over (TRAILING_BYTES), and lanes
// entered behind it return OK and do nothing -- a sound file's last symbol may end a few pad bits into the next segment.
// Returns a Status; at most one lane of an interval returns a non-zero one, and it is decode_interval's.
JPEGDEC_FN int write_segment(const unsigned char* p, int org, const int* iv, int own_end, const int* f, const TableSet& set,
                             SyncState in, long ord, const uint32_t* pred, int16_t* coef) {
  const int hi = iv[1];
  const int bpm = sync_blocks_per_mcu(f);
  const long total = (long)iv[4] * bpm;
  if (in.pos >= own_end || ord < 0 || ord >= total) return OK;
  SyncBits r;
  if (!sync_open(r, p, org, hi, in)) return INPUT_EXHAUSTED;
  int blk = (int)(in.meta >> 3 & 31u), k = (int)(in.meta >> 8 & 127u);
  WriteSink sink;
  sink.cur = coef + sync_block_of(iv, f, ord) * 64;
  sink.pred[0] = pred[0];
  sink.pred[1] = pred[1];
  sink.pred[2] = pred[2];
#pragma unroll 1
  for (long n = sync_step_cap(hi, in.pos); n > 0; --n) {
    if (sync_byte(r) >= own_end) return OK;
    bool done;
    const int st = sync_symbol(r, set, f, blk, k, done, sink);
    if (st != OK) return st;
    if (done) {
      if (++ord == total) {
        sync_refill(r);
        return (r.org + r.b.pos < hi || r.b.cnt >= 8) ? TRAILING_BYTES : OK;
      }
      blk = blk + 1 == bpm ? 0 : blk + 1;
      k = 0;
      sink.cur = coef + sync_block_of(iv, f, ord) * 64;
    }
  }
  return INPUT_EXHAUSTED;        // (a spent step cap: every step consumed a bit, so the bits are gone)
}

}  // namespace jpegdec
