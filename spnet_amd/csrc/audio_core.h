// Note envelopes: the parts that do not depend on where the arrays live.  The rule is stated beside the prototype in
// spnet_hip.h ("Note envelopes").  csrc/audio.hip calls these from its one kernel; tools/audio_host_check.cpp calls them
// over exact-size heap arrays, with the workgroups, waves and lanes in loops, under AddressSanitizer and UBSan.
//
// A WORKGROUP takes one recording s and a GROUP of nf <= frames consecutive frames t0 .. t0 + nf - 1.  Its three tables:
//   x     the recording's samples n0 .. n0 + span - 1, n0 = start(t0), zero outside 0 .. len-1        int16 [span]
//   win   the window                                                                                   int16 [Wn]
//   trig  cos and sin of table position q in ONE word: low half ctab[q], high half ctab[(q + 3072) & 4095]   [4096]
// so that a term costs two contiguous 16-bit reads and ONE data-dependent read.  A UNIT is one (frame, note) of the group;
// the waves take the units round robin, a lane the terms i = lane, lane + 64, ..: lane_sums.  The 64 partial sums of a
// unit are added by the caller (a shuffle reduction on the device); integer addition is associative, so any order gives
// the same 64 bits.
//
// SPAN.  start(t) = offset + floor(t hop_num / hop_den) does not decrease with t, and floor(a + b) - floor(a) <= floor(b)
// + 1, so a group of nf frames spans at most floor((nf - 1) hop_num / hop_den) + 1 + Wn samples: group_frames picks the
// largest nf in 1 .. MAX_FRAMES for which that is at most SPAN_MAX (nf = 1 always fits: Wn <= MAX_WN <= SPAN_MAX).  Frame
// f of the group reads x[off .. off + Wn - 1] with off = start(t0 + f) - n0 >= 0 and off + Wn <= span.
//
// BOUNDS OF THE SUMS.  |x win| <= 2^15 2^15 = 2^30 fits int32 for ANY two int16; a term is at most 2^30 2^15 = 2^45 in
// magnitude for any table content, and 8192 of them 2^58: int64 cannot overflow whatever the arrays hold.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AU_HD __host__ __device__ __forceinline__
#else
#define AU_HD inline
#endif

namespace audio {

constexpr int MAX_K = 64, MIN_WN = 64, MAX_WN = 8192, TAB = 4096, TAB_SHIFT = 20, QUARTER3 = 3072;
constexpr int SPAN_MAX = 12288, MAX_FRAMES = 8, THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;
constexpr long MAX_T = 1L << 20, MAX_I32 = 0x7fffffffL, MAX_OFFSET = 1L << 40;

AU_HD bool limits_ok(long S, long L, long T, long offset, long hop_num, long hop_den, long Wn, long K) {
  if (S < 0 || T < 1 || T > MAX_T || K < 1 || K > MAX_K || Wn < MIN_WN || Wn > MAX_WN || L < 1 || L > MAX_I32) return false;
  if (hop_num < 1 || hop_num > MAX_I32 || hop_den < 1 || hop_den > MAX_I32) return false;
  if (offset < -MAX_OFFSET || offset > MAX_OFFSET) return false;
  return S <= MAX_I32 / (T * K);                            // S T K <= 2^31 - 1; T K <= 2^26
}

// First sample of frame t's window.  t hop_num < 2^51 and is not negative: the division is the floor.
AU_HD long start(long t, long offset, long hop_num, long hop_den) { return offset + (t * hop_num) / hop_den; }

AU_HD int group_frames(long hop_num, long hop_den, int Wn) {
  int nf = 1;
  while (nf < MAX_FRAMES && (nf * hop_num) / hop_den + 1 + Wn <= SPAN_MAX) ++nf;
  return nf;
}

// Samples of the group t0 .. t0 + nf - 1: at most SPAN_MAX when nf <= group_frames (SPAN above).
AU_HD long group_span(long t0, int nf, long offset, long hop_num, long hop_den, int Wn) {
  return start(t0 + nf - 1, offset, hop_num, hop_den) - start(t0, offset, hop_num, hop_den) + Wn;
}

AU_HD long clamp_len(long len, long L) { return len < 0 ? 0 : len > L ? L : len; }

// Sample n of a recording row of `len` valid samples (already clamped to 0 .. L): zero outside.
AU_HD int16_t sample(const int16_t* row, long len, long n) { return (n >= 0 && n < len) ? row[n] : (int16_t)0; }

AU_HD uint32_t pack_trig(const int16_t* ctab, int q) {
  return (uint32_t)(uint16_t)ctab[q] | ((uint32_t)(uint16_t)ctab[(q + QUARTER3) & (TAB - 1)] << 16);
}

// The terms i = lane, lane + WAVE, .. of one unit: x points at the frame's first sample in the group's span.
AU_HD void lane_sums(const int16_t* x, const int16_t* win, int Wn, const uint32_t* trig, uint32_t step, int lane,
                     long long* re, long long* im) {
  long long r = 0, m = 0;
  uint32_t p = (uint32_t)lane * step;                       // (uint32)(i step), wrapping; advanced by WAVE step a term
  const uint32_t dp = (uint32_t)WAVE * step;
  for (int i = lane; i < Wn; i += WAVE, p += dp) {
    const int xw = (int)x[i] * (int)win[i];
    const uint32_t cs = trig[p >> TAB_SHIFT];
    r += (long long)xw * (int16_t)(cs & 0xffffu);
    m += (long long)xw * (int16_t)(cs >> 16);
  }
  *re = r;
  *im = m;
}

}  // namespace audio
