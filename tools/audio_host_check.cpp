// note_envelopes_kernel of spnet_amd/csrc/audio.hip over plain arrays: the workgroups, waves and lanes in loops, the same
// start / group_frames / group_span / sample / pack_trig / lane_sums of csrc/audio_core.h, with the three LDS tables as
// heap blocks of their EXACT size in use (span, Wn, 4096) and pcm, len, re, im of their exact size, so that a read or write
// outside any of them is an AddressSanitizer report and an overflowing sum a UBSan report.  Beside it the rule as a naive
// triple loop over __int128 is the oracle.
//
//   audio_host_check               the built-in battery; prints "case NAME ... equal 1" per case and "all equal" at the
//                                  end; exit status 1 on the first difference
// Build: clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc tools/audio_host_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "audio_core.h"

using namespace audio;

namespace {

unsigned rng_state = 2025u;
unsigned rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <class T>
T* exact(size_t n) { return (T*)malloc(sizeof(T) * (n ? n : 1)); }

typedef __int128 wide;

struct Case {
  const char* name;
  int S, T, Wn, K;
  long L, offset, hop_num, hop_den;
  int fill;                       // 0: random samples, 1: all -32768 with step 0 and a window of 32767 (the magnitude bound)
};

// the launch as the device runs it; returns false if a group would not fit its table
bool as_the_device_does(const Case& c, const int16_t* pcm, const int* len, const int16_t* win, const uint32_t* step,
                        const int16_t* ctab, long long* re, long long* im) {
  const int frames = group_frames(c.hop_num, c.hop_den, c.Wn);
  const int groups = (int)((c.T + frames - 1) / frames);
  for (int s = c.S - 1; s >= 0; --s)                                     // any block order
    for (int g = groups - 1; g >= 0; --g) {
      const long t0 = (long)g * frames;
      const int nf = (int)(c.T - t0 < frames ? c.T - t0 : frames);
      const long n0 = start(t0, c.offset, c.hop_num, c.hop_den);
      const long span = group_span(t0, nf, c.offset, c.hop_num, c.hop_den, c.Wn);
      if (nf < 1 || span > SPAN_MAX) return false;
      int16_t* s_x = exact<int16_t>(span);
      int16_t* s_win = exact<int16_t>(c.Wn);
      uint32_t* s_trig = exact<uint32_t>(TAB);
      const long ln = clamp_len(len[s], c.L);
      for (int tid = 0; tid < THREADS; ++tid) {
        for (int j = tid; j < (int)span; j += THREADS) s_x[j] = sample(pcm + (long)s * c.L, ln, n0 + j);
        for (int j = tid; j < c.Wn; j += THREADS) s_win[j] = win[j];
        for (int j = tid; j < TAB; j += THREADS) s_trig[j] = pack_trig(ctab, j);
      }
      for (int wave = 0; wave < WAVES; ++wave)
        for (int unit = wave; unit < nf * c.K; unit += WAVES) {
          const int f = unit / c.K, k = unit - f * c.K;
          const int off = (int)(start(t0 + f, c.offset, c.hop_num, c.hop_den) - n0);
          long long r = 0, m = 0;
          for (int lane = WAVE - 1; lane >= 0; --lane) {                 // the reduction in another order
            long long lr, lm;
            lane_sums(s_x + off, s_win, c.Wn, s_trig, step[k], lane, &lr, &lm);
            r += lr;
            m += lm;
          }
          const long o = (((long)s * c.T) + t0 + f) * c.K + k;
          re[o] = r;
          im[o] = m;
        }
      free(s_x);
      free(s_win);
      free(s_trig);
    }
  return true;
}

bool run(const Case& c) {
  int16_t* pcm = exact<int16_t>((size_t)c.S * c.L);
  int* len = exact<int>(c.S);
  int16_t* win = exact<int16_t>(c.Wn);
  uint32_t* step = exact<uint32_t>(c.K);
  int16_t* ctab = exact<int16_t>(TAB);
  const size_t total = (size_t)c.S * c.T * c.K;
  long long* re = exact<long long>(total);
  long long* im = exact<long long>(total);
  for (size_t i = 0; i < (size_t)c.S * c.L; ++i) pcm[i] = c.fill ? (int16_t)-32768 : (int16_t)(rng() & 0xffff);
  for (int s = 0; s < c.S; ++s) len[s] = s == 0 ? (int)c.L : s == 1 ? 0 : s == 2 ? 50 : s == 3 ? -7 : (int)c.L + 1000;
  if (c.fill) for (int s = 0; s < c.S; ++s) len[s] = (int)c.L;
  for (int i = 0; i < c.Wn; ++i)
    win[i] = c.fill ? (int16_t)32767 : (int16_t)lrint(32767.0 * 0.5 * (1.0 - cos(2.0 * M_PI * i / c.Wn)));
  for (int i = 0; i < TAB; ++i) ctab[i] = (int16_t)lrint(16384.0 * cos(2.0 * M_PI * i / TAB));
  for (int k = 0; k < c.K; ++k) step[k] = c.fill ? 0u : (k == 0 ? 0xffffffffu : (rng() << 8) ^ rng());
  memset(re, 0x5a, sizeof(long long) * total);
  memset(im, 0x5a, sizeof(long long) * total);

  bool ok = limits_ok(c.S, c.L, c.T, c.offset, c.hop_num, c.hop_den, c.Wn, c.K) &&
            as_the_device_does(c, pcm, len, win, step, ctab, re, im);
  for (int s = 0; ok && s < c.S; ++s)
    for (int t = 0; ok && t < c.T; ++t)
      for (int k = 0; ok && k < c.K; ++k) {
        const long ln = len[s] < 0 ? 0 : len[s] > c.L ? c.L : len[s];
        const long st = c.offset + (long)(((wide)t * c.hop_num) / c.hop_den);
        wide r = 0, m = 0;
        for (int i = 0; i < c.Wn; ++i) {
          const long n = st + i;
          const wide x = (n >= 0 && n < ln) ? pcm[(long)s * c.L + n] : 0;
          const uint32_t q = (uint32_t)((uint32_t)i * step[k]) >> 20;
          r += x * win[i] * ctab[q];
          m += x * win[i] * ctab[(q + 3072) & 4095];
        }
        const long o = (((long)s * c.T) + t) * c.K + k;
        ok = (wide)re[o] == r && (wide)im[o] == m;
      }
  printf("case %s ... equal %d\n", c.name, ok ? 1 : 0);
  free(pcm); free(len); free(win); free(step); free(ctab); free(re); free(im);
  return ok;
}

}  // namespace

int main() {
  const Case cases[] = {
      {"hop 1/1, Wn 64, K 1", 5, 37, 64, 1, 300, 0, 1, 1, 0},
      {"hop 441/10, Wn 192, K 5, offset -100", 5, 37, 192, 5, 2000, -100, 441, 10, 0},
      {"hop 300/1 (gaps), Wn 64, K 3", 5, 9, 64, 3, 2500, 0, 300, 1, 0},
      {"offset past the end", 3, 5, 64, 2, 500, 490, 240, 1, 0},
      {"offset far outside", 2, 3, 64, 2, 100, -(1L << 40), 7, 3, 0},
      {"hop 240, Wn 2048, K 7", 2, 19, 2048, 7, 6000, 0, 240, 1, 0},
      {"span edge: hop 1463/1 with Wn 2048 (8 frames fit exactly or not)", 1, 17, 2048, 2, 30000, 3, 1463, 1, 0},
      {"span edge: hop 10239/7", 1, 17, 2047, 2, 30000, 3, 10239, 7, 0},
      {"huge hop, one frame a group", 1, 3, 8192, 1, 9000, 0, 2147483647, 1, 0},
      {"Wn 8192, K 64, one frame", 1, 1, 8192, 64, 8192, 0, 1, 1, 0},
      {"the magnitude bound: all -32768, step 0, window 32767, Wn 8192", 1, 2, 8192, 2, 9000, 0, 5, 1, 1},
  };
  for (const Case& c : cases)
    if (!run(c)) return 1;
  // the SPAN claim over a sweep of hops and windows: no group of group_frames frames exceeds the table
  for (long num = 1; num <= 40000; num += 37)
    for (long den : {1L, 3L, 7L, 1000L})
      for (int Wn : {64, 2047, 2048, 8192}) {
        const int fr = group_frames(num, den, Wn);
        for (long t0 = 0; t0 < 64; t0 += fr)
          if (group_span(t0, fr, -5, num, den, Wn) > SPAN_MAX) {
            printf("span: hop %ld/%ld Wn %d frames %d exceeds the table\n", num, den, Wn, fr);
            return 1;
          }
      }
  printf("all equal\n");
  return 0;
}
