// The mutual-best and identity steps of spnet_amd/csrc/track_score.hip over plain arrays: what track_match_kernel,
// ident_range_kernel and ident_walk_kernel do, with the workgroups and lanes in loops -- the same effective_ident and
// ident_walk of csrc/track_score_core.h and mutual_choose_a / mutual_choose_b / mutual_partner of csrc/tracks_core.h --
// over heap blocks of their exact size, so that a read or write outside inter, the areas, ident, track, match, eff or
// ident_stats is an AddressSanitizer report, and an overflowing product a UBSan report.  Beside each, a plain
// restatement is the oracle: an all-pairs search with 128-bit cross products for the mutual best, and for an identity
// the list of its frames built first and then read off.  The inputs are seeded, and hostile on purpose: idents below 0
// and above M, duplicates, tracks of any value, counts that are no counts, match entries that are no indices.
//
//   track_score_host_check         the built-in battery; prints "case NAME ... equal 1" per case and "all equal" at the
//                                  end; exit status 1 on the first difference
// Build: clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "track_score_core.h"

using namespace track_score;

namespace {

unsigned rng_state = 77u;
unsigned rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <class T>
T* exact(size_t n) { return (T*)malloc(sizeof(T) * (n ? n : 1)); }

typedef __int128 wide;

bool ref_eligible(wide in, wide ai, wide aj, int q) { return in > 0 && in <= ai && in <= aj && 1024 * in >= q * (ai + aj - in); }

int ref_best(const int* inter, long stride, int n, int a_self, const int* a_other, const unsigned char* open_other, int q) {
  for (int m = 0; m < n; ++m) {
    if (!open_other[m] || !ref_eligible(inter[m * stride], a_self, a_other[m], q)) continue;
    bool beaten = false;
    for (int o = 0; o < n && !beaten; ++o) {
      if (o == m || !open_other[o] || !ref_eligible(inter[o * stride], a_self, a_other[o], q)) continue;
      const wide im = inter[m * stride], io = inter[o * stride];
      const wide um = (wide)a_self + a_other[m] - im, uo = (wide)a_self + a_other[o] - io;
      const wide lhs = io * um, rhs = im * uo;
      beaten = lhs > rhs || (lhs == rhs && o < m);
    }
    if (!beaten) return m;
  }
  return -1;
}

int hostile_int(int lo, int hi) {                                       // mostly lo .. hi, now and then far outside
  const unsigned r = rng() % 16;
  if (r == 0) return INT_MIN + (int)(rng() % 3);
  if (r == 1) return INT_MAX - (int)(rng() % 3);
  if (r == 2) return lo - 1 - (int)(rng() % 5);
  if (r == 3) return hi + 1 + (int)(rng() % 5);
  return lo + (int)(rng() % (unsigned)(hi - lo + 1));
}

// One movie: N frames, Kt truth rows, Kp predicted rows, M identities.  Returns 1 when the device's way and the plain
// restatement agree on match, frame_counts and ident_stats.
int run_case(const char* name, int N, int Kt, int Kp, int M, int iou_q, bool huge_counts) {
  int* inter = exact<int>((size_t)N * Kt * Kp);
  int* area_t = exact<int>((size_t)N * Kt);
  int* area_p = exact<int>((size_t)N * Kp);
  int* ident = exact<int>((size_t)N * Kt);
  int* track = exact<int>((size_t)N * Kp);
  unsigned char* live_t = exact<unsigned char>((size_t)N * Kt);
  unsigned char* live_p = exact<unsigned char>((size_t)N * Kp);
  int* match = exact<int>((size_t)N * Kt);
  int* counts = exact<int>((size_t)N * 3);
  int* eff = exact<int>((size_t)N * Kt);
  int* stats = exact<int>((size_t)(M + 1) * STATS);
  int* first = exact<int>(M + 1);
  int* last = exact<int>(M + 1);
  const int amax = huge_counts ? INT_MAX : 400;
  for (long x = 0; x < (long)N * Kt; ++x) {
    area_t[x] = 1 + (int)(rng() % (unsigned)amax);
    ident[x] = hostile_int(0, M < 12 ? M : 12);
    live_t[x] = rng() % 8 != 0;
  }
  for (long x = 0; x < (long)N * Kp; ++x) {
    area_p[x] = 1 + (int)(rng() % (unsigned)amax);
    track[x] = hostile_int(0, 5);
    live_p[x] = rng() % 8 != 0;
  }
  for (long x = 0; x < (long)N * Kt * Kp; ++x)
    inter[x] = rng() % 3 == 0 ? 0 : huge_counts ? hostile_int(0, INT_MAX - 8) : hostile_int(0, 300);

  // ---- as the device does: per frame, lanes in any order, a "barrier" between the steps
  int equal = 1;
  for (int n = 0; n < N; ++n) {
    const int* in = inter + (long)n * Kt * Kp;
    unsigned char* open_t = exact<unsigned char>(Kt);
    unsigned char* open_p = exact<unsigned char>(Kp);
    int* fwd = exact<int>(Kt);
    int* bwd = exact<int>(Kp);
    for (int k = Kt - 1; k >= 0; --k) {
      eff[(long)n * Kt + k] = effective_ident(ident + (long)n * Kt, live_t + (long)n * Kt, k, M);
      open_t[k] = eff[(long)n * Kt + k] ? 1 : 0;
    }
    for (int k = 0; k < Kp; ++k) open_p[k] = (live_p[(long)n * Kp + k] && track[(long)n * Kp + k] > 0) ? 1 : 0;
    for (int k = Kt - 1; k >= 0; --k) fwd[k] = tracks::mutual_choose_a(in, Kp, k, area_t + (long)n * Kt, area_p + (long)n * Kp, open_t, open_p, iou_q);
    for (int k = Kp - 1; k >= 0; --k) bwd[k] = tracks::mutual_choose_b(in, Kt, Kp, k, area_t + (long)n * Kt, area_p + (long)n * Kp, open_t, open_p, iou_q);
    int tp = 0, nt = 0, np = 0;
    for (int k = 0; k < Kt; ++k) {
      match[(long)n * Kt + k] = tracks::mutual_partner(fwd, bwd, Kp, k);
      tp += match[(long)n * Kt + k] >= 0;
      nt += open_t[k];
    }
    for (int k = 0; k < Kp; ++k) np += open_p[k];
    counts[n * 3] = tp; counts[n * 3 + 1] = nt - tp; counts[n * 3 + 2] = np - tp;

    // the restatement of this frame
    for (int i = 0; i < Kt; ++i) {
      int want = -1;
      if (open_t[i]) {
        const int j = ref_best(in + (long)i * Kp, 1, Kp, area_t[(long)n * Kt + i], area_p + (long)n * Kp, open_p, iou_q);
        if (j >= 0 && ref_best(in + j, Kp, Kt, area_p[(long)n * Kp + j], area_t + (long)n * Kt, open_t, iou_q) == i) want = j;
      }
      if (want != match[(long)n * Kt + i]) equal = 0;
      // the effective identity by definition
      int e = 0;
      const int g = ident[(long)n * Kt + i];
      if (live_t[(long)n * Kt + i] && g >= 1 && g <= M) {
        e = g;
        for (int o = 0; o < i; ++o)
          if (live_t[(long)n * Kt + o] && ident[(long)n * Kt + o] == g) e = 0;
      }
      if (e != eff[(long)n * Kt + i]) equal = 0;
    }
    free(open_t); free(open_p); free(fwd); free(bwd);
  }

  // a hostile match array for the identity pass: entries that are no indices count as unmatched
  for (long x = 0; x < (long)N * Kt; ++x)
    if (rng() % 6 == 0) match[x] = hostile_int(-1, Kp - 1);

  // ---- the identity pass as the device does it: ranges by min / max, then one lane per identity
  for (int g = 0; g <= M; ++g) { first[g] = -1; last[g] = -1; }         // first as uint32: all ones
  for (int n = N - 1; n >= 0; --n)
    for (int k = 0; k < Kt; ++k) {
      const int g = eff[(long)n * Kt + k];
      if (!g) continue;
      if ((unsigned)n < (unsigned)first[g]) first[g] = n;
      if (n > last[g]) last[g] = n;
    }
  for (int c = 0; c < STATS; ++c) stats[c] = 0;
  for (int g = M; g >= 1; --g)
    ident_walk(eff, match, track, N, Kt, Kp, g, (long)(unsigned)first[g], last[g], stats + (long)g * STATS);

  // the restatement: the list of (frame, matched, track) of every identity, then read off
  for (int g = 1; g <= M; ++g) {
    std::vector<int> frames, tracks_;
    std::vector<bool> matched;
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < Kt; ++k)
        if (eff[(long)n * Kt + k] == g) {
          const int m = match[(long)n * Kt + k];
          const bool ok = m >= 0 && m < Kp;
          frames.push_back(n);
          matched.push_back(ok);
          tracks_.push_back(ok ? track[(long)n * Kp + m] : 0);
        }
    int want[STATS] = {(int)frames.size(), 0, 0, 0, -1};
    int prev = -1;                                                      // the previous matched entry of the list
    for (size_t e = 0; e < frames.size(); ++e) {
      if (!matched[e]) continue;
      ++want[1];
      if (prev < 0) want[4] = frames[e];
      if (prev >= 0 && tracks_[e] != tracks_[prev]) ++want[2];
      if (prev >= 0 && (size_t)prev + 1 < e) ++want[3];                 // a present, unmatched entry lies between
      prev = (int)e;
    }
    for (int c = 0; c < STATS; ++c)
      if (want[c] != stats[(long)g * STATS + c]) equal = 0;
  }
  printf("case %s N %d Kt %d Kp %d M %d iou_q %d ... equal %d\n", name, N, Kt, Kp, M, iou_q, equal);
  free(inter); free(area_t); free(area_p); free(ident); free(track); free(live_t); free(live_p); free(match); free(counts);
  free(eff); free(stats); free(first); free(last);
  return equal;
}

}  // namespace

int main() {
  int ok = 1;
  const int Ks[] = {1, 2, 7, 128};
  const int Ms[] = {1, 7, 300, MAX_M};
  const int qs[] = {1, 256, 1024};
  int id = 0;
  for (int Kt : Ks)
    for (int Kp : Ks)
      for (int M : Ms)
        for (int q : qs) {
          if ((id++ % 3) && Kt * Kp > 900) continue;                    // the large tables now and then only
          char name[32];
          snprintf(name, sizeof name, "seeded %d", id);
          const int N = M == MAX_M ? 2 : 1 + (int)(rng() % 9);
          ok &= run_case(name, N, Kt, Kp, M, q, false);
          ok &= run_case(name, N, Kt, Kp, M, q, true);
          if (!ok) return 1;
        }
  ok &= run_case("no frames", 0, 4, 4, 3, 256, false);
  ok &= run_case("long movie, few identities", 400, 3, 4, 2, 128, false);
  if (!sizes_ok(0, 1, 1) || sizes_ok(1L << 17, 128, 128) || sizes_ok(2, 0, 1) || sizes_ok(2, 1, 129) || idents_ok(0) ||
      idents_ok(MAX_M + 1) || !idents_ok(MAX_M))
    ok = 0;
  printf("case limits ... equal %d\n", ok);
  if (!ok) return 1;
  printf("all equal\n");
  return 0;
}
