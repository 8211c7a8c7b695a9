// The link and rank steps of spnet_amd/csrc/tracks.hip over plain arrays: what track_link_kernel and the track_rank_*
// kernels do, with the workgroups and lanes in loops -- the same mutual_choose_a / mutual_choose_b / mutual_partner /
// rank_init / rank_jump of csrc/tracks_core.h -- over heap blocks of their exact size, so that a read or write outside
// inter, area, next, prev or the ping-pong halves is an AddressSanitizer report, and an overflowing product a UBSan report.
// Beside each, a plain restatement is the oracle: an all-pairs search with 128-bit cross products for the mutual best, a
// walk along the sanitised prev for heads and ages.
//
//   tracks_host_check              the built-in battery; prints "case NAME ... equal 1" per case and "all equal" at the
//                                  end; exit status 1 on the first difference
// Build (the test does): clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "tracks_core.h"

using namespace tracks;

namespace {

unsigned rng_state = 2024u;
unsigned rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

template <class T>
T* exact(size_t n) { return (T*)malloc(sizeof(T) * (n ? n : 1)); }

// ---- one frame pair as the kernel runs it (Ka = Kb there): all lanes choose, then (the barrier) the mutual test
void link_as_the_device_does(const int* inter, int Ka, int Kb, const int* area_a, const int* area_b, const unsigned char* open_a,
                             const unsigned char* open_b, int iou_q, int* link_of_i) {
  int* fwd = exact<int>(Ka);
  int* bwd = exact<int>(Kb);
  for (int tid = Ka + Kb - 1; tid >= 0; --tid) {                        // any lane order: the choices are independent
    if (tid < Ka) fwd[tid] = mutual_choose_a(inter, Kb, tid, area_a, area_b, open_a, open_b, iou_q);
    else bwd[tid - Ka] = mutual_choose_b(inter, Ka, Kb, tid - Ka, area_a, area_b, open_a, open_b, iou_q);
  }
  for (int i = 0; i < Ka; ++i) link_of_i[i] = mutual_partner(fwd, bwd, Kb, i);
  free(fwd);
  free(bwd);
}

typedef __int128 wide;

bool ref_eligible(wide in, wide ai, wide aj, int q) { return in > 0 && in <= ai && in <= aj && 1024 * in >= q * (ai + aj - in); }

// the best by definition: eligible, open, and no other eligible open candidate is better or equal-with-a-lower-index
int ref_best(const int* inter, long stride, int n, int a_self, const int* a_other, const unsigned char* open_other, int q) {
  for (int m = 0; m < n; ++m) {
    if (!open_other[m] || !ref_eligible(inter[m * stride], a_self, a_other[m], q)) continue;
    bool beaten = false;
    for (int o = 0; o < n && !beaten; ++o) {
      if (o == m || !open_other[o] || !ref_eligible(inter[o * stride], a_self, a_other[o], q)) continue;
      const wide im = inter[m * stride], io = inter[o * stride];
      const wide um = (wide)a_self + a_other[m] - im, uo = (wide)a_self + a_other[o] - io;
      const wide lhs = io * um, rhs = im * uo;                           // o beats m iff io / uo > im / um
      beaten = lhs > rhs || (lhs == rhs && o < m);
    }
    if (!beaten) return m;
  }
  return -1;
}

bool link_case(const char* name, int Ka, int Kb, int iou_q, int mode) {
  int* inter = exact<int>((size_t)Ka * Kb);
  int *aa = exact<int>(Ka), *ab = exact<int>(Kb), *got = exact<int>(Ka);
  unsigned char *oa = exact<unsigned char>(Ka), *ob = exact<unsigned char>(Kb);
  for (int k = 0; k < Ka; ++k) {
    aa[k] = mode == 2 ? 0x7fffffff : 1 + (int)(rng() % 400u);
    oa[k] = rng() % 4u != 0;
  }
  for (int k = 0; k < Kb; ++k) {
    ab[k] = mode == 2 ? 0x7fffffff : 1 + (int)(rng() % 400u);
    ob[k] = rng() % 4u != 0;
  }
  for (int i = 0; i < Ka; ++i)
    for (int j = 0; j < Kb; ++j) {
      int v;
      if (mode == 0) v = (rng() % 3u) ? 0 : (int)(rng() % (unsigned)((aa[i] < ab[j] ? aa[i] : ab[j]) + 1));   // true counts
      else if (mode == 1) v = (int)(rng() % 5u) * ((aa[i] < ab[j] ? aa[i] : ab[j]) / 4);                       // many exact ties
      else v = (int)(rng() << 8 ^ rng());                                                                      // hostile
      inter[i * Kb + j] = v;
    }
  link_as_the_device_does(inter, Ka, Kb, aa, ab, oa, ob, iou_q, got);
  bool equal = true;
  int links = 0;
  for (int i = 0; i < Ka; ++i) {
    int want = -1;
    if (oa[i]) {
      const int j = ref_best(inter + (long)i * Kb, 1, Kb, aa[i], ab, ob, iou_q);
      if (j >= 0 && ref_best(inter + j, Kb, Ka, ab[j], aa, oa, iou_q) == i) want = j;
    }
    equal = equal && got[i] == want;
    links += want >= 0;
  }
  for (int i = 0; i < Ka && equal; ++i)                                  // at most one predecessor
    for (int o = i + 1; o < Ka; ++o) equal = equal && (got[i] < 0 || got[i] != got[o]);
  printf("case link %s Ka %d Kb %d iou_q %d links %d equal %d\n", name, Ka, Kb, iou_q, links, equal ? 1 : 0);
  free(inter); free(aa); free(ab); free(got); free(oa); free(ob);
  return equal;
}

// ---- the rank step as spnet_track_rank runs it: init, rank_rounds(N) rounds between two halves, finish
void rank_as_the_device_does(const int* prev, int N, int K, int* head, int* age) {
  const int total = N * K;
  int* half[2][2] = {{exact<int>(total), exact<int>(total)}, {exact<int>(total), exact<int>(total)}};
  for (int x = 0; x < total; ++x) {
    const int a = rank_init(prev, x, K);
    half[0][0][x] = a;
    half[0][1][x] = a == x ? 0 : 1;
  }
  const int rounds = rank_rounds(N);
  for (int r = 0; r < rounds; ++r) {
    memset(half[(r + 1) & 1][0], 0xA5, sizeof(int) * total);            // a round writes every element it is read from
    memset(half[(r + 1) & 1][1], 0xA5, sizeof(int) * total);
    for (int x = total - 1; x >= 0; --x)
      rank_jump(half[r & 1][0], half[r & 1][1], half[(r + 1) & 1][0], half[(r + 1) & 1][1], x, total);
  }
  memcpy(head, half[rounds & 1][0], sizeof(int) * total);
  memcpy(age, half[rounds & 1][1], sizeof(int) * total);
  for (int h = 0; h < 2; ++h) { free(half[h][0]); free(half[h][1]); }
}

bool rank_case(const char* name, int N, int K, int mode) {
  const int total = N * K;
  int *prev = exact<int>(total), *head = exact<int>(total), *age = exact<int>(total);
  for (int x = 0; x < total; ++x) {
    const int t = x / K, k = x % K;
    if (mode == 0) prev[x] = t > 0 ? (t - 1) * K + k : -1;                          // K chains of length N
    else if (mode == 1) prev[x] = (t > 0 && rng() % 3u) ? (int)(rng() % (unsigned)(t * K)) : -1;   // a forest, gaps of any length
    else {                                                                          // hostile: anything at all
      const unsigned pick = rng() % 6u;
      prev[x] = pick == 0 ? x : pick == 1 ? total + (int)(rng() % 1000u) : pick == 2 ? -(int)(rng() % 1000u) - 2
              : pick == 3 ? (int)0x7fffffff : pick == 4 ? (int)(rng() % (unsigned)total) : -1;
    }
  }
  rank_as_the_device_does(prev, N, K, head, age);
  bool equal = true;
  int longest = 0;
  for (int x = 0; x < total; ++x) {
    int y = x, n = 0;
    for (;;) {                                                                      // the walk: strictly earlier frames
      const int p = prev[y];
      if (!(p >= 0 && p < (y / K) * K)) break;
      y = p;
      ++n;
    }
    equal = equal && head[x] == y && age[x] == n;
    longest = n > longest ? n : longest;
  }
  printf("case rank %s N %d K %d rounds %d longest %d equal %d\n", name, N, K, rank_rounds(N), longest, equal ? 1 : 0);
  free(prev); free(head); free(age);
  return equal;
}

}  // namespace

int main() {
  bool ok = true;
  const int ks[] = {1, 2, 4, 72, 128};
  const int qs[] = {1, 256, 1024};
  for (int K : ks)
    for (int q : qs) {
      ok = link_case("counts", K, K, q, 0) && ok;
      ok = link_case("ties", K, K, q, 1) && ok;
      ok = link_case("hostile", K, K, q, 2) && ok;
    }
  for (int mode = 0; mode < 3; ++mode) {                                 // a rectangle, both ways: the score's use of the matcher
    ok = link_case("rectangle", 7, 128, 256, mode) && ok;
    ok = link_case("rectangle", 72, 3, 256, mode) && ok;
  }
  const int ns[] = {1, 2, 3, 4, 5, 8, 9, 33, 40, 64, 65, 257};
  for (int N : ns) {
    ok = rank_case("chains", N, 3, 0) && ok;
    ok = rank_case("forest", N, 4, 1) && ok;
    ok = rank_case("hostile", N, 5, 2) && ok;
  }
  ok = (rank_rounds(1) == 1 && rank_rounds(2) == 1 && rank_rounds(3) == 2 && rank_rounds(4) == 2 && rank_rounds(5) == 3 &&
        rank_rounds(1L << 20) == 20 && rank_rounds((1L << 20) + 1) == 21) && ok;
  ok = (sizes_ok(0, 1) && sizes_ok(16777215, 128) && !sizes_ok(16777216, 128) && !sizes_ok(1, 0) && !sizes_ok(1, 129) &&
        !sizes_ok(-1, 4)) && ok;
  if (!ok) return 1;
  printf("all equal\n");
  return 0;
}
