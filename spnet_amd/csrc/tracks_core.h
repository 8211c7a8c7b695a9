// Antinode tracking: the parts that do not depend on where the arrays live.  The rule is stated beside the prototypes in
// spnet_hip.h ("Antinode tracks").  csrc/tracks.hip calls these from its link and rank kernels, one lane per detection;
// tools/tracks_host_check.cpp calls them over exact-size heap arrays, with the lanes in a loop, under AddressSanitizer.
//
// ORDER.  Candidates are compared by IoU = inter / union as the cross product inter_p * union_q > inter_q * union_p.
// A count is trusted only when 0 < inter <= min(area_i, area_j) -- every true intersection count is --, so that
// union = area_i + area_j - inter lies in [max(area), 2^32) and every product below stays under 2^63, whatever the arrays
// hold.  best_candidate scans in ascending index and replaces only on STRICTLY better: on equality the lower index wins.
//
// POINTER JUMPING.  anc[x] is an ancestor of x along prev (itself for a head), dist[x] the number of links between them.
// rank_init takes anc = prev where prev points INTO AN EARLIER FRAME (0 <= prev < (x / K) * K) and x itself otherwise, so
// whatever prev holds the graph is a forest whose every path runs to strictly earlier frames: at most N - 1 links.  One
// round reads (anc, dist) and writes (anc', dist') = (anc[anc[x]], dist[x] + dist[anc[x]]) into OTHER arrays; after r
// rounds anc[x] is the ancestor 2^r links up, or the head.  ceil(log2(max(N, 2))) rounds reach every head.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define TR_HD __host__ __device__ __forceinline__
#else
#define TR_HD inline
#endif

namespace tracks {

constexpr int MAX_K = 128, MAX_GAP = 8, MAX_DIM = 16384, IOU_ONE = 1024;
constexpr long MAX_FLAT = 0x7ffffffeL;             // N * K <= 2^31 - 2

TR_HD bool sizes_ok(long N, int K) { return N >= 0 && K >= 1 && K <= MAX_K && N * (long)K <= MAX_FLAT; }

// Rounds of pointer jumping for N frames: ceil(log2(max(N, 2))).
TR_HD int rank_rounds(long N) {
  int r = 1;
  while ((1L << r) < N) ++r;
  return r;
}

// A count that can be one: 0 < inter <= min(area_i, area_j).
TR_HD bool plausible(int inter, int area_i, int area_j) { return inter > 0 && inter <= area_i && inter <= area_j; }

// Eligible: inter > 0 and 1024 * inter >= iou_q * union.
TR_HD bool eligible(int inter, int area_i, int area_j, int iou_q) {
  if (!plausible(inter, area_i, area_j)) return false;
  const long long uni = (long long)area_i + area_j - inter;
  return (long long)IOU_ONE * inter >= (long long)iou_q * uni;
}

// Candidate p beats q (strictly).
TR_HD bool better(int inter_p, long long union_p, int inter_q, long long union_q) {
  return (long long)inter_p * union_q > (long long)inter_q * union_p;
}

// The best eligible candidate for one detection of area `area_self` among n others: candidate m has inter[m * stride],
// area area_other[m] and is open iff open_other[m] != 0.  -1 if none is eligible.
TR_HD int best_candidate(const int* inter, long stride, int n, int area_self, const int* area_other,
                         const unsigned char* open_other, int iou_q) {
  int best = -1, best_inter = 0;
  long long best_union = 1;
  for (int m = 0; m < n; ++m) {
    if (!open_other[m]) continue;
    const int in = inter[m * stride];
    if (!eligible(in, area_self, area_other[m], iou_q)) continue;
    const long long uni = (long long)area_self + area_other[m] - in;
    if (best < 0 || better(in, uni, best_inter, best_union)) {
      best = m;
      best_inter = in;
      best_union = uni;
    }
  }
  return best;
}

// The mutual best of two sides A and B, lane by lane.  inter: int32 [Ka][Kb], [i][j] = |S_a(i) ^ S_b(j)|; area_a, area_b
// and open_a, open_b the two sides' areas and open flags.  The linker's sides are the frames t and t + d of a pair
// (Ka = Kb = K; open: live with no successor / no predecessor yet), the score's are a frame's truth and prediction.
//   mutual_choose_a(i)  -> the best eligible open j for i, or -1 (also -1 when i is not open)
//   mutual_choose_b(j)  -> the best eligible open i for j, or -1
// and once ALL lanes have chosen (a barrier on the device): i <-> j iff best_a[i] == j and best_b[j] == i.
TR_HD int mutual_choose_a(const int* inter, int Kb, int i, const int* area_a, const int* area_b, const unsigned char* open_a,
                          const unsigned char* open_b, int iou_q) {
  if (!open_a[i]) return -1;
  return best_candidate(inter + (long)i * Kb, 1, Kb, area_a[i], area_b, open_b, iou_q);
}

TR_HD int mutual_choose_b(const int* inter, int Ka, int Kb, int j, const int* area_a, const int* area_b,
                          const unsigned char* open_a, const unsigned char* open_b, int iou_q) {
  if (!open_b[j]) return -1;
  return best_candidate(inter + j, Kb, Ka, area_b[j], area_a, open_a, iou_q);
}

// The mutual-best test for lane i of side A; the partner j, or -1.  best_a holds Ka entries, best_b Kb.
TR_HD int mutual_partner(const int* best_a, const int* best_b, int Kb, int i) {
  const int j = best_a[i];
  return (j >= 0 && j < Kb && best_b[j] == i) ? j : -1;
}

// prev of flat index x as an address: prev if it points into an earlier frame, else x (a head).
TR_HD int rank_init(const int* prev, int x, int K) {
  const int p = prev[x];
  return (p >= 0 && p < (x / K) * K) ? p : x;
}

// One round for flat index x over `total` detections.  anc_in is range-checked again: a value outside 0 .. total-1 counts
// as a head, so no array content can cause an access outside the arrays.
TR_HD void rank_jump(const int* anc_in, const int* dist_in, int* anc_out, int* dist_out, int x, int total) {
  const int a = anc_in[x];
  if (a < 0 || a >= total || a == x) {
    anc_out[x] = x;
    dist_out[x] = (a == x) ? dist_in[x] : 0;
    return;
  }
  const int aa = anc_in[a];
  anc_out[x] = (aa >= 0 && aa < total) ? aa : a;
  dist_out[x] = dist_in[x] + dist_in[a];
}

}  // namespace tracks
