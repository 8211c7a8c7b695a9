// Connected-component labelling of ring-count masks: the parts that do not depend on where the arrays live.  The rule is
// stated beside the prototypes in spnet_hip.h ("Mask fitting").  csrc/mask_fit.hip instantiates these templates over LDS
// and over global memory (atomics); tools/mask_fit_host_check.cpp instantiates them over exact-size heap arrays, with the
// lanes in a loop, under AddressSanitizer.
//
// THE UNION-FIND.  A parent store holds, per pixel, the index of another pixel of the same component that is NOT LARGER
// than the pixel's own index; a root is its own parent.  The only write is fetch_min(i, v) with v < i a pixel already
// proven to be in i's component, so two things hold at every moment, under any interleaving of any number of lanes:
//   (1) parents only decrease, and parent[i] <= i: every path i, parent[i], ... is strictly decreasing until it reaches a
//       root, so find_root ends after at most as many steps as the store has pixels (`bound`);
//   (2) a path never leaves its component.
// unite(a, b) is the lock-free form of Komura / Playne & Hawick: find both roots, hang the LARGER root under the smaller
// with one fetch_min, and if the larger one had meanwhile stopped being a root (the fetch_min returned another parent
// `old` < a) go on uniting `old` with b -- which also repairs the link a -> old where the fetch_min replaced it.  Each
// round that does not return replaces a by a strictly smaller pixel, so unite ends after at most `bound` rounds.  When
// every unite of every edge has returned, all pixels of a component share one root, and that root is the component's
// SMALLEST index: its first pixel in raster order, which is the label the rule asks for.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MF_HD __host__ __device__ __forceinline__
#else
#define MF_HD inline
#endif

namespace maskfit {

constexpr int TW = 64, TH = 16, TILE = TW * TH;      // the tile of masks.hip and overlay.hip
constexpr int MAX_C = 128, MAX_DIM = 16384, NSUMS = 8;
constexpr int BORDER_JOBS = TW + 2 * (TH - 1);        // per tile: top row, left column, right column (rows 1 .. TH-1)

// The adjacency predicate on two 8-neighbours' values.
MF_HD bool joined(int v, int w, int tol) {
  if (v == 0 || w == 0) return false;
  const int d = v - w;
  return (d < 0 ? -d : d) <= tol;
}

// P: int load(int i), int fetch_min(int i, int v) (returns the value before).  bound: pixels in the store.
template <class P>
MF_HD int find_root(P& p, int i, int bound) {
  for (int step = 0; step < bound; ++step) {          // (1): a strictly decreasing path, at most `bound` pixels long
    const int q = p.load(i);
    if (q == i) return i;
    i = q;
  }
  return i;
}

template <class P>
MF_HD void unite(P& p, int a, int b, int bound) {
  for (int round = 0; round < bound; ++round) {       // a strictly decreases from round to round: at most `bound` rounds
    a = find_root(p, a, bound);
    b = find_root(p, b, bound);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = p.fetch_min(a, b);
    if (old == a) return;                             // a was still a root: now it hangs under b
    a = old;                                          // a had a parent old < a by then: unite that one with b
  }
}

// Phase 1, one pixel of a tile: unite it with its W, NW, N, NE neighbours inside the tile.  val: the tile's values
// uint8 [TH][TW], 0 outside the frame; par: the tile's store over local indices ly * TW + lx.
template <class P>
MF_HD void tile_link_pixel(const unsigned char* val, P& par, int lx, int ly, int tol) {
  const int i = ly * TW + lx, v = val[i];
  if (v == 0) return;
  if (lx > 0 && joined(v, val[i - 1], tol)) unite(par, i, i - 1, TILE);
  if (ly > 0) {
    if (lx > 0 && joined(v, val[i - TW - 1], tol)) unite(par, i, i - TW - 1, TILE);
    if (joined(v, val[i - TW], tol)) unite(par, i, i - TW, TILE);
    if (lx < TW - 1 && joined(v, val[i - TW + 1], tol)) unite(par, i, i - TW + 1, TILE);
  }
}

// Frame-linear index of a tile-local one.
MF_HD int tile_to_frame(int local, int x0, int y0, int W) { return (y0 + local / TW) * W + x0 + local % TW; }

// Phase 2, job t (0 .. BORDER_JOBS-1) of tile (tx, ty): the pairs (pixel, earlier 8-neighbour IN ANOTHER TILE).  Every
// such pair of a frame belongs to exactly one job: the earlier neighbour q of p is W, NW, N or NE of p; N / NW / NE lie
// in another tile iff p is in its tile's top row (jobs 0 .. TW-1, which also take W for lx == 0), or, below the top row,
// NW iff lx == 0 and NE iff lx == TW-1; W iff lx == 0.  mask: the frame uint8 [H][W]; par: the frame's store over
// y * W + x.  No pixel outside the frame is read.
template <class P>
MF_HD void border_link(const unsigned char* mask, P& par, int H, int W, int tx, int ty, int t, int tol) {
  int lx, ly;
  bool w = false, nw = false, n = false, ne = false;
  if (t < TW) { lx = t; ly = 0; w = lx == 0; nw = n = ne = true; }
  else if (t < TW + TH - 1) { lx = 0; ly = t - TW + 1; w = nw = true; }
  else { lx = TW - 1; ly = t - (TW + TH - 1) + 1; ne = true; }
  const int x = tx * TW + lx, y = ty * TH + ly;
  if (x >= W || y >= H) return;
  const int i = y * W + x, v = mask[i], bound = H * W;
  if (v == 0) return;
  if (w && x > 0 && joined(v, mask[i - 1], tol)) unite(par, i, i - 1, bound);
  if (y > 0) {
    if (nw && x > 0 && joined(v, mask[i - W - 1], tol)) unite(par, i, i - W - 1, bound);
    if (n && joined(v, mask[i - W], tol)) unite(par, i, i - W, bound);
    if (ne && x + 1 < W && joined(v, mask[i - W + 1], tol)) unite(par, i, i - W + 1, bound);
  }
}

// The slot of a component: the position of `first` in firsts[0 .. m-1] (ascending), or -1.  At most 8 rounds for m <= 128.
MF_HD int find_slot(const int* firsts, int m, int first) {
  int lo = 0, hi = m;
  while (lo < hi) {                                   // the interval halves: at most log2(m) + 1 rounds
    const int mid = (lo + hi) >> 1;
    if (firsts[mid] < first) lo = mid + 1; else hi = mid;
  }
  return (lo < m && firsts[lo] == first) ? lo : -1;
}

}  // namespace maskfit
