// The ring-count mask rule's device pieces, shared by its two consumers: csrc/masks.hip (the painter) and csrc/tracks.hip
// (antinode tracking, which counts the same pixel sets).  The rule is stated beside the prototypes in spnet_hip.h
// ("Ring-count masks"); both files compile THESE functions, so a pixel is inside a row for the tracker iff the painter
// paints it.  The argument that the box holds every inside pixel, and the ranges of the integers, are in masks.hip.
#pragma once
#include "common.h"

constexpr int MK_TW = 64, MK_TH = 16, MK_THREADS = 256, MK_MAX_K = 128;
constexpr int MK_SUB = 16, MK_CENTER = 8, MK_TRIG_BITS = 14;
constexpr double MK_COORD_LIMIT = 32768.0;
constexpr int MK_MAX_DIM = 16384;

struct MaskRow {                          // one quantised row (quantise_row returned true: it is live)
  int cxq, cyq, aq, bq, c, s, value;
  int bx0, by0, bx1, by1;                 // pixel box, inclusive
};
static_assert(sizeof(MaskRow) == 44, "eleven ints a row");

__device__ __forceinline__ bool quantise_row(const double* __restrict__ r, MaskRow& q) {
  const double cx = r[0], cy = r[1], a = r[2], b = r[3], ang = r[4], rings = r[5];
  // (x - x == 0) is false for NaN and +-Inf
  if (!((cx - cx) == 0.0 && (cy - cy) == 0.0 && (a - a) == 0.0 && (b - b) == 0.0 && (ang - ang) == 0.0 &&
        (rings - rings) == 0.0))
    return false;
  if (!(fabs(cx) < MK_COORD_LIMIT && fabs(cy) < MK_COORD_LIMIT && a < MK_COORD_LIMIT && b < MK_COORD_LIMIT)) return false;
  q.cxq = (int)rint(16.0 * cx);
  q.cyq = (int)rint(16.0 * cy);
  const double aqd = rint(16.0 * a), bqd = rint(16.0 * b);
  if (!(aqd > 0.0 && bqd > 0.0)) return false;
  q.aq = (int)aqd;
  q.bq = (int)bqd;
  const double rad = __dmul_rn(-ang, 3.14159265358979323846 / 180.0);
  q.c = (int)rint(__dmul_rn(16384.0, cos(rad)));
  q.s = (int)rint(__dmul_rn(16384.0, sin(rad)));
  q.value = (int)fmin(fmax(trunc(__dmul_rn(10.0, rings)), 0.0), 255.0);
  const double A = fmax(a, b);
  const int R = (int)ceil(A) + 1 + (A > 16384.0 ? 1 : 0);
  const int fx = (int)floor(cx), fy = (int)floor(cy);
  q.bx0 = fx - R; q.bx1 = fx + R;
  q.by0 = fy - R; q.by1 = fy + R;
  return true;
}

// Row k of frame n is live: k is below the frame's count (clamped to 0 .. K) and the row quantises.
__device__ __forceinline__ bool row_live(const double* __restrict__ rows, const int* __restrict__ count, long n, int K, int k) {
  MaskRow q;
  return k < min(max(count[n], 0), K) && quantise_row(rows + (n * K + k) * 6, q);
}

// The argument gates of the family's entry points (host): an int32 array, a rows / count pair, a frame size.
static inline bool mk_int_ok(const void* p) { return p && !((uintptr_t)p & 3); }
static inline bool mk_rows_ok(const double* rows, const int* count) { return rows && !((uintptr_t)rows & 7) && mk_int_ok(count); }
static inline bool mk_dims_ok(int H, int W) { return H >= 1 && W >= 1 && H <= MK_MAX_DIM && W <= MK_MAX_DIM; }

// Does the row's box meet the pixel rectangle [x0, x1) x [y0, y1)?
__device__ __forceinline__ bool mask_box_meets(const MaskRow& q, int x0, int y0, int x1, int y1) {
  return q.bx0 < x1 && q.bx1 >= x0 && q.by0 < y1 && q.by1 >= y0;
}

// The inside test on the 4 pixels (px .. px + 3, py) of one lane: bit j is set iff pixel px + j is inside the row.  The
// 128-bit comparison of the rule; 0 at once where the lane's pixels lie outside the row's box.
__device__ __forceinline__ unsigned mask_inside4(const MaskRow& q, int px, int py) {
  if (py < q.by0 || py > q.by1 || px + 3 < q.bx0 || px > q.bx1) return 0u;
  const long long dy = (long long)py * MK_SUB + MK_CENTER - q.cyq, dx0 = (long long)px * MK_SUB + MK_CENTER - q.cxq;
  const long long c = q.c, s = q.s, aq = q.aq, bq = q.bq;
  const long long rr = (aq * bq) << MK_TRIG_BITS;
  const unsigned __int128 rhs = (unsigned __int128)(unsigned long long)rr * (unsigned long long)rr;
  long long u = dx0 * c + dy * s, v = dy * c - dx0 * s;
  unsigned in = 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long long P = u * bq, Q = v * aq;
    const unsigned long long Pa = (unsigned long long)(P < 0 ? -P : P), Qa = (unsigned long long)(Q < 0 ? -Q : Q);
    const unsigned __int128 lhs = (unsigned __int128)Pa * Pa + (unsigned __int128)Qa * Qa;
    if (lhs <= rhs) in |= 1u << j;
    u += MK_SUB * c;
    v -= MK_SUB * s;
  }
  return in;
}

// Quantise the first `cnt` rows of a frame (threads 0 .. cnt-1 of the workgroup, one row each) and list those whose box
// meets the tile, IN ROW ORDER (ballot + prefix count over the waves: no atomics).  Every thread of the workgroup calls it
// (it holds two barriers); s_wave has one int per wave.  Returns the list's length.  The rows of the list are in s_row at
// their own index.
__device__ __forceinline__ int mask_cull_rows(const double* __restrict__ frame_rows, int cnt, int x0, int y0, int x1, int y1,
                                              MaskRow* s_row, int* s_list, int* s_wave) {
  const int tid = threadIdx.x, lane = tid & (SPNET_WAVE - 1), wave = tid / SPNET_WAVE;
  const int k = tid;
  bool hit = false;
  if (k < cnt) {
    MaskRow q;
    if (quantise_row(frame_rows + (long)k * 6, q)) {
      hit = mask_box_meets(q, x0, y0, x1, y1);
      if (hit) s_row[k] = q;
    }
  }
  const unsigned long long ball = __ballot(hit);
  if (lane == 0) s_wave[wave] = __popcll(ball);
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < MK_THREADS / SPNET_WAVE; ++w) {
    const int c = s_wave[w];
    before += (w < wave) ? c : 0;
    total += c;
  }
  if (hit) s_list[before + __popcll(ball & ((1ull << lane) - 1ull))] = k;
  __syncthreads();
  return total;
}
