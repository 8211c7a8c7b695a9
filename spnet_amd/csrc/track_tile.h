// One (frame A, frame B, 64 x 16 tile) of the pixel-set intersection counts, shared by its two consumers: csrc/tracks.hip
// (track_overlap_kernel: A and B are two frames of ONE movie) and csrc/track_score.hip (track_match_overlap_kernel: A is a
// frame of the truth, B the same frame of the prediction, with widths of their own).  Both compile THIS body, so a pixel is
// counted for the score iff the linker counts it.
//
// BOTH frames' rows are culled against the tile into two ordered LDS lists; a tile that either list leaves empty ends
// there.  A lane first collects, per pixel, a 128-bit set of the positions in list B whose rows contain the pixel, then
// walks list A: for a pixel inside row A[i] it adds 1 to table[i][j] for every j of the pixel's set.  The table is uint16
// [128][128] in LDS (a tile has 1,024 pixels), two counters to a 32-bit word, so an LDS atomicAdd of 1 or 1 << 16 cannot
// carry from one counter into the next.  The nonzero entries of the first nA x nB corner go to out[i][j] (row stride
// stride_b) by global integer atomics.  Integer sums do not depend on their order: the result does not depend on the grid
// or on the order of arrival.
//
// Bounds: cnt_a (by the caller) and B's count (here) are clamped to 0 .. 128; list positions are < 128; pixels beyond W
// or H are masked out of every count; out is addressed by row indices below the two counts only.
#pragma once
#include "mask_rule.h"
#include "tracks_core.h"

constexpr int TR_THREADS = MK_THREADS;
static_assert(tracks::MAX_K == MK_MAX_K && tracks::MAX_DIM == MK_MAX_DIM && TR_THREADS == 2 * MK_MAX_K, "one set of limits");

struct TrackTileLds {
  MaskRow row[2][MK_MAX_K];
  int list[2][MK_MAX_K];
  int wave[TR_THREADS / SPNET_WAVE];
  unsigned table[MK_MAX_K][MK_MAX_K / 2];                               // uint16 counters [i][j], j and j + 1 share a word
};

// Bits of the lane's 4 pixels that lie inside the frame.
__device__ __forceinline__ unsigned valid4(int px, int py, int x1, int y1) {
  if (py >= y1) return 0u;
  const int n = x1 - px;
  return n >= 4 ? 15u : n <= 0 ? 0u : (1u << n) - 1u;
}

// Every thread of the workgroup calls it (it holds barriers; its early exits are uniform over the workgroup).
// count_b points at frame B's count, which is loaded and clamped to 0 .. k_b only once list A is known not to be empty.
__device__ __forceinline__ void track_tile_overlap(const double* __restrict__ frame_a, int cnt_a, const double* __restrict__ frame_b,
                                                   const int* __restrict__ count_b, int k_b, int H, int W, int tiles_x, int tile,
                                                   TrackTileLds& s, int* __restrict__ out, int stride_b) {
  const int tx = tile % tiles_x, ty = tile / tiles_x;
  const int x0 = tx * MK_TW, y0 = ty * MK_TH;
  const int x1 = min(x0 + MK_TW, W), y1 = min(y0 + MK_TH, H);
  const int tid = threadIdx.x;
  const int px = x0 + (tid & 15) * 4, py = y0 + (tid >> 4);

  const int nA = mask_cull_rows(frame_a, cnt_a, x0, y0, x1, y1, s.row[0], s.list[0], s.wave);
  if (nA == 0) return;                                                  // uniform over the workgroup
  const int nB = mask_cull_rows(frame_b, min(max(*count_b, 0), k_b), x0, y0, x1, y1, s.row[1], s.list[1], s.wave);
  if (nB == 0) return;

  for (int w = tid; w < nA * (MK_MAX_K / 2); w += TR_THREADS) (&s.table[0][0])[w] = 0u;
  __syncthreads();

  // ---- per pixel: the set of list-B positions whose rows contain it
  const unsigned ok = valid4(px, py, x1, y1);
  unsigned long long setB[2][4] = {{0ull, 0ull, 0ull, 0ull}, {0ull, 0ull, 0ull, 0ull}};   // [half][pixel]: registers
  unsigned any = 0u;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int jn = min(nB - 64 * h, 64);
    for (int j = 0; j < jn; ++j) {
      const unsigned in = mask_inside4(s.row[1][s.list[1][64 * h + j]], px, py) & ok;
      any |= in;
      const unsigned long long bit = 1ull << j;
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (in >> p & 1u) setB[h][p] |= bit;
    }
  }

  // ---- list A: count the pairs
  if (any) {
    for (int i = 0; i < nA; ++i) {
      const unsigned in = mask_inside4(s.row[0][s.list[0][i]], px, py) & any;
      if (!in) continue;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (!(in >> p & 1u)) continue;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          unsigned long long m = setB[h][p];
          while (m) {
            const int j = 64 * h + __ffsll((long long)m) - 1;
            m &= m - 1ull;
            atomicAdd(&s.table[i][j >> 1], 1u << (16 * (j & 1)));
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- the nonzero counts of the nA x nB corner
  for (int e = tid; e < nA * nB; e += TR_THREADS) {
    const int i = e / nB, j = e - i * nB;
    const unsigned c = (s.table[i][j >> 1] >> (16 * (j & 1))) & 0xffffu;
    if (c) atomicAdd(out + (long)s.list[0][i] * stride_b + s.list[1][j], (int)c);
  }
}

// The mutual best of one [Ka][Kb] table by a workgroup of 2 x 128 threads: thread side * 128 + k is lane k of side A
// (side 0) or B (side 1).  s_area and s_open are filled and behind a barrier; every lane chooses into s_best, a barrier,
// and a side-A lane gets its partner (tracks_core.h), every other thread -1.  Every thread of the workgroup calls it.
__device__ __forceinline__ int track_mutual_best(const int* __restrict__ inter, int Ka, int Kb, const int (*s_area)[MK_MAX_K],
                                                 const unsigned char (*s_open)[MK_MAX_K], int (*s_best)[MK_MAX_K], int iou_q) {
  const int side = threadIdx.x / MK_MAX_K, k = threadIdx.x % MK_MAX_K;
  if (k < (side ? Kb : Ka))
    s_best[side][k] = side ? tracks::mutual_choose_b(inter, Ka, Kb, k, s_area[0], s_area[1], s_open[0], s_open[1], iou_q)
                           : tracks::mutual_choose_a(inter, Kb, k, s_area[0], s_area[1], s_open[0], s_open[1], iou_q);
  __syncthreads();
  return (side == 0 && k < Ka) ? tracks::mutual_partner(s_best[0], s_best[1], Kb, k) : -1;
}
