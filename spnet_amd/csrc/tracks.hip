// Antinode tracking: which ellipse of frame t + d is the same antinode as one of frame t.  The rule is stated beside the
// prototypes in spnet_hip.h ("Antinode tracks"); spnet_amd/tracks.py is the host side and holds the same rule in numpy
// (link_tracks_host), tests/helpers/tracks_ref.py restates it in Python integers and sets.  The pixel sets are the mask
// rule's: quantise_row and the 128-bit inside test come from mask_rule.h, the header masks.hip paints with.
//
// track_area_kernel: one workgroup per (frame, 64 x 16 tile).  The frame's rows are culled against the tile into an ordered
// LDS list; a lane counts its 4 pixels inside every listed row into an LDS counter per row, and the nonzero counters are
// added to area[t][k] with one global atomic each.  area is zeroed by a memset node ahead of the launch.
//
// track_overlap_kernel (the hot path): one workgroup per (frame pair, 64 x 16 tile).  The tile body and its LDS pair table
// are track_tile.h's, which csrc/track_score.hip compiles too: both frames' rows culled into two ordered LDS lists, a
// 128-bit set of list-B positions per pixel, uint16 LDS counters, and the nonzero counts added to inter[pair][i][j] by
// global integer atomics.  Integer sums do not depend on their order: the result does not depend on the grid or on the
// order of arrival.
//
// track_link_kernel: one workgroup per frame pair, threads 0 .. K-1 for the detections of frame t, 128 .. 128+K-1 for those
// of frame t + d (track_tile.h's track_mutual_best: every lane chooses its best, a barrier, then the mutual test).  The
// workgroup of pair (t, t + d) is the only writer of next[t] and prev[t + d] in its launch and reads nothing that another
// pair writes.
//
// track_rank_*: pointer jumping over prev (tracks_core.h) between two ping-pong halves of ws, one launch per round: a round
// reads one half and writes the other, so no lane reads what another lane of the same launch writes.
//
// Bounds: count is clamped to 0 .. K; list positions are < K <= 128; pixels beyond W or H are masked out of every count;
// next and prev are only compared with -1 by the link step; prev is range-checked by rank_init before it is an address.
#include "track_tile.h"

namespace {

__global__ __launch_bounds__(TR_THREADS) void track_area_kernel(const double* __restrict__ rows, const int* __restrict__ count,
                                                                int n_base, int K, int H, int W, int tiles_x,
                                                                int* __restrict__ area) {
  __shared__ MaskRow s_row[MK_MAX_K];
  __shared__ int s_list[MK_MAX_K];
  __shared__ int s_cnt[MK_MAX_K];
  __shared__ int s_wave[TR_THREADS / SPNET_WAVE];

  const long n = (long)n_base + blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  const int x0 = tx * MK_TW, y0 = ty * MK_TH;
  const int x1 = min(x0 + MK_TW, W), y1 = min(y0 + MK_TH, H);
  const int tid = threadIdx.x;
  const int px = x0 + (tid & 15) * 4, py = y0 + (tid >> 4);
  const int cnt = min(max(count[n], 0), K);

  if (tid < MK_MAX_K) s_cnt[tid] = 0;
  const int total = mask_cull_rows(rows + n * K * 6, cnt, x0, y0, x1, y1, s_row, s_list, s_wave);   // holds the barriers
  if (total == 0) return;
  const unsigned ok = valid4(px, py, x1, y1);
  for (int i = 0; i < total; ++i) {
    const int c = __popc(mask_inside4(s_row[s_list[i]], px, py) & ok);
    if (c) atomicAdd(&s_cnt[i], c);
  }
  __syncthreads();
  if (tid < total) {
    const int c = s_cnt[tid];
    if (c) atomicAdd(area + n * K + s_list[tid], c);
  }
}

__global__ __launch_bounds__(TR_THREADS) void track_overlap_kernel(const double* __restrict__ rows, const int* __restrict__ count,
                                                                   int K, int H, int W, int tiles_x, long t0, int pair_base,
                                                                   int d, int* __restrict__ inter) {
  __shared__ TrackTileLds s;
  const long pair = (long)pair_base + blockIdx.y;
  const long ta = t0 + pair, tb = ta + d;
  track_tile_overlap(rows + ta * K * 6, min(max(count[ta], 0), K), rows + tb * K * 6, count + tb, K, H, W, tiles_x, (int)blockIdx.x, s,
                     inter + pair * K * K, K);
}

__global__ __launch_bounds__(TR_THREADS) void track_link_kernel(const int* __restrict__ inter, const int* __restrict__ area,
                                                                const double* __restrict__ rows, const int* __restrict__ count,
                                                                int K, long t0, int pair_base, int d, int iou_q,
                                                                int* __restrict__ next, int* __restrict__ prev) {
  __shared__ int s_area[2][MK_MAX_K];
  __shared__ unsigned char s_open[2][MK_MAX_K];
  __shared__ int s_best[2][MK_MAX_K];

  const long pair = (long)pair_base + blockIdx.x;
  const long ta = t0 + pair, tb = ta + d;
  const int tid = threadIdx.x, side = tid / MK_MAX_K, k = tid % MK_MAX_K;   // side 0: frame t, 1: frame t + d
  const long t = side ? tb : ta;
  if (k < K) {
    const int link = side ? prev[t * K + k] : next[t * K + k];
    s_open[side][k] = (row_live(rows, count, t, K, k) && link == -1) ? 1 : 0;
    s_area[side][k] = area[t * K + k];
  }
  __syncthreads();
  const int j = track_mutual_best(inter + pair * K * K, K, K, s_area, s_open, s_best, iou_q);
  if (j >= 0) {                                             // lanes of frame t only
    next[ta * K + k] = (int)(tb * K + j);
    prev[tb * K + j] = (int)(ta * K + k);
  }
}

__global__ __launch_bounds__(TR_THREADS) void track_rank_init_kernel(const int* __restrict__ prev, int K, long total,
                                                                     int* __restrict__ anc, int* __restrict__ dist) {
  for (long x = (long)blockIdx.x * TR_THREADS + threadIdx.x; x < total; x += (long)gridDim.x * TR_THREADS) {
    const int a = tracks::rank_init(prev, (int)x, K);
    anc[x] = a;
    dist[x] = a == (int)x ? 0 : 1;
  }
}

__global__ __launch_bounds__(TR_THREADS) void track_rank_jump_kernel(const int* __restrict__ anc_in, const int* __restrict__ dist_in,
                                                                     int* __restrict__ anc_out, int* __restrict__ dist_out,
                                                                     long total) {
  for (long x = (long)blockIdx.x * TR_THREADS + threadIdx.x; x < total; x += (long)gridDim.x * TR_THREADS)
    tracks::rank_jump(anc_in, dist_in, anc_out, dist_out, (int)x, (int)total);
}

__global__ __launch_bounds__(TR_THREADS) void track_rank_finish_kernel(const int* __restrict__ anc, const int* __restrict__ dist,
                                                                       const double* __restrict__ rows,
                                                                       const int* __restrict__ count, int K, long total,
                                                                       int* __restrict__ track, int* __restrict__ age) {
  for (long x = (long)blockIdx.x * TR_THREADS + threadIdx.x; x < total; x += (long)gridDim.x * TR_THREADS) {
    const long t = x / K;
    const int k = (int)(x - t * K);
    const bool live = row_live(rows, count, t, K, k);
    const int a = anc[x];
    track[x] = live ? 1 + ((a >= 0 && a < total) ? a : (int)x) : 0;
    age[x] = live ? dist[x] : 0;
  }
}

bool frames_ok(const double* rows, const int* count, long N, int K) { return mk_rows_ok(rows, count) && tracks::sizes_ok(N, K); }
// pairs (t, t + d), t = t0 .. t0 + n_pairs - 1, all inside 0 .. N-1
bool range_ok(long N, long t0, long n_pairs, int d) {
  return d >= 1 && d <= tracks::MAX_GAP && t0 >= 0 && n_pairs >= 0 && t0 + n_pairs + d <= N;
}

}  // namespace

extern "C" int spnet_track_area(const double* rows, const int* count, int N, int K, int H, int W, int* area, void* stream) {
  if (!frames_ok(rows, count, N, K) || !mk_dims_ok(H, W) || !mk_int_ok(area)) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipError_t e = hipMemsetAsync(area, 0, (size_t)N * K * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const int tiles_x = spnet_cdiv(W, MK_TW), tiles = tiles_x * spnet_cdiv(H, MK_TH);
  spnet_for_grid_chunks(N, [&](int n0, int n) {
    hipLaunchKernelGGL(track_area_kernel, dim3(tiles, n), dim3(TR_THREADS), 0, (hipStream_t)stream, rows, count, n0, K, H, W,
                       tiles_x, area);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_track_overlap(const double* rows, const int* count, int N, int K, int H, int W, int t0, int n_pairs,
                                   int d, int* inter, void* stream) {
  if (!frames_ok(rows, count, N, K) || !mk_dims_ok(H, W) || !range_ok(N, t0, n_pairs, d) || !mk_int_ok(inter))
    return (int)hipErrorInvalidValue;
  if (n_pairs == 0) return 0;
  hipError_t e = hipMemsetAsync(inter, 0, (size_t)n_pairs * K * K * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const int tiles_x = spnet_cdiv(W, MK_TW), tiles = tiles_x * spnet_cdiv(H, MK_TH);
  spnet_for_grid_chunks(n_pairs, [&](int p0, int n) {
    hipLaunchKernelGGL(track_overlap_kernel, dim3(tiles, n), dim3(TR_THREADS), 0, (hipStream_t)stream, rows, count, K, H, W,
                       tiles_x, (long)t0, p0, d, inter);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_track_link(const int* inter, const int* area, const double* rows, const int* count, int N, int K, int t0,
                                int n_pairs, int d, int iou_q, int* next, int* prev, void* stream) {
  if (!frames_ok(rows, count, N, K) || !range_ok(N, t0, n_pairs, d) || !mk_int_ok(inter) || !mk_int_ok(area) ||
      !mk_int_ok(next) || !mk_int_ok(prev) || iou_q < 1 || iou_q > tracks::IOU_ONE)
    return (int)hipErrorInvalidValue;
  if (n_pairs == 0) return 0;
  spnet_for_grid_chunks(n_pairs, [&](int p0, int n) {
    hipLaunchKernelGGL(track_link_kernel, dim3(n), dim3(TR_THREADS), 0, (hipStream_t)stream, inter, area, rows, count, K,
                       (long)t0, p0, d, iou_q, next, prev);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" long spnet_track_rank_ws(int N, int K) {
  if (!tracks::sizes_ok(N, K)) return -1;
  const long total = (long)N * K;
  return 4 * sizeof(int) * (total > 0 ? total : 1);       // two halves of (anc, dist)
}

extern "C" int spnet_track_rank(const int* prev, const double* rows, const int* count, int N, int K, int* track, int* age,
                                void* ws, void* stream) {
  if (!frames_ok(rows, count, N, K) || !mk_int_ok(prev) || !mk_int_ok(track) || !mk_int_ok(age) || !mk_int_ok(ws))
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  const long total = (long)N * K;
  int* half[2][2] = {{(int*)ws, (int*)ws + total}, {(int*)ws + 2 * total, (int*)ws + 3 * total}};
  const int grid = spnet_ew_grid(total, TR_THREADS);
  hipLaunchKernelGGL(track_rank_init_kernel, dim3(grid), dim3(TR_THREADS), 0, (hipStream_t)stream, prev, K, total, half[0][0],
                     half[0][1]);
  const int rounds = tracks::rank_rounds(N);               // a function of N alone
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(track_rank_jump_kernel, dim3(grid), dim3(TR_THREADS), 0, (hipStream_t)stream, half[r & 1][0],
                       half[r & 1][1], half[(r + 1) & 1][0], half[(r + 1) & 1][1], total);
  hipLaunchKernelGGL(track_rank_finish_kernel, dim3(grid), dim3(TR_THREADS), 0, (hipStream_t)stream, half[rounds & 1][0],
                     half[rounds & 1][1], rows, count, K, total, track, age);
  SPNET_RETURN_LAUNCH_STATUS();
}
