// The tracking score: predicted tracks against ground-truth identities.  The rule is stated beside the prototypes in
// spnet_hip.h ("Tracking score"); spnet_amd/tracks.py holds the same rule in numpy (match_tracks_host, ident_stats_host),
// tests/helpers/track_score_ref.py restates it in Python integers, sets and fractions.
//
// spnet_track_match, four steps on one stream, no readback between them:
//   areas      spnet_track_area (csrc/tracks.hip) on the truth and on the predicted rows, into ws
//   overlap    track_match_overlap_kernel: one workgroup per (frame, 64 x 16 tile), the tile body of track_tile.h with
//              A = the frame's truth rows, B = its predicted rows; inter int32 [N][Kt][Kp] in ws, zeroed by a memset node.
//              Every row the TRACK rule calls live is counted; identities and tracks take no part yet
//   match      track_match_kernel: one workgroup per frame, threads 0 .. Kt-1 for the truth rows, 128 .. 128+Kp-1 for the
//              predicted rows (liveness and track_score_core.h's effective identities, a barrier, then track_tile.h's
//              track_mutual_best -- every lane chooses its best, a barrier, the mutual test -- and the three counts)
// spnet_track_ident, the identity statistics: a LANE PER IDENTITY WALKING ITS OWN FRAMES.
//   range      ident_range_kernel: one workgroup per frame writes the effective identities eff [N][Kt] into ws and widens
//              first[g] / last[g] (atomicMin on uint32 / atomicMax; order-free) to the frames in which g is present
//   walk       ident_walk_kernel: lane g walks first[g] .. last[g] in time order, finds its row among the frame's Kt
//              effective identities and steps the four counters (track_score_core.h); it alone writes ident_stats[g]
//   The statistics are sequential in time per identity (a switch compares with the PREVIOUS matched frame), and an
//   identity lives for a short run of frames, so a walk of that run is short; a scatter table identity x frame would
//   need M * N words, 65,536 * N at the limit.
//
// Bounds: counts are clamped to 0 .. K; an ident is an index only after 1 <= ident <= M; track is only compared; a match
// entry is an index only after 0 <= m < Kp; first / last are clamped into 0 .. N-1 by the walk.
#include "track_tile.h"
#include "track_score_core.h"

namespace {

__global__ __launch_bounds__(TR_THREADS) void track_match_overlap_kernel(const double* __restrict__ rows_t,
                                                                         const int* __restrict__ count_t, int Kt,
                                                                         const double* __restrict__ rows_p,
                                                                         const int* __restrict__ count_p, int Kp, int H, int W,
                                                                         int tiles_x, int n_base, int* __restrict__ inter) {
  __shared__ TrackTileLds s;
  const long n = (long)n_base + blockIdx.y;
  track_tile_overlap(rows_t + n * Kt * 6, min(max(count_t[n], 0), Kt), rows_p + n * Kp * 6, count_p + n, Kp, H, W, tiles_x,
                     (int)blockIdx.x, s, inter + n * Kt * Kp, Kp);
}

__global__ __launch_bounds__(TR_THREADS) void track_match_kernel(const int* __restrict__ inter, const int* __restrict__ area_t,
                                                                 const int* __restrict__ area_p, const double* __restrict__ rows_t,
                                                                 const int* __restrict__ count_t, const int* __restrict__ ident,
                                                                 int Kt, const double* __restrict__ rows_p,
                                                                 const int* __restrict__ count_p, const int* __restrict__ track,
                                                                 int Kp, int n_base, int iou_q, int M, int* __restrict__ match,
                                                                 int* __restrict__ frame_counts) {
  __shared__ int s_area[2][MK_MAX_K];
  __shared__ int s_ident[MK_MAX_K];
  __shared__ unsigned char s_live[MK_MAX_K];
  __shared__ unsigned char s_open[2][MK_MAX_K];
  __shared__ int s_best[2][MK_MAX_K];
  __shared__ int s_n[3];                                                // open truth rows, open predicted rows, matches

  const long n = (long)n_base + blockIdx.x;
  const int tid = threadIdx.x, side = tid / MK_MAX_K, k = tid % MK_MAX_K;   // side 0: truth, 1: prediction
  const int K = side ? Kp : Kt;
  if (tid < 3) s_n[tid] = 0;
  if (k < K) {
    if (side) {
      s_open[1][k] = (row_live(rows_p, count_p, n, Kp, k) && track[n * Kp + k] > 0) ? 1 : 0;
      s_area[1][k] = area_p[n * Kp + k];
    } else {
      s_live[k] = row_live(rows_t, count_t, n, Kt, k) ? 1 : 0;
      s_ident[k] = ident[n * Kt + k];
      s_area[0][k] = area_t[n * Kt + k];
    }
  }
  __syncthreads();
  if (side == 0 && k < Kt) s_open[0][k] = track_score::effective_ident(s_ident, s_live, k, M) ? 1 : 0;
  __syncthreads();
  const int j = track_mutual_best(inter + n * Kt * Kp, Kt, Kp, s_area, s_open, s_best, iou_q);
  if (k < K) {
    if (s_open[side][k]) atomicAdd(&s_n[side], 1);
    if (side == 0) {
      match[n * Kt + k] = j;
      if (j >= 0) atomicAdd(&s_n[2], 1);
    }
  }
  __syncthreads();
  if (tid < 3) frame_counts[n * 3 + tid] = tid == 0 ? s_n[2] : s_n[tid - 1] - s_n[2];     // tp, fn, fp
}

__global__ __launch_bounds__(MK_MAX_K) void ident_range_kernel(const double* __restrict__ rows_t, const int* __restrict__ count_t,
                                                               const int* __restrict__ ident, int Kt, int M, int n_base,
                                                               int* __restrict__ eff, int* __restrict__ first,
                                                               int* __restrict__ last) {
  __shared__ int s_ident[MK_MAX_K];
  __shared__ unsigned char s_live[MK_MAX_K];
  const long n = (long)n_base + blockIdx.x;
  const int k = threadIdx.x;
  if (k < Kt) {
    s_live[k] = row_live(rows_t, count_t, n, Kt, k) ? 1 : 0;
    s_ident[k] = ident[n * Kt + k];
  }
  __syncthreads();
  if (k < Kt) {
    const int g = track_score::effective_ident(s_ident, s_live, k, M);      // 0 .. M
    eff[n * Kt + k] = g;
    if (g) {
      atomicMin((unsigned*)first + g, (unsigned)n);
      atomicMax(last + g, (int)n);
    }
  }
}

__global__ __launch_bounds__(TR_THREADS) void ident_walk_kernel(const int* __restrict__ eff, const int* __restrict__ match,
                                                                const int* __restrict__ track, long N, int Kt, int Kp, int M,
                                                                const int* __restrict__ first, const int* __restrict__ last,
                                                                int* __restrict__ ident_stats) {
  const int g = blockIdx.x * TR_THREADS + threadIdx.x;
  if (g > M) return;
  int* out = ident_stats + (long)g * track_score::STATS;
  if (g == 0) {
#pragma unroll
    for (int c = 0; c < track_score::STATS; ++c) out[c] = 0;
    return;
  }
  track_score::ident_walk(eff, match, track, N, Kt, Kp, g, (long)(unsigned)first[g], last[g], out);
}

}  // namespace

extern "C" long spnet_track_match_ws(int N, int Kt, int Kp) {
  if (!track_score::sizes_ok(N, Kt, Kp)) return -1;
  const long n = (long)N * Kt * Kp + (long)N * Kt + (long)N * Kp;
  return sizeof(int) * (n > 0 ? n : 1);
}

extern "C" int spnet_track_match(const double* rows_t, const int* count_t, const int* ident, int Kt, const double* rows_p,
                                 const int* count_p, const int* track, int Kp, int N, int H, int W, int iou_q, int M, void* ws,
                                 int* match, int* frame_counts, void* stream) {
  if (!mk_rows_ok(rows_t, count_t) || !mk_rows_ok(rows_p, count_p) || !track_score::sizes_ok(N, Kt, Kp) || !mk_dims_ok(H, W) ||
      !track_score::idents_ok(M) || iou_q < 1 || iou_q > tracks::IOU_ONE || !mk_int_ok(ident) || !mk_int_ok(track) ||
      !mk_int_ok(ws) || !mk_int_ok(match) || !mk_int_ok(frame_counts))
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  int* inter = (int*)ws;
  int* area_t = inter + (long)N * Kt * Kp;
  int* area_p = area_t + (long)N * Kt;
  int e = spnet_track_area(rows_t, count_t, N, Kt, H, W, area_t, stream);
  if (e) return e;
  e = spnet_track_area(rows_p, count_p, N, Kp, H, W, area_p, stream);
  if (e) return e;
  hipError_t he = hipMemsetAsync(inter, 0, (size_t)N * Kt * Kp * sizeof(int), (hipStream_t)stream);
  if (he != hipSuccess) return (int)he;
  const int tiles_x = spnet_cdiv(W, MK_TW), tiles = tiles_x * spnet_cdiv(H, MK_TH);
  spnet_for_grid_chunks(N, [&](int n0, int n) {
    hipLaunchKernelGGL(track_match_overlap_kernel, dim3(tiles, n), dim3(TR_THREADS), 0, (hipStream_t)stream, rows_t, count_t, Kt,
                       rows_p, count_p, Kp, H, W, tiles_x, n0, inter);
  });
  spnet_for_grid_chunks(N, [&](int n0, int n) {
    hipLaunchKernelGGL(track_match_kernel, dim3(n), dim3(TR_THREADS), 0, (hipStream_t)stream, inter, area_t, area_p, rows_t,
                       count_t, ident, Kt, rows_p, count_p, track, Kp, n0, iou_q, M, match, frame_counts);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" long spnet_track_ident_ws(int N, int Kt, int M) {
  if (!tracks::sizes_ok(N, Kt) || !track_score::idents_ok(M)) return -1;
  return sizeof(int) * ((long)N * Kt + 2L * (M + 1));
}

extern "C" int spnet_track_ident(const double* rows_t, const int* count_t, const int* ident, const int* match, const int* track,
                                 int N, int Kt, int Kp, int M, void* ws, int* ident_stats, void* stream) {
  if (!mk_rows_ok(rows_t, count_t) || !track_score::sizes_ok(N, Kt, Kp) || !track_score::idents_ok(M) || !mk_int_ok(ident) ||
      !mk_int_ok(match) || !mk_int_ok(track) || !mk_int_ok(ws) || !mk_int_ok(ident_stats))
    return (int)hipErrorInvalidValue;
  int* first = (int*)ws;                                                // [M + 1], then last [M + 1], then eff [N][Kt]
  int* last = first + (M + 1);
  int* eff = last + (M + 1);
  // first as uint32 0xffffffff (above every frame), last -1
  hipError_t he = hipMemsetAsync(first, 0xff, 2 * (size_t)(M + 1) * sizeof(int), (hipStream_t)stream);
  if (he != hipSuccess) return (int)he;
  spnet_for_grid_chunks(N, [&](int n0, int n) {
    hipLaunchKernelGGL(ident_range_kernel, dim3(n), dim3(MK_MAX_K), 0, (hipStream_t)stream, rows_t, count_t, ident, Kt, M, n0, eff,
                       first, last);
  });
  hipLaunchKernelGGL(ident_walk_kernel, dim3(spnet_cdiv(M + 1, TR_THREADS)), dim3(TR_THREADS), 0, (hipStream_t)stream, eff, match,
                     track, (long)N, Kt, Kp, M, first, last, ident_stats);
  SPNET_RETURN_LAUNCH_STATUS();
}
