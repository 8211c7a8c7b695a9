// Ring-count segmentation masks painted from label rows, and the pixel-level comparison of two such masks.  The rule is
// stated beside the prototypes in spnet_hip.h ("Ring-count masks"); spnet_amd/masks.py is the host side and holds the same
// rule in numpy (ring_masks_host), tests/helpers/mask_ref.py restates it in Python integers: all three agree bit for bit.
//
// ring_masks_kernel: one workgroup per 64 x 16 tile of one frame (the overlay kernel's tiling; a lane owns 4 pixels of one
// row).  Lanes 0 .. K-1 quantise the frame's rows into LDS -- the seven integers of the rule and a pixel box -- and the
// rows whose box meets the tile go into an LDS list that keeps their order (ballot + prefix count, no atomics).  Every lane
// then walks the list in order: the last row that contains a pixel wins.
//
// THE BOX IS A SUPERSET OF THE ELLIPSE.  Inside means (u bq)^2 + (v aq)^2 <= (aq bq 2^14)^2, hence
// u^2 + v^2 <= 2^28 m^2 with m = max(aq, bq).  (u, v) is (dx, dy) turned by the integer pair (c, s), so
// u^2 + v^2 = (c^2 + s^2)(dx^2 + dy^2), and with c, s within 0.5 (+ one part in 2^52) of 2^14 cos, 2^14 sin:
// c^2 + s^2 >= 2^28 - 2^14 (|cos| + |sin|) - 1 >= 2^28 (1 - 8.7e-5).  So |dx| <= m (1 + d), d < 4.4e-5, in 1/16 pixel.
// m <= 16 A + 0.5 (A = max(a, b)) and cxq / 16 is within 1/32 of cx, so the pixel's centre x + 0.5 lies within
// A + 1/16 + d (A + 1/32) pixels of cx: less than A + 1 while A <= 16,384, less than A + 1.51 up to the limit of 32,768.
// With R = ceil(A) + 1 (+ 1 more beyond 16,384) every x with |x + 0.5 - cx| <= R - 0 satisfies
// floor(cx) - R <= x <= floor(cx) + R, which is the box; y likewise.  A row dropped for a tile, or skipped by a lane, can
// therefore not have painted there.
//
// Ranges: |cxq|, |cyq|, aq, bq < 2^19; |c|, |s| <= 2^14; pixel centres < 2^18, so |dx|, |dy| < 2^20, |u|, |v| < 2^35,
// |u bq|, |v aq| < 2^54 (int64), their squares and the sum < 2^109 and (aq bq 2^14)^2 < 2^104 (unsigned __int128).
//
// mask_compare_kernel: blocks (chunk, frame); integer counts per lane, wave reduction by shuffles, one LDS reduction per
// workgroup, five integer atomics per workgroup on the frame's counts (zeroed by a memset node ahead of the launch):
// integer sums do not depend on their order, so the result does not depend on the grid.
#include "mask_rule.h"        // MaskRow, quantise_row, the 128-bit inside test and the ordered cull: shared with tracks.hip

namespace {

__global__ __launch_bounds__(MK_THREADS) void ring_masks_kernel(const double* __restrict__ rows, const int* __restrict__ count,
                                                                int b_base, int K, int H, int W,
                                                                unsigned char* __restrict__ out, int vec16) {
  __shared__ MaskRow s_row[MK_MAX_K];
  __shared__ int s_list[MK_MAX_K];
  __shared__ int s_wave[MK_THREADS / SPNET_WAVE];
  __shared__ __attribute__((aligned(16))) unsigned s_tile[MK_TH][MK_TW / 4];

  const long n = (long)b_base + blockIdx.z;
  const int x0 = blockIdx.x * MK_TW, y0 = blockIdx.y * MK_TH;
  const int x1 = min(x0 + MK_TW, W), y1 = min(y0 + MK_TH, H);
  const int tid = threadIdx.x;
  const int px = x0 + (tid & 15) * 4, py = y0 + (tid >> 4);
  const int cnt = min(max(count[n], 0), K);

  // ---- quantise and cull, keeping the rows' order
  const int total = mask_cull_rows(rows + n * K * 6, cnt, x0, y0, x1, y1, s_row, s_list, s_wave);

  // ---- paint: every lane walks the list in order over its 4 pixels
  unsigned pix = 0;                                                     // pixel px + i in byte i
  for (int i = 0; i < total; ++i) {
    const MaskRow& q = s_row[s_list[i]];
    const unsigned in = mask_inside4(q, px, py);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (in >> j & 1u) pix = (pix & ~(255u << (8 * j))) | (unsigned)q.value << (8 * j);
  }

  // ---- store
  unsigned char* frame = out + n * H * W;
  if (vec16) {                                                          // W % 16 == 0: the tile is whole 16-byte pieces
    s_tile[tid >> 4][tid & 15] = pix;
    __syncthreads();
    const int tw = x1 - x0, th = y1 - y0, ipr = tw / 16;
    if (tid < th * ipr) {
      const int r = tid / ipr, j = tid - r * ipr;
      *reinterpret_cast<uint4*>(frame + (long)(y0 + r) * W + x0 + 16 * j) = *reinterpret_cast<const uint4*>(&s_tile[r][4 * j]);
    }
  } else if (py < y1) {
    unsigned char* o = frame + (long)py * W + px;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (px + j < x1) o[j] = (unsigned char)(pix >> (8 * j));
  }
}

constexpr int MC_THREADS = 256, MC_MAX_BLOCKS = 64, MC_BYTES_PER_BLOCK = MC_THREADS * 16 * 4;

__device__ __forceinline__ void mc_classify(unsigned p, unsigned t, int tol, int* k) {
  if (p == 0u && t == 0u) {
    ++k[0];
  } else if (p != 0u && t != 0u) {
    const int d = (int)p - (int)t;
    if ((d < 0 ? -d : d) <= tol) ++k[1]; else ++k[2];
  } else if (p != 0u) {
    ++k[3];
  } else {
    ++k[4];
  }
}

__global__ __launch_bounds__(MC_THREADS) void mask_compare_kernel(const unsigned char* __restrict__ pred,
                                                                  const unsigned char* __restrict__ truth, int n_base,
                                                                  long n_pixels, int tol, int* __restrict__ counts) {
  __shared__ int s_part[MC_THREADS / SPNET_WAVE][5];
  const long n = (long)n_base + blockIdx.y;
  const unsigned char* p = pred + n * n_pixels;
  const unsigned char* t = truth + n * n_pixels;
  const int tid = threadIdx.x, lane = tid & (SPNET_WAVE - 1), wave = tid / SPNET_WAVE;
  const long gtid = (long)blockIdx.x * MC_THREADS + tid, gsize = (long)gridDim.x * MC_THREADS;
  int k[5] = {0, 0, 0, 0, 0};

  const bool vec = (((uintptr_t)p | (uintptr_t)t) & 15) == 0;            // uniform over the frame
  const long n16 = vec ? n_pixels / 16 : 0;
  for (long i = gtid; i < n16; i += gsize) {
    const uint4 a = reinterpret_cast<const uint4*>(p)[i], b = reinterpret_cast<const uint4*>(t)[i];
    const unsigned aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int j = 0; j < 4; ++j) mc_classify((aw[w] >> (8 * j)) & 255u, (bw[w] >> (8 * j)) & 255u, tol, k);
  }
  for (long i = n16 * 16 + gtid; i < n_pixels; i += gsize) mc_classify(p[i], t[i], tol, k);

#pragma unroll
  for (int c = 0; c < 5; ++c) {
    int v = k[c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) s_part[wave][c] = v;
  }
  __syncthreads();
  if (tid < 5) {
    int v = 0;
#pragma unroll
    for (int w = 0; w < MC_THREADS / SPNET_WAVE; ++w) v += s_part[w][tid];
    if (v) atomicAdd(counts + n * 5 + tid, v);
  }
}

}  // namespace

extern "C" int spnet_ring_masks(const double* rows, const int* count, int B, int K, int H, int W, unsigned char* out,
                                void* stream) {
  if (!mk_rows_ok(rows, count) || !out || B < 0 || K < 1 || K > MK_MAX_K || !mk_dims_ok(H, W)) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  const int vec16 = (W % 16 == 0) && !((uintptr_t)out & 15);
  spnet_for_grid_chunks(B, [&](int b0, int n) {
    const dim3 grid(spnet_cdiv(W, MK_TW), spnet_cdiv(H, MK_TH), n);
    hipLaunchKernelGGL(ring_masks_kernel, grid, dim3(MK_THREADS), 0, (hipStream_t)stream, rows, count, b0, K, H, W, out, vec16);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_mask_compare(const unsigned char* pred, const unsigned char* truth, int N, long n_pixels, int tol,
                                  int* counts, void* stream) {
  if (!pred || !truth || !mk_int_ok(counts) || N < 0 || n_pixels < 1 || n_pixels > 0x7fffffffL || tol < 0 || tol > 255)
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)N * 5 * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const long want = (n_pixels + MC_BYTES_PER_BLOCK - 1) / MC_BYTES_PER_BLOCK;
  const int blocks = want < MC_MAX_BLOCKS ? (int)want : MC_MAX_BLOCKS;
  spnet_for_grid_chunks(N, [&](int n0, int n) {
    hipLaunchKernelGGL(mask_compare_kernel, dim3(blocks, n), dim3(MC_THREADS), 0, (hipStream_t)stream, pred, truth, n0, n_pixels,
                       tol, counts);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}
