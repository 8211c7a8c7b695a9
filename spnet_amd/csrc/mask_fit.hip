// Ellipses from ring-count masks, the device half: connected-component labelling of uint8 masks and eight integer sums per
// component.  The rule is stated beside the prototypes in spnet_hip.h ("Mask fitting"); the union-find and the tile / border
// geometry are in mask_fit_core.h (shared with tools/mask_fit_host_check.cpp); spnet_amd/masks.py is the host side and
// holds the same rule in numpy; tests/helpers/mask_fit_ref.py restates it as a flood fill.  DESIGN.md 5h.
//
// spnet_mask_label: THREE launches, whatever the mask (no readback, no "until unchanged").  The labels array itself is the
// union-find's parent store, in LABEL FORM: labels[p] = 1 + (index of p's parent), 0 for background; a root has
// labels[p] == p + 1.  Every value ever stored for p is 1 + an ancestor of p, so the array is a valid forest after every
// phase and the last phase leaves 1 + root = the rule's label.
//   1. mf_tile_label_kernel   one workgroup per 64 x 16 tile (a lane owns 4 pixels of one row, as in masks.hip): union-find
//                             over the tile's 1,024 pixels in LDS, then every pixel's tile-local root is written in frame
//                             coordinates.  VISIBILITY: LDS only (workgroup barriers); global memory is written with plain
//                             stores and read by nobody in this launch.
//   2. mf_border_merge_kernel one workgroup per tile, one lane per border pixel (94 jobs): unites each pixel with its earlier
//                             8-neighbours that lie in ANOTHER tile.  Here workgroups do read and write each other's words
//                             within one launch.  VISIBILITY: phase 1's stores are visible through the kernel boundary;
//                             inside the launch EVERY access to the parent store is an agent-scope atomic -- relaxed
//                             atomic loads (served past the CU's L1) and atomic min -- so there is no cached copy that
//                             could be stale, on either side.  Nothing is ordered by these atomics and nothing needs to
//                             be: the union-find is correct under every interleaving (mask_fit_core.h), a stale-free read
//                             of ANY value the word has held is an ancestor, and no workgroup waits for another.
//   3. mf_flatten_kernel      one lane per pixel: walk to the root, store 1 + root.  VISIBILITY: phase 2's atomics are
//                             complete at the kernel boundary.  Lanes store while others still walk, in place: a walker
//                             sees a word's old value or its new one, both ancestors of the same root, and roots are never
//                             rewritten with another value.  The accesses are relaxed agent-scope atomic loads / stores so
//                             that this is defined behaviour and no L1 copy is involved; no ordering is needed.
//
// spnet_mask_moments: TWO launches.
//   4. mf_compact_kernel      one workgroup of 1,024 lanes per frame walks the frame's labels in raster order, 4,096 a round
//                             (16-byte loads where the frame is aligned; the next round's load is issued before this round's
//                             scan), counts the roots (labels[p] == p + 1) with a wave scan + 16 wave totals in LDS, and
//                             gives the first C of them their slot: sums[b][slot][7] = first.  It zeroes the frame's other
//                             sums first and writes n_components[b] = the true count.  One workgroup per frame keeps the
//                             order without any workspace in HBM and without one workgroup waiting for another; the frames
//                             of a batch run side by side.  VISIBILITY: reads labels written by an earlier launch; writes
//                             words nobody else touches in this launch.
//   5. mf_moments_kernel      one workgroup per tile: the frame's <= 128 `first` values go to LDS, every pixel finds its
//                             component's slot by binary search (ascending by construction), the seven sums are formed per
//                             lane over its 4 pixels, per wave by shuffles where the wave holds one component (the common
//                             case), in LDS per tile (64-bit LDS atomics), and each non-zero LDS total is added to the slot
//                             with ONE 64-bit integer atomic.  Integer sums do not depend on their order, so the result does
//                             not depend on the grid.  VISIBILITY: `first` and n_components come through the kernel
//                             boundary and are not written here; the words that are written here are only ever touched by
//                             agent-scope atomic adds and read by nobody before the launch ends.
// Components beyond the first C of a frame are counted and otherwise ignored (their pixels find no slot).
#include "mask_rule.h"        // the family's argument gates
#include "mask_fit_core.h"

namespace {

using namespace maskfit;

constexpr int MF_THREADS = 256, MF_BORDER_THREADS = 128, MF_COMPACT_THREADS = 1024;
constexpr int MF_COMPACT_WAVES = MF_COMPACT_THREADS / SPNET_WAVE, MF_COMPACT_STEP = 4 * MF_COMPACT_THREADS;
static_assert(BORDER_JOBS <= MF_BORDER_THREADS, "one lane per border job");
static_assert(MAX_DIM == MK_MAX_DIM && MAX_C == MK_MAX_K, "one set of limits");
static_assert(MF_THREADS * 4 == TILE, "a lane owns 4 pixels");

struct LdsStore {                       // phase 1: tile-local indices, the store is the index itself
  int* p;
  __device__ __forceinline__ int load(int i) const {
    return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __device__ __forceinline__ int fetch_min(int i, int v) const {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

struct GlobalStore {                    // phases 2 and 3: one frame's labels, label form (1 + parent)
  int* lab;
  __device__ __forceinline__ int load(int i) const {
    return __hip_atomic_load(lab + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
  }
  __device__ __forceinline__ int fetch_min(int i, int v) const {
    return __hip_atomic_fetch_min(lab + i, v + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
  }
};

__global__ __launch_bounds__(MF_THREADS) void mf_tile_label_kernel(const unsigned char* __restrict__ masks, int b_base, int H,
                                                                  int W, int tol, int* __restrict__ labels) {
  __shared__ unsigned char s_val[TILE];
  __shared__ int s_par[TILE];
  const long n = (long)b_base + blockIdx.z, frame = n * H * W;
  const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int tid = threadIdx.x, lx0 = (tid & 15) * 4, ly = tid >> 4, y = y0 + ly;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + lx0 + j, i = ly * TW + lx0 + j;
    s_val[i] = (x < W && y < H) ? masks[frame + (long)y * W + x] : (unsigned char)0;
    s_par[i] = i;
  }
  __syncthreads();
  LdsStore par{s_par};
  for (int j = 0; j < 4; ++j) tile_link_pixel(s_val, par, lx0 + j, ly, tol);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int x = x0 + lx0 + j, i = ly * TW + lx0 + j;
    if (x < W && y < H)
      labels[frame + (long)y * W + x] = s_val[i] ? 1 + tile_to_frame(find_root(par, i, TILE), x0, y0, W) : 0;
  }
}

__global__ __launch_bounds__(MF_BORDER_THREADS) void mf_border_merge_kernel(const unsigned char* __restrict__ masks, int b_base,
                                                                           int H, int W, int tol, int* labels) {
  const long n = (long)b_base + blockIdx.z, frame = n * H * W;
  if (threadIdx.x >= BORDER_JOBS) return;
  GlobalStore par{labels + frame};
  border_link(masks + frame, par, H, W, blockIdx.x, blockIdx.y, threadIdx.x, tol);
}

__global__ __launch_bounds__(MF_THREADS) void mf_flatten_kernel(int* labels, long total, int HW) {
  const long step = (long)gridDim.x * MF_THREADS;
  for (long p = (long)blockIdx.x * MF_THREADS + threadIdx.x; p < total; p += step) {
    const int L = __hip_atomic_load(labels + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (L == 0) continue;
    const int i = (int)(p % HW);
    GlobalStore par{labels + (p - i)};
    const int root = find_root(par, L - 1, HW);
    if (root + 1 != L) __hip_atomic_store(labels + p, root + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(MF_COMPACT_THREADS) void mf_compact_kernel(const int* __restrict__ labels, int HW, int C,
                                                                       int* __restrict__ n_components,
                                                                       long long* __restrict__ sums) {
  __shared__ int s_wave[2][MF_COMPACT_WAVES];
  const long b = blockIdx.x;
  const int* lab = labels + b * HW;
  long long* out = sums + b * C * NSUMS;
  const int tid = threadIdx.x, lane = tid & (SPNET_WAVE - 1), wave = tid / SPNET_WAVE;
  for (int k = tid; k < C * NSUMS; k += MF_COMPACT_THREADS) out[k] = 0;
  __syncthreads();                                        // the slots are zero before any lane writes a `first`

  const bool vec = ((uintptr_t)lab & 15) == 0;            // uniform over the frame
  auto load4 = [&](int i0) {                              // labels i0 .. i0+3; 0 beyond the frame (0 is never a root's word)
    int4 v = make_int4(0, 0, 0, 0);
    if (i0 < HW) {
      if (vec && i0 + 3 < HW) {
        v = *reinterpret_cast<const int4*>(lab + i0);
      } else {
        v.x = lab[i0];
        if (i0 + 1 < HW) v.y = lab[i0 + 1];
        if (i0 + 2 < HW) v.z = lab[i0 + 2];
        if (i0 + 3 < HW) v.w = lab[i0 + 3];
      }
    }
    return v;
  };

  int running = 0;                                        // roots before this round: the same in every lane
  int4 cur = load4(4 * tid);
  for (int base = 0, it = 0; base < HW; base += MF_COMPACT_STEP, ++it) {      // ceil(HW / 4096) rounds
    const int i0 = base + 4 * tid;
    // (i0 + 4 + 4096 cannot overflow: HW <= 2^28)
    const int4 nxt = base + MF_COMPACT_STEP < HW ? load4(i0 + MF_COMPACT_STEP) : make_int4(0, 0, 0, 0);
    const int l[4] = {cur.x, cur.y, cur.z, cur.w};
    bool root[4];
    int c = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      root[j] = l[j] == i0 + j + 1;                       // beyond the frame l is 0 and i0 + j + 1 > 0
      c += root[j] ? 1 : 0;
    }
    int s = c;                                            // inclusive scan over the wave
#pragma unroll
    for (int off = 1; off < SPNET_WAVE; off <<= 1) {
      const int t = __shfl_up(s, off, SPNET_WAVE);
      if (lane >= off) s += t;
    }
    if (lane == SPNET_WAVE - 1) s_wave[it & 1][wave] = s;
    __syncthreads();                                      // two buffers: round it + 2 rewrites this one behind round it + 1's barrier
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < MF_COMPACT_WAVES; ++w) {
      const int v = s_wave[it & 1][w];
      before += (w < wave) ? v : 0;
      total += v;
    }
    int rank = running + before + s - c;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (root[j]) {
        if (rank < C) out[(long)rank * NSUMS + 7] = i0 + j;
        ++rank;
      }
    running += total;
    cur = nxt;
  }
  if (tid == 0) n_components[b] = running;
}

__device__ __forceinline__ long long mf_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, SPNET_WAVE);
  return v;
}

__global__ __launch_bounds__(MF_THREADS) void mf_moments_kernel(const unsigned char* __restrict__ masks,
                                                               const int* __restrict__ labels, int b_base, int H, int W, int C,
                                                               const int* __restrict__ n_components, long long* sums) {
  __shared__ int s_first[MAX_C];
  __shared__ unsigned long long s_acc[MAX_C * 7];
  const long n = (long)b_base + blockIdx.z, frame = n * H * W;
  const int m = min(max(n_components[n], 0), C);          // uniform over the workgroup
  if (m == 0) return;
  long long* out = sums + n * C * NSUMS;
  const int tid = threadIdx.x;
  for (int k = tid; k < m; k += MF_THREADS) s_first[k] = (int)out[(long)k * NSUMS + 7];     // not written in this launch
  for (int k = tid; k < m * 7; k += MF_THREADS) s_acc[k] = 0ull;
  __syncthreads();

  const int x0 = blockIdx.x * TW + (tid & 15) * 4, y = blockIdx.y * TH + (tid >> 4);
  int cur = -1;                                           // the slot the lane's sums belong to
  long long a[7] = {0, 0, 0, 0, 0, 0, 0};
  if (y < H) {
    for (int j = 0; j < 4; ++j) {
      const int x = x0 + j;
      if (x >= W) break;
      const long p = frame + (long)y * W + x;
      const int L = labels[p];
      const int slot = L > 0 ? find_slot(s_first, m, L - 1) : -1;
      if (slot < 0) continue;
      if (slot != cur) {                                  // a second component among the lane's 4 pixels: rare
        if (cur >= 0)
          for (int k = 0; k < 7; ++k) {
            atomicAdd(&s_acc[cur * 7 + k], (unsigned long long)a[k]);
            a[k] = 0;
          }
        cur = slot;
      }
      const long long v = masks[p];
      a[0] += 1; a[1] += x; a[2] += y; a[3] += (long long)x * x; a[4] += (long long)y * y; a[5] += (long long)x * y; a[6] += v;
    }
  }
  // per wave: one component in the whole wave (the common case) is summed by shuffles, else every lane adds its own
  const unsigned long long ball = __ballot(cur >= 0);
  if (ball) {                                             // wave-uniform
    const int ref = __shfl(cur, __ffsll((long long)ball) - 1, SPNET_WAVE);
    if (__all(cur < 0 || cur == ref)) {                   // wave-uniform
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const long long t = mf_wave_sum(cur >= 0 ? a[k] : 0ll);
        if ((tid & (SPNET_WAVE - 1)) == 0) atomicAdd(&s_acc[ref * 7 + k], (unsigned long long)t);
      }
    } else if (cur >= 0) {
      for (int k = 0; k < 7; ++k) atomicAdd(&s_acc[cur * 7 + k], (unsigned long long)a[k]);
    }
  }
  __syncthreads();
  for (int k = tid; k < m * 7; k += MF_THREADS) {
    const unsigned long long v = s_acc[k];
    if (v) atomicAdd(reinterpret_cast<unsigned long long*>(out) + (long)(k / 7) * NSUMS + k % 7, v);
  }
}

}  // namespace

extern "C" int spnet_mask_label(const unsigned char* masks, int B, int H, int W, int join_tol, int* labels, void* stream) {
  if (!masks || !mk_int_ok(labels) || B < 0 || !mk_dims_ok(H, W) || join_tol < 0 || join_tol > 255) return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int tx = spnet_cdiv(W, TW), ty = spnet_cdiv(H, TH);
  spnet_for_grid_chunks(B, [&](int b0, int n) {
    hipLaunchKernelGGL(mf_tile_label_kernel, dim3(tx, ty, n), dim3(MF_THREADS), 0, st, masks, b0, H, W, join_tol, labels);
  });
  spnet_for_grid_chunks(B, [&](int b0, int n) {
    hipLaunchKernelGGL(mf_border_merge_kernel, dim3(tx, ty, n), dim3(MF_BORDER_THREADS), 0, st, masks, b0, H, W, join_tol, labels);
  });
  const long total = (long)B * H * W;
  hipLaunchKernelGGL(mf_flatten_kernel, dim3(spnet_ew_grid(total, MF_THREADS)), dim3(MF_THREADS), 0, st, labels, total, H * W);
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_mask_moments(const unsigned char* masks, const int* labels, int B, int H, int W, int C, int* n_components,
                                  long long* sums, void* stream) {
  if (!masks || !mk_int_ok(labels) || !mk_int_ok(n_components) || !sums || ((uintptr_t)sums & 7) || B < 0 || !mk_dims_ok(H, W) ||
      C < 1 || C > MAX_C)
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mf_compact_kernel, dim3(B), dim3(MF_COMPACT_THREADS), 0, st, labels, H * W, C, n_components, sums);
  spnet_for_grid_chunks(B, [&](int b0, int n) {
    const dim3 grid(spnet_cdiv(W, TW), spnet_cdiv(H, TH), n);
    hipLaunchKernelGGL(mf_moments_kernel, grid, dim3(MF_THREADS), 0, st, masks, labels, b0, H, W, C, n_components, sums);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}
