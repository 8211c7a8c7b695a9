// Grid targets of B frames from their metadata rows, on the device: parse_meta_file's row processing -> true_to_pred_grid ->
// norm_Y (spnet/utils.py:260-286, 191-244, 181-184), bit-identical to spnet_amd/augmentation.py _encode_targets, and -- given
// the frames' warp records -- warp_metadata and warp_targets' rejection ahead of it (flip_image -> rotate_image ->
// translate_image's metadata halves, spnet/augmentation.py:91-104, 196-204, 230).
//
// One wave per frame:
//   rows    lane k < count holds ellipse k: the warp arithmetic, the a/b swap and the cell of its centre, all in float64
//           with every operation rounded on its own
//   order   the host sorts the kept rows by (cx, cy), stably, and hands out a cell's slots in that order; a lane's slot is
//           the number of kept lanes of its cell that come before it in that order (K <= 16 shuffles, no sort is formed)
//   reject  a warped frame with an ellipse beyond its cell's slots is placed again from its unwarped rows, and its warp
//           record is overwritten with the identity: the warp launch that follows then copies the frame
//   write   the placed lanes put their eight normalised values into LDS; all 64 lanes then write the frame's row of Y, one
//           element each per pass, an element from the ellipse that owns its (cell, slot) or else the blank value
#include "common.h"

// every product and sum below is rounded on its own, as numpy rounds it (__dmul_rn / __dadd_rn are plain operators here)
#pragma clang fp contract(off)

namespace {

constexpr int MAX_K = 16;                // spnet_amd/augmentation.py MAX_OBJECTS
constexpr int CLEANUP_TURNS = 64;        // cleanup_angle's loops stop here: an angle beyond +-11,520 degrees (or inf) ends

struct WarpRecord {                      // csrc/warp.hip, spnet_amd/augmentation.py WARP_RECORD
  double m[6];
  int flip, xt, yt, pad;
};

struct TargetArgs {
  const double* rows;
  const int* count;
  const float* trig;
  const double* fwd;
  WarpRecord* rec;
  float* Y;
  int* flags;
  int K, nx, ny, ns, H, W, xbin, ybin;
};

// NaN sorts last and equal to itself, as numpy orders it: the order stays total whatever the rows hold
__device__ __forceinline__ bool lt(double a, double b) { return a < b || (a == a && b != b); }
__device__ __forceinline__ bool eq(double a, double b) { return a == b || (a != a && b != b); }

__device__ __forceinline__ double cleanup_angle(double a) {
  for (int i = 0; i < CLEANUP_TURNS && a < 0.0; ++i) a = __dadd_rn(a, 180.0);
  for (int i = 0; i < CLEANUP_TURNS && a >= 180.0; ++i) a = __dsub_rn(a, 180.0);
  return a;
}

// clip(trunc((c - 40) / bin), 0, n - 1); NaN goes to cell 0
__device__ __forceinline__ int cell_index(double c, int bin, int n) {
  const double t = trunc(__ddiv_rn(__dsub_rn(c, 40.0), (double)bin));
  return (int)fmin(fmax(t, 0.0), (double)(n - 1));
}

// Slot of this lane's ellipse in its cell (meaningful where keep), by counting the kept lanes before it in the host's
// sorted order.  Every lane of the wave calls it.
__device__ __forceinline__ int slot_of(double cx, double cy, bool keep, int cell, int lane, int K) {
  int slot = 0;
  for (int j = 0; j < K; ++j) {
    const double xj = __shfl(cx, j, 64), yj = __shfl(cy, j, 64);
    const int cj = __shfl(cell, j, 64);
    const bool kj = __shfl((int)keep, j, 64) != 0;
    const bool before = lt(xj, cx) || (eq(xj, cx) && (lt(yj, cy) || (eq(yj, cy) && j < lane)));
    slot += (kj && cj == cell && before) ? 1 : 0;
  }
  return slot;
}

// mean, range and blank value of variable v of cell (ix, iy): setup_means_and_ranges, in the float32 it stores them in
__device__ __forceinline__ void cell_codec(const TargetArgs& a, int v, int ix, int iy, float& mean, float& range, float& blank) {
  const float gx = (float)((double)((long)ix * a.xbin + 40) + (double)a.xbin / 2.0);
  const float gy = (float)((double)((long)iy * a.ybin + 40) + (double)a.ybin / 2.0);
  const float hx = (float)((double)a.xbin / 2.0), hy = (float)((double)a.ybin / 2.0);
  switch (v) {
    case 0: mean = gx; range = (float)a.xbin; blank = gx; break;
    case 1: mean = gy; range = (float)a.ybin; blank = gy; break;
    case 2: mean = hx; range = (float)a.xbin; blank = hx; break;
    case 3: mean = hy; range = (float)a.ybin; blank = hy; break;
    case 4: mean = 0.f; range = 2.f; blank = -1.f; break;
    case 5: mean = 0.f; range = 2.f; blank = 0.f; break;
    case 6: mean = 0.f; range = 1.f; blank = 1.f; break;
    default: mean = 5.f; range = 10.f; blank = 0.f; break;
  }
}

__device__ __forceinline__ float norm(float g, float mean, float range) { return __fdiv_rn(__fsub_rn(g, mean), range); }

__global__ __launch_bounds__(64) void encode_targets_kernel(const TargetArgs a) {
  __shared__ int s_cs[MAX_K];                                             // cell * ns + slot of a placed lane, else -1
  __shared__ float s_val[MAX_K][8];
  const int lane = threadIdx.x;
  const long b = blockIdx.x;
  const int K = a.K, ns = a.ns;
  const int cnt = min(max(a.count[b], 0), K);
  const bool live = lane < cnt;

  double cx = 0.0, cy = 0.0, ea = 0.0, eb = 0.0, ang = 0.0, rings = 0.0;
  if (live) {
    const double* r = a.rows + (b * K + lane) * 6;
    cx = r[0]; cy = r[1]; ea = r[2]; eb = r[3]; ang = r[4]; rings = r[5];
  }
  const bool keep = live && rings > 0.0;

  // ---- warp_metadata: flip reflections, rotation, shift
  double wx = cx, wy = cy, wang = ang;
  if (a.fwd) {
    const WarpRecord* rec = a.rec + b;
    const double* f = a.fwd + b * 8;
    const int flip = rec->flip;
    const double rot = f[6];
    if (flip == 0 || flip == -1) { wy = __dsub_rn((double)a.H, wy); wang = -wang; }
    if (flip != -2) wang = cleanup_angle(wang);
    if (flip == 1 || flip == -1) { wx = __dsub_rn((double)a.W, wx); wang = __dsub_rn(180.0, wang); }
    if (flip != -2) wang = cleanup_angle(wang);
    if (rot != 0.0) {
      wang = cleanup_angle(__dadd_rn(wang, rot));
      const double px = __dadd_rn(__dadd_rn(__dmul_rn(f[0], wx), __dmul_rn(f[1], wy)), f[2]);
      const double py = __dadd_rn(__dadd_rn(__dmul_rn(f[3], wx), __dmul_rn(f[4], wy)), f[5]);
      wx = rint(px);
      wy = rint(py);
    }
    wx = __dadd_rn(wx, (double)rec->xt);
    wy = __dadd_rn(wy, (double)rec->yt);
  }

  // ---- placement; a warped frame that overflows a cell falls back to its unwarped rows
  int ix = cell_index(wx, a.xbin, a.nx), iy = cell_index(wy, a.ybin, a.ny);
  int slot = slot_of(wx, wy, keep, ix * a.ny + iy, lane, K);
  int flag = __any(keep && slot >= ns) ? 1 : 0;
  if (a.fwd && flag) {                                                    // (wave-uniform)
    wx = cx; wy = cy; wang = ang;
    ix = cell_index(wx, a.xbin, a.nx);
    iy = cell_index(wy, a.ybin, a.ny);
    slot = slot_of(wx, wy, keep, ix * a.ny + iy, lane, K);
    if (__any(keep && slot >= ns)) flag = 2;
    WarpRecord* rec = a.rec + b;
    if (lane < 6) rec->m[lane] = (lane == 0 || lane == 4) ? 1.0 : 0.0;
    else if (lane == 6) rec->flip = -2;
    else if (lane == 7) rec->xt = 0;
    else if (lane == 8) rec->yt = 0;
  }

  // ---- the placed ellipses' normalised values -> LDS
  const bool put = keep && slot < ns;
  if (lane < MAX_K) s_cs[lane] = put ? (ix * a.ny + iy) * ns + slot : -1;
  if (put) {
    const bool swap = eb > ea;
    const double aa = swap ? eb : ea, bb = swap ? ea : eb;
    const double t = swap ? __dadd_rn(wang, 90.0) : wang;
    float c2, s2;
    if (t >= 0.0 && t < 360.0 && t == trunc(t)) {                         // whole degrees: the host's own table
      c2 = a.trig[2 * (int)t];
      s2 = a.trig[2 * (int)t + 1];
    } else {                                                              // 2 * np.deg2rad(angle)
      const double r2 = __dmul_rn(2.0, __dmul_rn(t, 3.14159265358979323846 / 180.0));
      c2 = (float)cos(r2);
      s2 = (float)sin(r2);
    }
    const float g[8] = {(float)wx, (float)wy, (float)aa, (float)bb, c2, s2, 0.f, (float)rings};
#pragma unroll
    for (int v = 0; v < 8; ++v) {
      float mean, range, blank;
      cell_codec(a, v, ix, iy, mean, range, blank);
      s_val[lane][v] = norm(g[v], mean, range);
    }
  }
  __syncthreads();

  // ---- the frame's row of Y
  const long nel = (long)a.nx * a.ny * ns * 8;
  float* y = a.Y + b * nel;
  for (long e = lane; e < nel; e += 64) {
    const int cs = (int)(e >> 3), v = (int)(e & 7);
    const int cell = cs / ns;
    float mean, range, blank;
    cell_codec(a, v, cell / a.ny, cell % a.ny, mean, range, blank);
    float out = norm(blank, mean, range);
    for (int j = 0; j < K; ++j)
      if (s_cs[j] == cs) out = s_val[j][v];
    y[e] = out;
  }
  if (lane == 0) a.flags[b] = flag;
}

}  // namespace

extern "C" int spnet_encode_targets(const double* rows, const int* count, int B, int K, int nx, int ny, int ns, int H, int W,
                                    const float* trig, const double* fwd, void* warp_records, float* Y, int* flags,
                                    void* stream) {
  static_assert(sizeof(WarpRecord) == 64, "the host packs 64-byte records");
  if (!rows || !count || !trig || !Y || !flags || B < 0 || K < 1 || K > MAX_K || nx < 1 || ny < 1 || ns < 1)
    return (int)hipErrorInvalidValue;
  if ((fwd == nullptr) != (warp_records == nullptr)) return (int)hipErrorInvalidValue;
  if (fwd && (H < 1 || W < 1)) return (int)hipErrorInvalidValue;
  if (nx > 430 || ny > 310) return (int)hipErrorInvalidValue;             // a bin of 0 pixels: the host codec divides by it
  if ((long)nx * ny * ns > (1L << 24)) return (int)hipErrorInvalidValue;  // (cell, slot) numbers stay far inside an int
  if ((((uintptr_t)rows | (uintptr_t)fwd | (uintptr_t)warp_records) & 7) ||
      (((uintptr_t)count | (uintptr_t)trig | (uintptr_t)Y | (uintptr_t)flags) & 3))
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  TargetArgs a;
  a.rows = rows; a.count = count; a.trig = trig; a.fwd = fwd; a.rec = reinterpret_cast<WarpRecord*>(warp_records);
  a.Y = Y; a.flags = flags;
  a.K = K; a.nx = nx; a.ny = ny; a.ns = ns; a.H = H; a.W = W;
  a.xbin = 430 / nx;
  a.ybin = 310 / ny;
  hipLaunchKernelGGL(encode_targets_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, a);
  SPNET_RETURN_LAUNCH_STATUS();
}
