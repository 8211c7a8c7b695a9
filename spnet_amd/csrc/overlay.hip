// Prediction overlays (spnet/utils.py:67-137, show_pred_ellipses) drawn on frames that are already in device memory:
// ellipse outlines as 72-gons of round-jointed segments, ring-count labels and the file name as coverage-mask blits.
// spnet_amd/overlay.py is the host side (selection, order, vertices in 1/16 pixel, masks from Pillow's font, boxes).
//
// One workgroup per 64 x 16 tile of a frame.  The frame's command list is culled against the tile 256 commands at a time
// into an LDS list that keeps command order (ballot + prefix count, no atomics); after every round each thread walks the
// list in order over the 4 pixels it owns (registers), so a frame with more commands than the list holds simply takes
// more rounds.  A tile no command touches is copied grey -> RGB with 16-byte loads and stores where W % 16 == 0 and the
// buffers are 16-byte aligned.
//
// The outline rule is integer arithmetic only (see overlay.py): the restatement in tests/helpers/overlay_ref.py agrees
// bit for bit.  Inside an edge's box grown by r, |v| <= |e| + r per component, and the plan keeps |e| < 2^13 per component
// (outlines with longer edges arrive with an empty box and are culled): dot products stay below 2^28 (int32), the squared
// cross product and r^2 * L2 below 2^55 (int64).
#include "common.h"

namespace {

constexpr int OV_TW = 64, OV_TH = 16, OV_THREADS = 256, OV_CAP = 256, OV_CW = 12, OV_VERTS = 72;
constexpr int OV_SUB = 16, OV_CENTER = 8, OV_R = 24;            // overlay.py: SUBPIXEL, CENTER, RADIUS

__device__ __forceinline__ unsigned ov_blend(unsigned dst, unsigned ink, unsigned m) {
  const unsigned t = dst * (255u - m) + ink * m + 128u;
  return ((t >> 8) + t) >> 8;
}

__device__ __forceinline__ unsigned ov_blend_rgb(unsigned dst, unsigned ink, unsigned m) {
  return ov_blend(dst & 255u, ink & 255u, m) | ov_blend((dst >> 8) & 255u, (ink >> 8) & 255u, m) << 8 |
         ov_blend((dst >> 16) & 255u, (ink >> 16) & 255u, m) << 16;
}

// Does the closed polygon v[0..72) paint pixels px .. px+3 of row py?  bit i of the result: pixel px + i.  `want`: the
// pixels that may be painted at all (inside the command's box).
__device__ __forceinline__ unsigned ov_outline(const int* __restrict__ v, int px, int py, unsigned want) {
  const int cy = py * OV_SUB + OV_CENTER;
  const int cx0 = px * OV_SUB + OV_CENTER;
  unsigned got = 0;
  int Px = v[0], Py = v[1];
  for (int k = 0; k < OV_VERTS && got != want; ++k) {
    const int kq = (k + 1 == OV_VERTS) ? 0 : k + 1;
    const int Qx = v[2 * kq], Qy = v[2 * kq + 1];
    const int lox = min(Px, Qx) - OV_R, hix = max(Px, Qx) + OV_R;
    const int loy = min(Py, Qy) - OV_R, hiy = max(Py, Qy) + OV_R;
    if (cy >= loy && cy <= hiy && cx0 + 3 * OV_SUB >= lox && cx0 <= hix) {
      const int ex = Qx - Px, ey = Qy - Py;
      const int vy = cy - Py, wy = cy - Qy;
      const int L2 = ex * ex + ey * ey;
      const long long rl = (long long)(OV_R * OV_R) * L2;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int cx = cx0 + i * OV_SUB;
        if (!((want & ~got) >> i & 1u) || cx < lox || cx > hix) continue;
        const int vx = cx - Px;
        const int t = vx * ex + vy * ey;
        bool hit;
        if (t <= 0) {
          hit = vx * vx + vy * vy <= OV_R * OV_R;
        } else if (t >= L2) {
          const int wx = cx - Qx;
          hit = wx * wx + wy * wy <= OV_R * OV_R;
        } else {
          const long long cr = (long long)vx * ey - (long long)vy * ex;
          hit = cr * cr <= rl;
        }
        if (hit) got |= 1u << i;
      }
    }
    Px = Qx;
    Py = Qy;
  }
  return got;
}

__global__ __launch_bounds__(OV_THREADS) void overlay_kernel(const unsigned char* __restrict__ frames, int n_base, int H, int W,
                                                             int channels, const int* __restrict__ frame_start,
                                                             const int* __restrict__ cmd, int n_cmd,
                                                             const int* __restrict__ verts, int n_verts,
                                                             const unsigned char* __restrict__ masks, long mask_bytes,
                                                             unsigned char* __restrict__ out, int vec16) {
  __shared__ int s_list[OV_CAP];
  __shared__ int s_wave[OV_THREADS / SPNET_WAVE];
  __shared__ __attribute__((aligned(16))) unsigned char s_grey[OV_TH][OV_TW];

  const int n = n_base + blockIdx.z;
  const int x0 = blockIdx.x * OV_TW, y0 = blockIdx.y * OV_TH;
  const int x1 = min(x0 + OV_TW, W), y1 = min(y0 + OV_TH, H);
  const int tid = threadIdx.x, lane = tid & (SPNET_WAVE - 1), wave = tid / SPNET_WAVE;
  const int px = x0 + (tid & 15) * 4, py = y0 + (tid >> 4);
  const bool mine = py < y1 && px < x1;                   // this thread owns pixels px .. min(px + 4, W) - 1 of row py
  const long pixel0 = ((long)n * H + py) * W + px;        // only used when `mine`
  const int c0 = max(frame_start[n], 0), c1 = min(frame_start[n + 1], n_cmd);

  unsigned pix[4] = {0u, 0u, 0u, 0u};                     // r | g << 8 | b << 16
  bool loaded = false;                                    // uniform over the workgroup

  auto load_pixels = [&]() {
    if (!mine) return;
    if (channels == 1) {
      if (vec16) {
        const unsigned g = *reinterpret_cast<const unsigned*>(frames + pixel0);
#pragma unroll
        for (int i = 0; i < 4; ++i) pix[i] = ((g >> (8 * i)) & 255u) * 0x010101u;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (px + i < x1) pix[i] = (unsigned)frames[pixel0 + i] * 0x010101u;
      }
    } else {
      const unsigned char* p = frames + pixel0 * 3;
      if (vec16) {
        const unsigned a = reinterpret_cast<const unsigned*>(p)[0], b = reinterpret_cast<const unsigned*>(p)[1],
                       c = reinterpret_cast<const unsigned*>(p)[2];
        pix[0] = a & 0xffffffu;
        pix[1] = (a >> 24) | (b & 0xffffu) << 8;
        pix[2] = (b >> 16) | (c & 0xffu) << 16;
        pix[3] = c >> 8;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (px + i < x1) pix[i] = (unsigned)p[3 * i] | (unsigned)p[3 * i + 1] << 8 | (unsigned)p[3 * i + 2] << 16;
      }
    }
  };

  for (int base = c0; base < c1; base += OV_CAP) {
    // ---- cull commands base .. base + 255 against the tile, keeping their order
    const int c = base + tid;
    bool hit = false;
    if (c < c1) {
      const int* k = cmd + (long)c * OV_CW;
      const int bx0 = max(k[2], 0), by0 = max(k[3], 0), bx1 = min(k[4], W), by1 = min(k[5], H);
      hit = bx0 < x1 && bx1 > x0 && by0 < y1 && by1 > y0;
      const long data = k[6];
      if (k[0] == 0) {
        hit = hit && data >= 0 && data + OV_VERTS <= n_verts;
      } else {
        const long mw = k[9], mh = k[10];
        hit = hit && k[0] == 1 && data >= 0 && mw > 0 && mh > 0 && mw <= 65536 && mh <= 65536 && data + mw * mh <= mask_bytes;
      }
    }
    const unsigned long long ball = __ballot(hit);
    if (lane == 0) s_wave[wave] = __popcll(ball);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < OV_THREADS / SPNET_WAVE; ++w) {
      const int cnt = s_wave[w];
      before += (w < wave) ? cnt : 0;
      total += cnt;
    }
    if (hit) s_list[before + __popcll(ball & ((1ull << lane) - 1ull))] = c;
    __syncthreads();

    // ---- paint: every thread walks the culled list in order over its own pixels
    if (total > 0) {
      if (!loaded) {
        load_pixels();
        loaded = true;
      }
      for (int i = 0; i < total; ++i) {
        const int ci = __builtin_amdgcn_readfirstlane(s_list[i]);
        const int* k = cmd + (long)ci * OV_CW;
        const int kind = k[0];
        const unsigned ink = (unsigned)k[1] & 0xffffffu;
        const int bx0 = max(k[2], 0), by0 = max(k[3], 0), bx1 = min(k[4], W), by1 = min(k[5], H);
        if (!mine || py < by0 || py >= by1 || px + 3 < bx0 || px >= bx1) continue;
        unsigned want = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (px + j >= bx0 && px + j < bx1) want |= 1u << j;
        if (kind == 0) {
          const unsigned got = ov_outline(verts + 2 * (long)k[6], px, py, want);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (got >> j & 1u) pix[j] = ink;
        } else {
          const int mx = k[7], my = k[8], mw = k[9], mh = k[10];
          const int ry = py - my;
          if (ry < 0 || ry >= mh) continue;
          const unsigned char* row = masks + (long)k[6] + (long)ry * mw;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int rx = px + j - mx;
            if ((want >> j & 1u) && rx >= 0 && rx < mw) pix[j] = ov_blend_rgb(pix[j], ink, row[rx]);
          }
        }
      }
    }
    __syncthreads();                                      // s_list / s_wave are rewritten by the next round
  }

  if (!loaded && vec16) {
    // ---- no command touches this tile: grey -> RGB (or RGB -> RGB) copy, 16 bytes per access
    const int tw = x1 - x0, th = y1 - y0;                 // tw is a multiple of 16 here
    const long row0 = ((long)n * H + y0) * W + x0;        // pixel index of the tile's first pixel; rows are W apart
    if (channels == 1) {
      const int ipr = tw / 16;
      if (tid < th * ipr) {
        const int r = tid / ipr, j = tid - r * ipr;
        *reinterpret_cast<uint4*>(&s_grey[r][16 * j]) = *reinterpret_cast<const uint4*>(frames + row0 + (long)r * W + 16 * j);
      }
      __syncthreads();
      const int opr = tw * 3 / 16;
      if (tid < th * opr) {
        const int r = tid / opr, j = tid - r * opr;
        unsigned w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          unsigned word = 0;
#pragma unroll
          for (int b = 0; b < 4; ++b) word |= (unsigned)s_grey[r][(16 * j + 4 * q + b) / 3] << (8 * b);
          w[q] = word;
        }
        *reinterpret_cast<uint4*>(out + (row0 + (long)r * W) * 3 + 16 * j) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    } else {
      const int opr = tw * 3 / 16;
      if (tid < th * opr) {
        const int r = tid / opr, j = tid - r * opr;
        const long o = (row0 + (long)r * W) * 3 + 16 * j;
        *reinterpret_cast<uint4*>(out + o) = *reinterpret_cast<const uint4*>(frames + o);
      }
    }
    return;
  }
  if (!loaded) load_pixels();
  if (!mine) return;
  unsigned char* o = out + pixel0 * 3;
  if (vec16) {
    reinterpret_cast<unsigned*>(o)[0] = pix[0] | pix[1] << 24;
    reinterpret_cast<unsigned*>(o)[1] = pix[1] >> 8 | pix[2] << 16;
    reinterpret_cast<unsigned*>(o)[2] = pix[2] >> 16 | pix[3] << 8;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (px + i < x1) {
        o[3 * i] = (unsigned char)pix[i];
        o[3 * i + 1] = (unsigned char)(pix[i] >> 8);
        o[3 * i + 2] = (unsigned char)(pix[i] >> 16);
      }
  }
}

}  // namespace

extern "C" int spnet_draw_overlays(const unsigned char* frames, int N, int H, int W, int channels, const int* frame_start,
                                   const int* cmd, int n_cmd, const int* verts, int n_verts, const unsigned char* masks,
                                   long mask_bytes, unsigned char* out, void* stream) {
  if (N == 0) return 0;
  if (N < 0 || H < 1 || W < 1 || H > 4096 || W > 4096 || (channels != 1 && channels != 3) || n_cmd < 0 || n_verts < 0 ||
      mask_bytes < 0 || !frames || !frame_start || !out || (n_cmd > 0 && !cmd) || (n_verts > 0 && !verts) ||
      (mask_bytes > 0 && !masks) || ((uintptr_t)frame_start & 3) || ((uintptr_t)cmd & 3) || ((uintptr_t)verts & 3))
    return (int)hipErrorInvalidValue;
  const int vec16 = (W % 16 == 0) && !((uintptr_t)frames & 15) && !((uintptr_t)out & 15);
  spnet_for_grid_chunks(N, [&](int n0, int n) {
    const dim3 grid(spnet_cdiv(W, OV_TW), spnet_cdiv(H, OV_TH), n);
    hipLaunchKernelGGL(overlay_kernel, grid, dim3(OV_THREADS), 0, (hipStream_t)stream, frames, n0, H, W, channels, frame_start,
                       cmd, n_cmd, verts, n_verts, masks, mask_bytes, out, vec16);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}
