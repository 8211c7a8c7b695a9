// Flip -> rotate -> translate of N one-channel uint8 frames as ONE gather (augment_preproc.py:74-99 through
// spnet/augmentation.py:82-112 flip_image, 184-207 rotate_image, 216-239 translate_image), bit-identical to the three
// steps run one after the other:
//   translate  destination (x, y) takes the rotated image at (u, v) = (x - xt, y - yt), 0 when that lies outside it
//   rotate     cv2.warpAffine's 8-bit path (warp_affine_fixed_kernel in augment.hip): 1/32-pixel coordinates
//              X = (X0[v] + adelta[u]) >> 5, X0[v] = rint((m01 v + m02) 1024) + 16, adelta[u] = rint(m00 u 1024) in
//              float64 with every product and sum rounded on its own, 15-bit weights, zero border
//   flip       the four bilinear taps read the source through the flip: an exact pixel permutation
// One read pass, one write pass, no intermediate image; per frame the host sends a 64-byte record, no tables.
//
// A workgroup owns a TW x TH tile of one output frame:
//   terms   the column terms of its TW columns and the row terms of its TH rows, once each -> LDS
//   stage   the terms are monotone in u and in v, so the tile's corners bound the source pixels it can touch exactly; that
//           box (in MEMORY coordinates, i.e. behind the flip, clipped to the frame) -> LDS as aligned dwords, every row at
//           its memory address modulo 4.  A box that does not fit (a matrix far from a small rotation) is not staged and
//           the taps read the frame through L2 instead: same arithmetic, same bits
//   gather  a lane owns 4 neighbouring pixels of a row: 4 taps each from LDS, packed into one dword of the output tile
//   store   the tile goes through LDS so that lanes own ALIGNED groups of 4 elements in memory: one dword of out_u8 and /
//           or one float4 of out_f per lane (rows of any W start at any alignment)
#include "common.h"
#include "u8_tile.h"

// Diagnostic builds only (tools/warp_time.py --knockouts through tools/build_variant_lib.sh and SPNET_HIP_LIB): where the
// launch's time goes.  The results are wrong by design; the product library is built without the macro.
// 1: the stage loads nothing from global memory; 2: nothing is stored to global memory; 4: one tap per pixel instead of
// four; 8: the box is never staged (every tap reads global memory).
#ifndef SPNET_WARP_KO
#define SPNET_WARP_KO 0
#endif

namespace {

constexpr int KO = SPNET_WARP_KO;
constexpr int TW = 64, TH = 64;          // output tile
constexpr int TWD = TW / 4;              // lanes (dwords) per tile row
constexpr int OP = TW + 4;               // pitch of the output tile in LDS, bytes
constexpr int BOX_BYTES = 24 * 1024;     // staged source box (a 64 x 64 tile turned by 20 degrees needs 84 x 84 pixels)
constexpr int TERM_LIM = 1 << 29;        // |row / column term| is saturated here: sums cannot wrap (2^19 pixels away)
constexpr int SHIFT_LIM = 4096;          // |xt|, |yt| saturate here: past the largest frame either way

struct WarpRecord {                      // one per output frame, 64 bytes (spnet_amd/augmentation.py WARP_RECORD)
  double m[6];                           // inverted matrix: source = m * (u, v, 1)
  int flip, xt, yt, pad;
};

struct WarpArgs {
  const unsigned char* src;
  const int* sel;
  const WarpRecord* rec;
  unsigned char* out_u8;
  float* out_f;
  long src_bytes;
  int n_src, N, H, W, nct, nrt;
};

__device__ __forceinline__ int term(double v) {          // cvRound, saturated
  return (int)fmin(fmax(rint(v), -(double)TERM_LIM), (double)TERM_LIM);
}

__global__ __launch_bounds__(256) void warp_chain_u8_kernel(const WarpArgs a) {
  __shared__ int s_col[TW][2];                                            // (adelta, bdelta) of u = c0 + i - xt
  __shared__ int s_row[TH][2];                                            // (X0, Y0) of v = r0 + j - yt
  __shared__ __attribute__((aligned(16))) unsigned char s_box[BOX_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned char s_out[TH * OP];
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int ct = bid % a.nct;
  bid /= a.nct;
  const int rt = bid % a.nrt;
  const int n = bid / a.nrt;
  const int H = a.H, W = a.W;
  const int c0 = ct * TW, tw = min(W, c0 + TW) - c0;
  const int r0 = rt * TH, nro = min(H, r0 + TH) - r0;

  const WarpRecord* rec = a.rec + n;
  const int flip = rec->flip;
  const bool flipx = flip == 1 || flip == -1, flipy = flip == 0 || flip == -1;
  const int xt = min(max(rec->xt, -SHIFT_LIM), SHIFT_LIM), yt = min(max(rec->yt, -SHIFT_LIM), SHIFT_LIM);
  int sf = a.sel ? a.sel[n] : n;
  sf = min(max(sf, 0), a.n_src - 1);

  // ---- terms: each column's and each row's once, products and sums rounded one by one as numpy rounds them
  if (tid < TW) {
    const double u = (double)(c0 + tid - xt);
    s_col[tid][0] = term(__dmul_rn(__dmul_rn(rec->m[0], u), 1024.0));
    s_col[tid][1] = term(__dmul_rn(__dmul_rn(rec->m[3], u), 1024.0));
  } else if (tid < TW + TH) {
    const double v = (double)(r0 + tid - TW - yt);
    s_row[tid - TW][0] = term(__dmul_rn(__dadd_rn(__dmul_rn(rec->m[1], v), rec->m[2]), 1024.0)) + 16;
    s_row[tid - TW][1] = term(__dmul_rn(__dadd_rn(__dmul_rn(rec->m[4], v), rec->m[5]), 1024.0)) + 16;
  }
  __syncthreads();

  // ---- the tile's pixels whose (u, v) lies inside the rotated image, and the source box they can touch
  const int i0 = max(0, xt - c0), i1 = min(tw, W + xt - c0);              // tile columns [i0, i1)
  const int j0 = max(0, yt - r0), j1 = min(nro, H + yt - r0);             // tile rows [j0, j1)
  int bx0 = 0, by0 = 0, bw = 0, bh = 0;                                   // staged box, memory coordinates
  bool staged = false;
  if (i0 < i1 && j0 < j1) {
    const int ca = s_col[i0][0], cb = s_col[i1 - 1][0], ra = s_row[j0][0], rb = s_row[j1 - 1][0];
    const int da = s_col[i0][1], db = s_col[i1 - 1][1], ea = s_row[j0][1], eb = s_row[j1 - 1][1];
    int x_lo = (min(ca, cb) + min(ra, rb)) >> 10, x_hi = ((max(ca, cb) + max(ra, rb)) >> 10) + 1;
    int y_lo = (min(da, db) + min(ea, eb)) >> 10, y_hi = ((max(da, db) + max(ea, eb)) >> 10) + 1;
    x_lo = max(x_lo, 0); x_hi = min(x_hi, W - 1);
    y_lo = max(y_lo, 0); y_hi = min(y_hi, H - 1);
    if (x_lo <= x_hi && y_lo <= y_hi) {
      bx0 = flipx ? W - 1 - x_hi : x_lo;
      by0 = flipy ? H - 1 - y_hi : y_lo;
      bw = x_hi - x_lo + 1;
      bh = y_hi - y_lo + 1;
    }
  }
  const int pitch = ((bw + 6) >> 2) << 2;                                 // bw bytes + 3 of misalignment, in dwords
  staged = bw > 0 && (long)pitch * bh <= BOX_BYTES && !(KO & 8);
  const unsigned char* frame = a.src + (long)sf * H * W;
  const long fb = (long)((uintptr_t)frame & 3) + bx0;                      // (fb + my * W) & 3: where a staged row begins

  if (staged) {
    const int sb = (int)((uintptr_t)a.src & 3);
    const unsigned char* src4 = a.src - sb;                               // byte b of the source = src4[sb + b]
    const long f0 = (long)sf * H * W + sb;
    const int npd = pitch >> 2;
    for (int i = tid; i < bh * npd; i += 256) {
      const int row = i / npd, c = i - row * npd;
      const long g = f0 + (long)(by0 + row) * W + bx0;
      const int off = (int)(g & 3);
      if (c * 4 >= off + bw) continue;
      const long b = g - off + (long)c * 4;
      unsigned q = 0u;
      if ((KO & 1) && a.N > 0) {
        q = (unsigned)b * 0x01010101u;
      } else if (b >= sb && b + 4 <= sb + a.src_bytes) {
        q = *reinterpret_cast<const unsigned*>(src4 + b);
      } else {                                                            // the first / last bytes of the source
        for (int k = 0; k < 4; ++k)
          if (b + k >= sb && b + k < sb + a.src_bytes) q |= (unsigned)src4[b + k] << (k * 8);
      }
      *reinterpret_cast<unsigned*>(s_box + row * pitch + c * 4) = q;
    }
  } else if (bw > 0) {                                                    // unstaged: the "box" is the whole frame
    bx0 = 0; by0 = 0; bw = W; bh = H;
  }
  __syncthreads();

  // ---- gather: 4 neighbouring pixels per lane, 16 rows per pass
  const int dc = tid & (TWD - 1), rg = tid / TWD;
  for (int j = rg; j < nro; j += 256 / TWD) {
    unsigned packed = 0u;
    if (j >= j0 && j < j1 && bw > 0) {
      const int X0 = s_row[j][0], Y0 = s_row[j][1];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = dc * 4 + k;
        if (i < i0 || i >= i1) continue;
        const int X = (X0 + s_col[i][0]) >> 5, Y = (Y0 + s_col[i][1]) >> 5;
        const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
        const int w00 = min((32 - fy) * (32 - fx) * 32, 32767), w01 = (32 - fy) * fx * 32;   // int16 table entries
        const int w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
        const bool vy0 = sy >= 0 && sy < H, vy1 = sy + 1 >= 0 && sy + 1 < H;
        const bool vx0 = sx >= 0 && sx < W, vx1 = sx + 1 >= 0 && sx + 1 < W;
        // memory coordinates behind the flip, clamped into the box (an invalid tap is masked, its address stays legal)
        const int cx0 = min(max(sx, 0), W - 1), cx1 = min(max(sx + 1, 0), W - 1);
        const int cy0 = min(max(sy, 0), H - 1), cy1 = min(max(sy + 1, 0), H - 1);
        const int mx0 = min(max(flipx ? W - 1 - cx0 : cx0, bx0), bx0 + bw - 1) - bx0;
        const int mx1 = min(max(flipx ? W - 1 - cx1 : cx1, bx0), bx0 + bw - 1) - bx0;
        const int my0 = min(max(flipy ? H - 1 - cy0 : cy0, by0), by0 + bh - 1);
        const int my1 = min(max(flipy ? H - 1 - cy1 : cy1, by0), by0 + bh - 1);
        int p00, p01, p10, p11;
        if (staged) {
          const unsigned char* q0 = s_box + (my0 - by0) * pitch + (int)((fb + (long)my0 * W) & 3);
          const unsigned char* q1 = s_box + (my1 - by0) * pitch + (int)((fb + (long)my1 * W) & 3);
          p00 = q0[mx0];
          p01 = (KO & 4) ? p00 : q0[mx1];
          p10 = (KO & 4) ? p00 : q1[mx0];
          p11 = (KO & 4) ? p00 : q1[mx1];
        } else {
          const unsigned char* q0 = frame + (long)my0 * W;
          const unsigned char* q1 = frame + (long)my1 * W;
          p00 = q0[mx0]; p01 = q0[mx1]; p10 = q1[mx0]; p11 = q1[mx1];
        }
        p00 = (vy0 && vx0) ? p00 : 0;
        p01 = (vy0 && vx1) ? p01 : 0;
        p10 = (vy1 && vx0) ? p10 : 0;
        p11 = (vy1 && vx1) ? p11 : 0;
        const int v = (p00 * w00 + p01 * w01 + p10 * w10 + p11 * w11 + (1 << 14)) >> 15;
        packed |= (unsigned)min(max(v, 0), 255) << (8 * k);
      }
    }
    *reinterpret_cast<unsigned*>(s_out + j * OP + dc * 4) = packed;
  }
  __syncthreads();

  // ---- store: a lane owns 4 elements that share an aligned dword (out_u8) / float4 (out_f) IN MEMORY
  const long row0 = ((long)n * H + r0) * W + c0;
  if ((KO & 2) && a.N > 0 && s_out[tid] != 77) return;                    // (keeps the work above alive)
  if (a.out_u8) store_tile<unsigned char>(a.out_u8, s_out, OP, row0, W, nro, tw, TWD + 1, tid);
  if (a.out_f) store_tile<float>(a.out_f, s_out, OP, row0, W, nro, tw, TWD + 1, tid);
}

}  // namespace

extern "C" int spnet_warp_chain_u8(const unsigned char* src, int n_src, const int* sel, const void* params, int N, int H, int W,
                                   unsigned char* out_u8, float* out_f, void* stream) {
  const int LIM = 2048;
  static_assert(sizeof(WarpRecord) == 64, "the host packs 64-byte records");
  if (!src || !params || n_src < 1 || N < 0 || H < 1 || W < 1 || H > LIM || W > LIM) return (int)hipErrorInvalidValue;
  if (!out_u8 && !out_f) return (int)hipErrorInvalidValue;
  if (!sel && N > n_src) return (int)hipErrorInvalidValue;               // without sel, frame n comes from source frame n
  if ((((uintptr_t)out_f | (uintptr_t)sel) & 3) || ((uintptr_t)params & 7)) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  WarpArgs a;
  a.src = src; a.sel = sel; a.rec = reinterpret_cast<const WarpRecord*>(params); a.out_u8 = out_u8; a.out_f = out_f;
  a.src_bytes = (long)n_src * H * W;
  a.n_src = n_src; a.N = N; a.H = H; a.W = W;
  a.nct = spnet_cdiv(W, TW);
  a.nrt = spnet_cdiv(H, TH);
  const long blocks = (long)N * a.nct * a.nrt;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(warp_chain_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  SPNET_RETURN_LAUNCH_STATUS();
}
