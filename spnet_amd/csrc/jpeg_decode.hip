// Baseline JPEG decoding of N files whose entropy-coded bytes sit in device memory: the inverse of jpeg.hip, but general --
// the files this project reads were written by jpeg.hip, Pillow / libjpeg and cameras' Motion-JPEG encoders, so custom
// Huffman tables, files with and without restart markers and chroma subsampled 2x1 and 2x2 occur.  Replaces the decoder
// behind Image.open(...).convert("RGB") (spnet/utils.py:325-345) for such files; the container (markers, tables, the
// search for the restart markers) stays on the host (spnet_amd/jpeg.py).  The decoder itself -- bit reader, Huffman
// decoding with its rejection rules, the inverse DCT, upsampling, colour -- is jpeg_decode_core.h, which
// tools/jpeg_decode_host_check.cpp runs under host sanitizers.
//
//   spnet_jpeg_entropy  ONE LANE PER RESTART INTERVAL.  An interval is byte aligned and starts with the DC predictors at 0,
//                       so intervals are independent; inside one, Huffman decoding is serial in its symbols.  jpeg.hip
//                       writes an interval per MCU row (48 per 384 x 512 frame), so a batch of 512 frames is 24,576 lanes;
//                       a file without restart markers is one interval, and the parallelism is then across files only, as
//                       for inflate.  A workgroup is one wave; the Huffman table set (3,616 bytes: four tables of an 8-bit
//                       lookahead, maxcode / valoff for the longer codes and the symbols) sits in LDS, loaded once per
//                       workgroup -- the host orders the intervals so that a workgroup's 64 share one set (all frames of
//                       a movie do).  The bit buffer (64 bits, left aligned) and the predictors live in registers; bytes
//                       are fetched from the blob one at a time by each lane.  Coefficients go to the int16 workspace in
//                       NATURAL order (the zigzag is undone here), [file][component][block][64]; the workspace arrives
//                       zeroed, so only non-zero coefficients are stored.
//   spnet_jpeg_pixels   a workgroup of 256 threads per 32 x 128 tile of a frame.  Phase 1, a thread per 8 x 8 block of the
//                       tile (and, for subsampled chroma, of the one-block halo the triangle filter reaches into): the 64
//                       coefficients are read once as eight 16-byte loads, dequantised and run through both passes of the
//                       islow inverse DCT in registers; the samples go to the component's plane in LDS (12 KiB for three
//                       components).  Phase 2, a thread per 4 pixels of a row: upsampling, colour, crop; one dword store
//                       for `first` and three for RGB where the four pixels are whole and the address is aligned
//                       (u8_tile.h's put4), single bytes otherwise.
#include "common.h"
#include "jpeg_decode_core.h"
#include "u8_tile.h"

namespace {

using namespace jpegdec;

constexpr int JD_MAX_DIM = 65535;
constexpr int PX_T = 256, PX_TILE_H = 32, PX_TILE_W = 128;
constexpr int PX_PLANE = PX_TILE_H * PX_TILE_W;          // bytes of a component's plane: 4 x 16 blocks; subsampled: 4 x 10

__global__ __launch_bounds__(SPNET_WAVE) void jpeg_entropy_kernel(const unsigned char* __restrict__ blob, long blob_bytes,
                                                                  const int* __restrict__ intervals, int n_intervals,
                                                                  const int* __restrict__ files, int n_files,
                                                                  const uint32_t* __restrict__ tables, int n_sets,
                                                                  int16_t* __restrict__ coef, long total_blocks,
                                                                  int* __restrict__ status) {
  __shared__ TableSet s_set;
  const int lane = threadIdx.x;
  const long first = (long)blockIdx.x * SPNET_WAVE;                       // < n_intervals (launcher)
  // the workgroup's table set: that of its first interval's file (uniform)
  const int f0 = intervals[first * INTERVAL_INTS + 2];
  int set = -1;
  if (f0 >= 0 && f0 < n_files) set = files[(long)f0 * FILE_INTS + F_TABLE_SET];
  if (set < 0 || set >= n_sets) set = -1;
  if (set >= 0) {
    uint32_t* dst = reinterpret_cast<uint32_t*>(&s_set);
    const uint32_t* src = tables + (long)set * (4 * TABLE_WORDS);
    for (int w = lane; w < 4 * TABLE_WORDS; w += SPNET_WAVE) dst[w] = src[w];
  }
  __syncthreads();
  const long i = first + lane;
  if (i >= n_intervals) return;
  const int* iv = intervals + i * INTERVAL_INTS;
  const int fi = iv[2];
  if (fi < 0 || fi >= n_files) return;                                    // no file to blame: nothing read, nothing written
  int st;
  if (set < 0 || files[(long)fi * FILE_INTS + F_TABLE_SET] != set) st = BAD_ARGS;
  else st = decode_interval(blob, blob_bytes, iv, files, n_files, n_sets, s_set, coef, total_blocks);
  if (st != OK) atomicMax(&status[fi], st);                               // the largest code of a file's intervals
}

struct PixelArgs {
  const int16_t* coef;
  long total_blocks;
  const int* files;
  const uint16_t* quant;
  unsigned char* first;
  unsigned char* full;
  int* status;
  int n_quant, H, W, C, tiles_x, n0;
};

// Dequantisation and both passes of the inverse DCT of block `blk`, in registers; the 8 x 8 samples to dst (pitch bytes).
__device__ __forceinline__ void jd_block(const int16_t* __restrict__ coef, long blk, const uint16_t* q, unsigned char* dst,
                                         int pitch) {
  const uint4* src = reinterpret_cast<const uint4*>(coef + blk * 64);
  int ws[64];
#pragma unroll
  for (int v = 0; v < 8; ++v) {
    const uint4 r = src[v];
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = (int)(int16_t)(uint16_t)(w[u >> 1] >> (16 * (u & 1)));
      ws[v * 8 + u] = c * (int)q[v * 8 + u];
    }
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {                                            // columns
    int x[8], o[8];
#pragma unroll
    for (int v = 0; v < 8; ++v) x[v] = ws[v * 8 + u];
    idct_1d(x, o, 11);
#pragma unroll
    for (int v = 0; v < 8; ++v) ws[v * 8 + u] = o[v];
  }
#pragma unroll
  for (int y = 0; y < 8; ++y) {                                            // rows
    int o[8];
    idct_1d(&ws[y * 8], o, 18);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      lo |= (uint32_t)clamp255(o[x] + 128) << (8 * x);
      hi |= (uint32_t)clamp255(o[x + 4] + 128) << (8 * x);
    }
    uint32_t* d = reinterpret_cast<uint32_t*>(dst + y * pitch);            // 8-byte aligned: pitch % 8 == 0
    d[0] = lo;
    d[1] = hi;
  }
}

__global__ __launch_bounds__(PX_T) void jpeg_pixels_kernel(const PixelArgs a) {
  __shared__ __align__(16) unsigned char s_plane[3][PX_PLANE];
  __shared__ uint16_t s_q[3][64];
  const int tid = threadIdx.x;
  const long n = (long)a.n0 + blockIdx.y;
  if (a.status[n] != 0) return;                                            // (uniform) rejected by the entropy decoder
  const int* f = a.files + n * FILE_INTS;
  const int nc = f[F_COMPONENTS], hs = f[F_HS], vs = f[F_VS], mw = f[F_MCU_W], mh = f[F_MCU_H];
  bool ok = file_ok(f, 1 << 30, a.total_blocks);                           // (the table set is not used here)
  if (ok) {
    ok = mw == (a.W + 8 * hs - 1) / (8 * hs) && mh == (a.H + 8 * vs - 1) / (8 * vs) && (!a.full || a.C == nc);
    for (int c = 0; c < nc; ++c) ok = ok && f[F_QUANT + c] >= 0 && f[F_QUANT + c] < a.n_quant;
  }
  if (!ok) {                                                               // (uniform)
    if (tid == 0) atomicMax(&a.status[n], (int)BAD_ARGS);                  // (every tile of the file says the same)
    return;
  }
  if (tid < nc * 64) s_q[tid >> 6][tid & 63] = a.quant[(long)f[F_QUANT + (tid >> 6)] * 64 + (tid & 63)];
  __syncthreads();

  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const int y0 = ty * PX_TILE_H, x0 = tx * PX_TILE_W;
  // the chroma planes: origin (in blocks of the component's grid), size in blocks, pitch; Y: (y0 / 8, x0 / 8), 4 x 16
  const int cby0 = vs == 2 ? y0 / 16 - 1 : y0 / 8, cbx0 = hs == 2 ? x0 / 16 - 1 : x0 / 8;
  const int cnbx = hs == 2 ? 10 : 16, cpitch = cnbx * 8;
  const int ybw = mw * hs, ybh = mh * vs;
  const long luma_blocks = (long)ybw * ybh, chroma_blocks = (long)mw * mh;
  const int ny = 4 * 16, ncj = 4 * cnbx;
  const int c_lo = a.full ? 1 : 2;                                         // `first` is R: Y and Cr
  const int jobs = ny + (nc == 3 ? (3 - c_lo) * ncj : 0);
  for (int job = tid; job < jobs; job += PX_T) {
    int c, by, bx, gby, gbx, bw, bh, pitch;
    long base = f[F_BLOCK0];
    if (job < ny) {
      c = 0; by = job >> 4; bx = job & 15; gby = y0 / 8 + by; gbx = x0 / 8 + bx; bw = ybw; bh = ybh; pitch = PX_TILE_W;
    } else {
      const int j = job - ny;
      c = c_lo + j / ncj;
      const int r = j % ncj;
      by = r / cnbx; bx = r % cnbx; gby = cby0 + by; gbx = cbx0 + bx; bw = mw; bh = mh; pitch = cpitch;
      base += luma_blocks + (c - 1) * chroma_blocks;
    }
    if (gby < 0 || gby >= bh || gbx < 0 || gbx >= bw) continue;            // outside the component: never fetched below
    jd_block(a.coef, base + (long)gby * bw + gbx, s_q[c], &s_plane[c][(by * 8) * pitch + bx * 8], pitch);
  }
  __syncthreads();

  const int dw = (a.W + hs - 1) / hs, dh = (a.H + vs - 1) / vs;
  const int cy0 = cby0 * 8, cx0 = cbx0 * 8;
  for (int g = tid; g < PX_TILE_H * (PX_TILE_W / 4); g += PX_T) {
    const int row = g / (PX_TILE_W / 4), xg = (g % (PX_TILE_W / 4)) * 4;
    const int y = y0 + row, x = x0 + xg;
    if (y >= a.H || x >= a.W) continue;
    const int cnt = min(4, a.W - x);
    unsigned r[4], gr[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xx = min(x + k, a.W - 1);
      const int Y = s_plane[0][row * PX_TILE_W + (xx - x0)];
      if (nc == 1) {
        r[k] = (unsigned)Y;
        continue;
      }
      const unsigned char* p2 = s_plane[2];
      const int cr = chroma_at([&](int rr, int cc) { return (int)p2[(rr - cy0) * cpitch + (cc - cx0)]; }, hs, vs, y, xx, dh,
                               dw) - 128;
      r[k] = (unsigned)red_of(Y, cr);
      if (a.full) {
        const unsigned char* p1 = s_plane[1];
        const int cb = chroma_at([&](int rr, int cc) { return (int)p1[(rr - cy0) * cpitch + (cc - cx0)]; }, hs, vs, y, xx,
                                 dh, dw) - 128;
        gr[k] = (unsigned)green_of(Y, cb, cr);
        b[k] = (unsigned)blue_of(Y, cb);
      }
    }
    const long px = (n * a.H + y) * (long)a.W + x;
    if (a.first) {
      unsigned char* p = a.first + px;
      if (cnt == 4 && ((uintptr_t)p & 3) == 0) put4(p, r[0], r[1], r[2], r[3]);
      else
        for (int k = 0; k < cnt; ++k) put1(p + k, r[k]);
    }
    if (a.full && nc == 1) {
      unsigned char* p = a.full + px;
      if (cnt == 4 && ((uintptr_t)p & 3) == 0) put4(p, r[0], r[1], r[2], r[3]);
      else
        for (int k = 0; k < cnt; ++k) put1(p + k, r[k]);
    } else if (a.full) {
      unsigned char* p = a.full + px * 3;
      if (cnt == 4 && ((uintptr_t)p & 3) == 0) {
        put4(p, r[0], gr[0], b[0], r[1]);
        put4(p + 4, gr[1], b[1], r[2], gr[2]);
        put4(p + 8, b[2], r[3], gr[3], b[3]);
      } else {
        for (int k = 0; k < cnt; ++k) {
          put1(p + 3 * k, r[k]);
          put1(p + 3 * k + 1, gr[k]);
          put1(p + 3 * k + 2, b[k]);
        }
      }
    }
  }
}

}  // namespace

extern "C" int spnet_jpeg_entropy(const unsigned char* blob, long blob_bytes, const int* intervals, int n_intervals,
                                  const int* files, int n_files, const uint32_t* tables, int n_sets, int16_t* coef,
                                  long total_blocks, int* status, void* stream) {
  if (n_intervals < 0 || n_files < 0 || n_sets < 0 || blob_bytes < 0 || blob_bytes > JPEG_MAX_BLOB || total_blocks < 0 ||
      total_blocks > JPEG_MAX_BLOCKS)
    return (int)hipErrorInvalidValue;
  if (n_files == 0) return 0;
  if (!blob || !intervals || !files || !tables || !coef || !status) return (int)hipErrorInvalidValue;
  if (((uintptr_t)intervals & 3) || ((uintptr_t)files & 3) || ((uintptr_t)tables & 3) || ((uintptr_t)status & 3) ||
      ((uintptr_t)coef & 15))
    return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)n_files, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  if (n_intervals == 0) return 0;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)spnet_cdiv(n_intervals, SPNET_WAVE)), dim3(SPNET_WAVE), 0,
                     (hipStream_t)stream, blob, blob_bytes, intervals, n_intervals, files, n_files, tables, n_sets, coef,
                     total_blocks, status);
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_jpeg_pixels(const int16_t* coef, long total_blocks, const int* files, int n_files, const uint16_t* quant,
                                 int n_quant, int H, int W, int channels, unsigned char* first, unsigned char* all, int* status,
                                 void* stream) {
  if (n_files < 0 || n_quant < 0 || H < 1 || W < 1 || H > JD_MAX_DIM || W > JD_MAX_DIM || total_blocks < 0 ||
      total_blocks > JPEG_MAX_BLOCKS || (channels != 1 && channels != 3))
    return (int)hipErrorInvalidValue;
  if (n_files == 0) return 0;
  if (!coef || !files || !quant || !status || (!first && !all)) return (int)hipErrorInvalidValue;
  if (((uintptr_t)coef & 15) || ((uintptr_t)files & 3) || ((uintptr_t)quant & 1) || ((uintptr_t)status & 3))
    return (int)hipErrorInvalidValue;
  PixelArgs a = {};
  a.coef = coef; a.total_blocks = total_blocks; a.files = files; a.quant = quant; a.first = first; a.full = all;
  a.status = status; a.n_quant = n_quant; a.H = H; a.W = W; a.C = channels;
  a.tiles_x = spnet_cdiv(W, PX_TILE_W);
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)spnet_cdiv(H, PX_TILE_H);          // <= 512 * 2048
  spnet_for_grid_chunks(n_files, [&](int n0, int cnt) {
    a.n0 = n0;
    hipLaunchKernelGGL(jpeg_pixels_kernel, dim3(tiles, (unsigned)cnt), dim3(PX_T), 0, (hipStream_t)stream, a);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}
