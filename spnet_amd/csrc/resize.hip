// PIL.Image.resize((OW, OH), ANTIALIAS) of N one-channel uint8 frames, bit-identical (spnet/utils.py:335-337): Pillow's
// 8-bit resampler is integer arithmetic once the taps exist -- out = clip((2^21 + sum_j pixel[lo + j] * k[j]) >> 22) with
// an int32 accumulator, horizontally first, then vertically over the uint8 result of the first pass.  The int32 taps
// come from the host (spnet_amd/resize.py, float64 as Pillow computes them); nothing here depends on float rounding
// except the optional network-input output, which is spnet_u8_to_input's arithmetic.
//
// One launch for the batch.  A workgroup owns one frame's tile of TH output rows x TW output columns (TW = the whole row
// up to 512 columns, so row bands overlap by the vertical support only):
//   stage   the source rows the band needs -> LDS, 16 aligned bytes per lane (each row lands at its memory address
//           modulo 16, so no alignment is asked of W, of a frame's first byte or of the buffer)
//   pass 1  horizontal: a lane owns one dword (4 neighbouring columns) of an intermediate row -> LDS, never HBM
//   pass 2  vertical: a lane owns the same dword column of RPT output rows, int32 accumulators in registers
//   store   the tile's bytes go through LDS once more so that lanes own ALIGNED groups of 4 output elements: one dword of
//           out_u8 and / or one float4 of out_f per lane (rows of 331 elements start at any alignment)
// A band that needs more source rows than fit in LDS (strong reductions) runs stage / pass 1 / pass 2 over chunks of
// rows; the accumulators carry over.  Tables are clamped to the staged ranges: a table that is not lanczos_taps' of the
// size pair gives wrong or unwritten pixels, never an out-of-range access.
#include "common.h"
#include "u8_tile.h"

// Diagnostic builds only (tools/resize_time.py --knockouts builds and times them through tools/build_variant_lib.sh and
// SPNET_HIP_LIB): knock-outs that say where the launch's time goes.  The results are wrong by design; the product
// library is built without the macro.  1: the stage loads nothing from HBM; 2: nothing is stored to HBM; 4: pass 1 does
// one tap per output; 8: pass 2 does one tap per output; 16: the network-input conversion is a plain int -> float.
#ifndef SPNET_RESIZE_KO
#define SPNET_RESIZE_KO 0
#endif

namespace {

constexpr int KO = SPNET_RESIZE_KO;
constexpr int RPT = 8;                 // output rows per lane in the vertical pass
constexpr int PREC = 22;               // Pillow's PRECISION_BITS for 8-bit channels
constexpr int XT_REG = 12;             // horizontal taps kept in registers up to this count (512 -> 331 has 10)
constexpr int LDS_BAND_BYTES = 48 * 1024;

struct ResizeArgs {
  const unsigned char* src;
  const int* xtab;
  const int* ytab;
  unsigned char* out_u8;
  float* out_f;
  long src_bytes;
  int N, H, W, OH, OW;
  int xtaps, ytaps;       // 0: that pass is skipped (size unchanged)
  int TW, TWD, nct;       // tile width in columns / dwords, column tiles per row
  int nrg, TH, nrb;       // row groups of the vertical pass, tile height = nrg * RPT, row bands per frame
  int RC, ps, pm;         // source rows per chunk, LDS pitches in bytes of the source rows / of the dword rows
  int maxseg;             // bound of the source columns one tile needs
};

// (first input index, tap count) of output o, clamped to the axis; an unchanged axis is the identity
__device__ __forceinline__ void tab_entry(const int* __restrict__ tab, int taps, int I, int o, int& lo, int& cnt) {
  if (taps == 0) { lo = o; cnt = 1; return; }
  const int* e = tab + (long)o * (taps + 2);
  lo = min(max(e[0], 0), I - 1);
  cnt = min(min(max(e[1], 0), taps), I - lo);
}
__device__ __forceinline__ int tab_tap(const int* __restrict__ tab, int taps, int o, int t) {
  return taps == 0 ? (1 << PREC) : tab[(long)o * (taps + 2) + 2 + t];
}
// pixel * tap with 24-bit operands (|tap| < 2^23: checked where the tables are made); sums wrap like Pillow's C int
__device__ __forceinline__ unsigned mac(unsigned acc, unsigned pixel, int k) { return acc + (unsigned)__mul24((int)pixel, k); }
// clip((acc + 2^21) >> 22, 0, 255), clamped BEFORE the shift (the same value).  Observation, not root-caused: written as
// shift-then-clamp, hipcc of ROCm 7.2 (clang 22.0.0git roc-7.2.0) packs two neighbouring bytes with v_ashr_pk_u8_i32
// and ORs bytes 2 and 3 into that register, and on the MI355X bytes 2 and 3 of every packed dword were then wrong
// (bytes 0 and 1 right).  In this form the instruction is not selected; tests/test_resize_gpu.py catches the other.
__device__ __forceinline__ unsigned finish(unsigned acc) {
  const int v = (int)(acc + (1u << (PREC - 1)));
  return (unsigned)(min(max(v, 0), (256 << PREC) - 1) >> PREC);
}

template <int XT>
__global__ __launch_bounds__(256) void resize_u8_kernel(const ResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char* s_src = smem;                                            // [RC][ps]
  unsigned* s_mid = reinterpret_cast<unsigned*>(smem + (size_t)a.RC * a.ps);   // [RC][pm / 4]
  const int pmd = a.pm >> 2;
  unsigned* s_out = s_mid + (size_t)a.RC * pmd;                           // [TH][pm / 4]
  const int tid = threadIdx.x;
  int bid = blockIdx.x;
  const int ct = bid % a.nct;
  bid /= a.nct;
  const int rb = bid % a.nrb;
  const int n = bid / a.nrb;
  const int c0 = ct * a.TW, tw = min(a.OW, c0 + a.TW) - c0;
  const int r0 = rb * a.TH, nro = min(a.OH, r0 + a.TH) - r0;

  // source columns / rows of this tile (first index and count rise with the output index)
  int sc0, sr0, lo, cnt;
  tab_entry(a.xtab, a.xtaps, a.W, c0, sc0, cnt);
  tab_entry(a.xtab, a.xtaps, a.W, c0 + tw - 1, lo, cnt);
  const int seg = lo + cnt - sc0;
  tab_entry(a.ytab, a.ytaps, a.H, r0, sr0, cnt);
  tab_entry(a.ytab, a.ytaps, a.H, r0 + nro - 1, lo, cnt);
  const int sr1 = lo + cnt;
  if (seg < 1 || seg > a.maxseg || sr1 <= sr0) return;                    // not a table of this size pair

  // this lane's dword column: 4 output columns, their taps (pass 1) and its output rows (pass 2)
  const int dc = tid % a.TWD, rg = tid / a.TWD;
  const int hrg = 256 / a.TWD;                                            // row groups of pass 1 (>= 2)
  int xlo[4], xcnt[4], xk[4][XT > 0 ? XT : 1];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = dc * 4 + i;
    xlo[i] = 0;
    xcnt[i] = 0;
    if (c < tw) {
      tab_entry(a.xtab, a.xtaps, a.W, c0 + c, lo, cnt);
      xlo[i] = min(max(lo - sc0, 0), seg - 1);
      xcnt[i] = min(cnt, seg - xlo[i]);
    }
#pragma unroll
    for (int t = 0; t < XT; ++t) xk[i][t] = t < xcnt[i] ? tab_tap(a.xtab, a.xtaps, c0 + c, t) : 0;
  }
  unsigned acc[RPT][4];
#pragma unroll
  for (int j = 0; j < RPT; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[j][i] = 0u;

  const int sb = (int)((uintptr_t)a.src & 15);                            // the staged rows are aligned in MEMORY: byte b of the
  const unsigned char* src16 = a.src - sb;                                // source is byte sb + b past a 16-byte boundary
  const long frame = (long)n * a.H * a.W + sb;
  const int nch = (seg + 30) >> 4;                                        // 16-byte pieces per staged row, at most
  for (int cr0 = sr0; cr0 < sr1; cr0 += a.RC) {
    const int nr = min(a.RC, sr1 - cr0);
    __syncthreads();                                                      // (the previous chunk's pass 2 has read s_mid)
    // ---- stage: source rows cr0 .. cr0 + nr, columns sc0 .. sc0 + seg, each row at its global address modulo 16
    for (int i = tid; i < nr * nch; i += 256) {
      const int row = i / nch, c = i - row * nch;
      const long g = frame + (long)(cr0 + row) * a.W + sc0;
      const int off = (int)(g & 15);
      if (c * 16 >= off + seg) continue;
      const long b = g - off + (long)c * 16;
      uint4 q;
      if ((KO & 1) && a.N > 0) {
        q = make_uint4((unsigned)b, 0x55aa55aau, (unsigned)i, 0x0f0f0f0fu);
      } else if (b >= sb && b + 16 <= sb + a.src_bytes) {
        q = *reinterpret_cast<const uint4*>(src16 + b);
      } else {                                                            // the first / last bytes of the source
        unsigned w[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < 16; ++k)
          if (b + k >= sb && b + k < sb + a.src_bytes) w[k >> 2] |= (unsigned)src16[b + k] << ((k & 3) * 8);
        q = make_uint4(w[0], w[1], w[2], w[3]);
      }
      *reinterpret_cast<uint4*>(s_src + (size_t)row * a.ps + c * 16) = q;
    }
    __syncthreads();
    // ---- pass 1: horizontal, one dword of the intermediate row per lane
    if (rg < hrg) {
      for (int row = rg; row < nr; row += hrg) {
        const int off = (int)((frame + (long)(cr0 + row) * a.W + sc0) & 15);
        const unsigned char* p = s_src + (size_t)row * a.ps + off;
        unsigned packed = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          unsigned s = 0u;
          if (XT > 0) {
#pragma unroll
            for (int t = 0; t < ((KO & 4) ? 1 : XT); ++t) s = mac(s, p[xlo[i] + t], xk[i][t]);     // (taps past the count are 0; the row
          } else {                                                                //  pitch covers the XT bytes read)
            for (int t = 0; t < xcnt[i]; ++t) s = mac(s, p[xlo[i] + t], tab_tap(a.xtab, a.xtaps, c0 + dc * 4 + i, t));
          }
          packed |= finish(s) << (8 * i);               // (an unchanged width: one tap of 2^22, the pixel itself)
        }
        s_mid[(size_t)row * pmd + dc] = packed;
      }
    }
    __syncthreads();
    // ---- pass 2: vertical, the taps of this chunk's rows
    if (rg < a.nrg) {
#pragma unroll
      for (int j = 0; j < RPT; ++j) {
        const int orow = rg * RPT + j;
        if (orow < nro) {
          tab_entry(a.ytab, a.ytaps, a.H, r0 + orow, lo, cnt);
          const int t0 = max(lo, cr0), t1 = (KO & 8) ? min(t0 + 1, cr0 + nr) : min(lo + cnt, cr0 + nr);
          for (int r = t0; r < t1; ++r) {
            const int k = tab_tap(a.ytab, a.ytaps, r0 + orow, r - lo);
            const unsigned w = s_mid[(size_t)(r - cr0) * pmd + dc];
            acc[j][0] = mac(acc[j][0], w & 0xffu, k);
            acc[j][1] = mac(acc[j][1], (w >> 8) & 0xffu, k);
            acc[j][2] = mac(acc[j][2], (w >> 16) & 0xffu, k);
            acc[j][3] = mac(acc[j][3], w >> 24, k);
          }
        }
      }
    }
  }
  // ---- the tile's bytes -> LDS (an unchanged height: the accumulator holds pixel << 22 exactly, and so does Pillow's copy)
  if (rg < a.nrg) {
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      const int orow = rg * RPT + j;
      if (orow < nro)
        s_out[(size_t)orow * pmd + dc] = finish(acc[j][0]) | (finish(acc[j][1]) << 8) | (finish(acc[j][2]) << 16) |
                                         (finish(acc[j][3]) << 24);
    }
  }
  __syncthreads();
  // ---- store: a lane owns 4 elements of the output that share an aligned dword (out_u8) / float4 (out_f) IN MEMORY,
  // clipped to the tile's row
  const unsigned char* so = reinterpret_cast<const unsigned char*>(s_out);
  const long row0 = ((long)n * a.OH + r0) * a.OW + c0;                    // the tile's first element
  if ((KO & 2) && a.N > 0 && so[tid] != 77) return;                       // (keeps the work above alive)
  if (a.out_u8) store_tile<unsigned char>(a.out_u8, so, a.pm, row0, a.OW, nro, tw, a.TWD + 1, tid);
  if (a.out_f) store_tile<float, (KO & 16) != 0>(a.out_f, so, a.pm, row0, a.OW, nro, tw, a.TWD + 1, tid);
}

}  // namespace

extern "C" int spnet_resize_u8(const unsigned char* src, int N, int H, int W, const int* xtab, int xtaps, const int* ytab,
                               int ytaps, int OH, int OW, unsigned char* out_u8, float* out_f, void* stream) {
  const int LIM = 2048;
  if (!src || N < 0 || H < 1 || W < 1 || OH < 1 || OW < 1 || H > LIM || W > LIM || OH > LIM || OW > LIM) return (int)hipErrorInvalidValue;
  if (!out_u8 && !out_f) return (int)hipErrorInvalidValue;
  if ((((uintptr_t)out_f | (uintptr_t)xtab | (uintptr_t)ytab) & 3)) return (int)hipErrorInvalidValue;
  // a pass exists exactly when its size changes (Pillow skips the other one), and then it needs its table
  if (OW == W) xtaps = 0;
  else if (!xtab || xtaps < 1 || xtaps > W) return (int)hipErrorInvalidValue;
  if (OH == H) ytaps = 0;
  else if (!ytab || ytaps < 1 || ytaps > H) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;

  ResizeArgs a;
  a.src = src; a.xtab = xtab; a.ytab = ytab; a.out_u8 = out_u8; a.out_f = out_f;
  a.src_bytes = (long)N * H * W;
  a.N = N; a.H = H; a.W = W; a.OH = OH; a.OW = OW; a.xtaps = xtaps; a.ytaps = ytaps;
  a.nct = spnet_cdiv(OW, 512);
  a.TW = spnet_cdiv(spnet_cdiv(OW, a.nct), 4) * 4;
  a.TWD = a.TW / 4;                                                       // <= 128
  const int nrg_max = 256 / a.TWD;
  a.nrg = nrg_max < spnet_cdiv(OH, RPT) ? nrg_max : spnet_cdiv(OH, RPT);
  a.TH = a.nrg * RPT;
  a.nrb = spnet_cdiv(OH, a.TH);
  // source extent of a tile: (count - 1) * scale + 2 * support + 1 indices, Pillow's window arithmetic
  const double xs = (double)W / OW, ys = (double)H / OH;
  const double xsup = 3.0 * (xs > 1.0 ? xs : 1.0), ysup = 3.0 * (ys > 1.0 ? ys : 1.0);
  long mseg = xtaps ? (long)(a.TW * xs + 2.0 * xsup) + 4 : a.TW;
  if (mseg > W) mseg = W;
  long mrow = ytaps ? (long)(a.TH * ys + 2.0 * ysup) + 4 : a.TH;
  if (mrow > H) mrow = H;
  a.maxseg = (int)mseg;
  a.ps = ((a.maxseg + 30) / 16) * 16 + 16;                                // 15 bytes of misalignment + XT_REG of over-read
  a.pm = a.TWD * 4 + 4;                                                   // one dword of padding per row
  long rc = LDS_BAND_BYTES / (a.ps + a.pm);
  if (rc > mrow) rc = mrow;
  if (rc < 1) return (int)hipErrorInvalidValue;
  a.RC = (int)rc;
  const size_t lds = (size_t)a.RC * (a.ps + a.pm) + (size_t)a.TH * a.pm;  // <= 48 KiB + 16 KiB
  if (lds > 64 * 1024) return (int)hipErrorInvalidValue;
  const long blocks = (long)N * a.nrb * a.nct;
  if (blocks > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  if (xtaps > 0 && xtaps <= XT_REG)
    hipLaunchKernelGGL(resize_u8_kernel<XT_REG>, dim3((unsigned)blocks), dim3(256), lds, st, a);
  else
    hipLaunchKernelGGL(resize_u8_kernel<0>, dim3((unsigned)blocks), dim3(256), lds, st, a);
  SPNET_RETURN_LAUNCH_STATUS();
}
