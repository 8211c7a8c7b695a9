// Band-pass mix-up (spnet/augmentation.py:10-62): the lowest spatial frequencies of a fake-ESPI frame are replaced by
// those of a real ESPI frame, s * T[k,l] for the 16 x 16 window k, l in [-8, 8) of the centred spectrum, followed by the
// complex magnitude and a min-max normalisation to [0, 255].
//
// No FFT: only 256 coefficients change, so with G = s*T - F over the window
//   y[r][c] = f[r][c] + 1/(H*W) * sum_{k,l} G[k][l] * exp(+2 pi i (k r / H + l c / W))
// and every step is a separable, windowed DFT:
//   projection      F[k][l] = sum_r exp(-2 pi i k r / H) * sum_c f[r][c] exp(-2 pi i l c / W)
//                   (per row block: the 16 row sums of every column, then the 16 column sums of those; one partial
//                   window per row block, summed in block order by the finish kernel)
//   reconstruction  Q[r][l] = sum_k G[k][l] exp(+2 pi i k r / H); y[r][c] = f[r][c] + sum_l Q[r][l] exp(+2 pi i l c / W)
// The fake frame is projected CENTRED, d = f - f[0][0]: the constant's DC coefficient lies inside the window, so it
// cancels out of y exactly (y = d + sum G' ..., G' = s*T - F_d), and a constant frame gives d = 0, F_d = 0 and, with
// s = 0, y = 0 exactly -- the all-zero image the reference's normalisation makes of a constant.
//
// Twiddles come from an exact integer phase j = (k*r) mod H or (l*c) mod W into cos / sin(2 pi j / n) evaluated in double
// and rounded to fp32.  Every sum runs in a fixed order, no atomics: a frame's bits depend on that frame, its window
// row and its s only, not on its position in the batch.
//
// Frames are [N][H][W], row-major, single channel.  x_kind: 0 uint8, 1 fp32 pixel units (0..255), 2 fp32 network units
// ([-1,1], pixel = (x/2 + 1/2) * 255).
#include "common.h"

#define BP_RB 64          // rows per block
#define BP_TPB 256        // threads per block = columns per column tile = 16 x 16 window
#define BP_CB_LD 257      // padded row of the column-sum buffer (two window rows of one half-wave on different banks)
#define BP_MAX_DIM 2048

static inline int bp_blocks(int H) { return (H + BP_RB - 1) / BP_RB; }

__device__ __forceinline__ float2 bp_twiddle(int j, int n) {     // (cos, sin)(2 pi j / n), j in [0, n)
  double s, c;
  sincospi(2.0 * (double)j / (double)n, &s, &c);
  return make_float2((float)c, (float)s);
}

__device__ __forceinline__ int bp_mod(long a, int n) {
  long r = a % n;
  return (int)(r < 0 ? r + n : r);
}

template <int KIND>
__device__ __forceinline__ float bp_pixel(const void* __restrict__ x, long i) {
  // Products written here, under contract(off): __fmul_rn is a plain product in a header, which the caller's
  // `pixel - p0` fuses with into one FMA -- the centred value is then not that of the rounded pixel, and x_kind 2 differs
  // from x_kind 1 on the same pixels.
#pragma clang fp contract(off)
  if (KIND == 0) return (float)static_cast<const unsigned char*>(x)[i];
  const float v = static_cast<const float*>(x)[i];
  if (KIND == 1) return v;
  return (v * 0.5f + 0.5f) * 255.f;
}

__device__ __forceinline__ int bp_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// partial[m][b][k][l] (complex): the window of rows [b*BP_RB, (b+1)*BP_RB) of frame m.  flip (or NULL): cv2.flip code
// per frame (0 rows, 1 columns, -1 both, anything else none), applied by index mapping.  center: project f - f[0][0].
template <int KIND>
__global__ __launch_bounds__(BP_TPB) void bp_project_kernel(const void* __restrict__ x, const int* __restrict__ sel,
                                                            int n_src, const int* __restrict__ flip, int center, int H,
                                                            int W, float2* __restrict__ partial,
                                                            float* __restrict__ p0buf) {
  extern __shared__ float2 bp_lds[];
  float2* twW = bp_lds;                 // [W]          (cos, sin)(2 pi j / W)
  float2* twH = twW + W;                // [BP_RB][16]  exp(-2 pi i k r / H)
  float2* cb = twH + BP_RB * 16;        // [16][BP_CB_LD] column sums of this column tile
  const int m = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, nb = gridDim.x;
  const int r0 = b * BP_RB, nr = min(BP_RB, H - r0);
  const long hw = (long)H * W;
  const long src = sel ? bp_clamp(sel[m], n_src) : m;
  const int fc = flip ? flip[m] : 2;
  const bool frow = fc == 0 || fc == -1, fcol = fc == 1 || fc == -1;
  const void* frame = KIND == 0 ? (const void*)(static_cast<const unsigned char*>(x) + src * hw)
                                : (const void*)(static_cast<const float*>(x) + src * hw);
  const float p0 = center ? bp_pixel<KIND>(frame, 0) : 0.f;
  if (p0buf && b == 0 && tid == 0) p0buf[m] = p0;
  for (int j = tid; j < W; j += BP_TPB) twW[j] = bp_twiddle(j, W);
  for (int i = tid; i < BP_RB * 16; i += BP_TPB) {
    const float2 t = bp_twiddle(bp_mod((long)((i & 15) - 8) * (r0 + (i >> 4)), H), H);
    twH[i] = make_float2(t.x, -t.y);
  }
  __syncthreads();
  const int kk = tid >> 4, ll = tid & 15;
  const int lstep = ll - 8 + W;          // (l mod W), l = ll - 8, W >= 16
  float accr = 0.f, acci = 0.f;
  for (int c0 = 0; c0 < W; c0 += BP_TPB) {
    const int c = c0 + tid;
    if (c < W) {
      float ar[16], ai[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) ar[q] = ai[q] = 0.f;
      const long cs = fcol ? W - 1 - c : c;
      for (int rl = 0; rl < nr; ++rl) {
        const int r = r0 + rl;
        const long rs = frow ? H - 1 - r : r;
        const float v = bp_pixel<KIND>(frame, rs * W + cs) - p0;
        const float2* t = twH + rl * 16;
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const float2 w = t[q];
          ar[q] += v * w.x;
          ai[q] += v * w.y;
        }
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) cb[q * BP_CB_LD + tid] = make_float2(ar[q], ai[q]);
    }
    __syncthreads();
    // (kk, ll): sum over this tile's columns of cb[kk][c] * exp(-2 pi i l c / W), phase j = (l * c) mod W
    const int cw = min(BP_TPB, W - c0);
    int j = bp_mod((long)lstep * c0, W);
    float tr = 0.f, ti = 0.f;
    const float2* row = cb + kk * BP_CB_LD;
    for (int cl = 0; cl < cw; ++cl) {
      const float2 v = row[cl], w = twW[j];
      tr += v.x * w.x + v.y * w.y;
      ti += v.y * w.x - v.x * w.y;
      j += lstep;
      j -= j >= W ? W : 0;
      j -= j >= W ? W : 0;
    }
    accr += tr;
    acci += ti;
    __syncthreads();
  }
  partial[((long)m * nb + b) * 256 + tid] = make_float2(accr, acci);
}

// Window of frame m = the row-block partials summed in block order.  table == NULL: win[m] = F.  Otherwise
// win[m] = (s[m] * table[row[m]] - F) / (H*W), the G of the reconstruction.
__global__ __launch_bounds__(256) void bp_finish_kernel(const float2* __restrict__ partial, int nb,
                                                        const float2* __restrict__ table, int n_table,
                                                        const int* __restrict__ row, const float* __restrict__ s,
                                                        float inv_hw, float2* __restrict__ win) {
  const int m = blockIdx.x, tid = threadIdx.x;
  float fr = 0.f, fi = 0.f;
  for (int b = 0; b < nb; ++b) {
    const float2 p = partial[((long)m * nb + b) * 256 + tid];
    fr += p.x;
    fi += p.y;
  }
  if (table) {
    const float2 t = table[(long)bp_clamp(row[m], n_table) * 256 + tid];
    const float sv = s[m];
    fr = __fmul_rn(__fsub_rn(__fmul_rn(sv, t.x), fr), inv_hw);
    fi = __fmul_rn(__fsub_rn(__fmul_rn(sv, t.y), fi), inv_hw);
  }
  win[(long)m * 256 + tid] = make_float2(fr, fi);
}

// PASS 0: per row block min / max of |y| -> mm[m][b].  PASS 1: the frame's min / max from mm, |y| recomputed and
// normalised to [0, 255] (cv2.normalize NORM_MINMAX, then np.clip) -> out_f (f_kind 0: pixel units, 1: [-1,1]) and / or
// out_u8 (round to nearest even, saturate).
template <int KIND, int PASS>
__global__ __launch_bounds__(BP_TPB) void bp_recon_kernel(const void* __restrict__ x, const int* __restrict__ sel,
                                                          int n_src, int H, int W, const float2* __restrict__ G,
                                                          const float* __restrict__ p0buf, float2* __restrict__ mm, float* __restrict__ out_f, int f_kind,
                                                          unsigned char* __restrict__ out_u8) {
  extern __shared__ float2 bp_lds[];
  float2* twW = bp_lds;                 // [W]
  float2* twH = twW + W;                // [BP_RB][16]  exp(+2 pi i k r / H)
  float2* q = twH + BP_RB * 16;         // [BP_RB][16]  Q[r][l]
  float2* g = q + BP_RB * 16;           // [16][16]
  __shared__ float red[2][BP_TPB / 64];
  const int m = blockIdx.y, b = blockIdx.x, tid = threadIdx.x, nb = gridDim.x;
  const int r0 = b * BP_RB, nr = min(BP_RB, H - r0);
  const long hw = (long)H * W;
  const long src = sel ? bp_clamp(sel[m], n_src) : m;
  const void* frame = KIND == 0 ? (const void*)(static_cast<const unsigned char*>(x) + src * hw)
                                : (const void*)(static_cast<const float*>(x) + src * hw);
  // the centring offset as the projection read it: in place (out_f == x) another block of this frame may already have
  // overwritten pixel 0
  const float p0 = p0buf[m];
  for (int j = tid; j < W; j += BP_TPB) twW[j] = bp_twiddle(j, W);
  for (int i = tid; i < BP_RB * 16; i += BP_TPB)
    twH[i] = bp_twiddle(bp_mod((long)((i & 15) - 8) * (r0 + (i >> 4)), H), H);
  g[tid] = G[(long)m * 256 + tid];
  __syncthreads();
  for (int i = tid; i < nr * 16; i += BP_TPB) {
    const int rl = i >> 4, ll = i & 15;
    float qr = 0.f, qi = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const float2 a = g[kk * 16 + ll], w = twH[rl * 16 + kk];
      qr += a.x * w.x - a.y * w.y;
      qi += a.x * w.y + a.y * w.x;
    }
    q[i] = make_float2(qr, qi);
  }
  __syncthreads();
  float mn = 0.f, scale = 0.f;
  if (PASS == 1) {
    float lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < nb; ++k) {
      const float2 v = mm[(long)m * nb + k];
      lo = fminf(lo, v.x);
      hi = fmaxf(hi, v.y);
    }
    mn = lo;
    const float range = hi - lo;
    scale = (double)range > 2.220446049250313e-16 ? 255.f / range : 0.f;    // cv2.normalize: DBL_EPSILON
  }
  float lmn = INFINITY, lmx = -INFINITY;
  for (int c = tid; c < W; c += BP_TPB) {
    float2 w[16];
    int j = bp_mod(-8L * c, W);
#pragma unroll
    for (int ll = 0; ll < 16; ++ll) {
      w[ll] = twW[j];
      j += c;
      j -= j >= W ? W : 0;
    }
    for (int rl = 0; rl < nr; ++rl) {
      const long i = (long)(r0 + rl) * W + c;
      float yr = bp_pixel<KIND>(frame, i) - p0, yi = 0.f;
      const float2* qq = q + rl * 16;
#pragma unroll
      for (int ll = 0; ll < 16; ++ll) {
        const float2 a = qq[ll];
        yr += a.x * w[ll].x - a.y * w[ll].y;
        yi += a.x * w[ll].y + a.y * w[ll].x;
      }
      const float mag = sqrtf(yr * yr + yi * yi);
      if (PASS == 0) {
        lmn = fminf(lmn, mag);
        lmx = fmaxf(lmx, mag);
      } else {
        const float o = fminf(fmaxf(__fmul_rn(__fsub_rn(mag, mn), scale), 0.f), 255.f);
        if (out_f)
          out_f[src * hw + i] = f_kind == 1 ? __fmul_rn(__fsub_rn(__fdiv_rn(o, 255.f), 0.5f), 2.f) : o;
        if (out_u8) out_u8[src * hw + i] = (unsigned char)rintf(o);
      }
    }
  }
  if (PASS == 0) {
    lmn = wave_min(lmn);
    lmx = wave_max(lmx);
    if ((tid & 63) == 0) {
      red[0][tid >> 6] = lmn;
      red[1][tid >> 6] = lmx;
    }
    __syncthreads();
    if (tid == 0) {
      float lo = red[0][0], hi = red[1][0];
      for (int k = 1; k < BP_TPB / 64; ++k) {
        lo = fminf(lo, red[0][k]);
        hi = fmaxf(hi, red[1][k]);
      }
      mm[(long)m * nb + b] = make_float2(lo, hi);
    }
  }
}

static size_t bp_project_lds(int W) { return sizeof(float2) * ((size_t)W + BP_RB * 16 + 16 * BP_CB_LD); }
static size_t bp_recon_lds(int W) { return sizeof(float2) * ((size_t)W + 2 * BP_RB * 16 + 256); }

static bool bp_dims_ok(int N, int H, int W) {
  return N >= 0 && H >= 16 && W >= 16 && H <= BP_MAX_DIM && W <= BP_MAX_DIM;
}

extern "C" long spnet_bandpass_ws(int N, int H, int W) {
  if (!bp_dims_ok(N, H, W)) return -1;
  const long nb = bp_blocks(H);
  return (long)N * (nb * 512 + 512 + nb * 2 + 1);
}

template <int KIND>
static void bp_launch_project(const void* x, const int* sel, int n_src, const int* flip, int center, int N, int H, int W,
                              float2* partial, float* p0buf, hipStream_t st) {
  hipLaunchKernelGGL(bp_project_kernel<KIND>, dim3(bp_blocks(H), N), dim3(BP_TPB), bp_project_lds(W), st, x, sel, n_src,
                     flip, center, H, W, partial, p0buf);
}

extern "C" int spnet_bandpass_project(const void* x, int x_kind, int N, int H, int W, const int* flip, float* win,
                                      float* ws, void* stream) {
  if (!bp_dims_ok(N, H, W) || x_kind < 0 || x_kind > 2 || !x || !win || !ws) return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  float2* partial = reinterpret_cast<float2*>(ws);
  if (x_kind == 0) bp_launch_project<0>(x, nullptr, N, flip, 0, N, H, W, partial, nullptr, st);
  else if (x_kind == 1) bp_launch_project<1>(x, nullptr, N, flip, 0, N, H, W, partial, nullptr, st);
  else bp_launch_project<2>(x, nullptr, N, flip, 0, N, H, W, partial, nullptr, st);
  hipLaunchKernelGGL(bp_finish_kernel, dim3(N), dim3(256), 0, st, partial, bp_blocks(H), nullptr, 0, nullptr, nullptr,
                     0.f, reinterpret_cast<float2*>(win));
  SPNET_RETURN_LAUNCH_STATUS();
}

template <int KIND>
static void bp_launch_apply(const void* x, const int* sel, int n_src, int N, int H, int W, const float2* table,
                            int n_table, const int* row, const float* s, float* out_f, int f_kind, unsigned char* out_u8,
                            float* ws, hipStream_t st) {
  const int nb = bp_blocks(H);
  float2* partial = reinterpret_cast<float2*>(ws);
  float2* G = partial + (long)N * nb * 256;
  float2* mm = G + (long)N * 256;
  float* p0 = reinterpret_cast<float*>(mm + (long)N * nb);
  bp_launch_project<KIND>(x, sel, n_src, nullptr, 1, N, H, W, partial, p0, st);
  hipLaunchKernelGGL(bp_finish_kernel, dim3(N), dim3(256), 0, st, partial, nb, table, n_table, row, s,
                     (float)(1.0 / ((double)H * W)), G);
  hipLaunchKernelGGL((bp_recon_kernel<KIND, 0>), dim3(nb, N), dim3(BP_TPB), bp_recon_lds(W), st, x, sel, n_src, H, W,
                     G, p0, mm, nullptr, 0, nullptr);
  hipLaunchKernelGGL((bp_recon_kernel<KIND, 1>), dim3(nb, N), dim3(BP_TPB), bp_recon_lds(W), st, x, sel, n_src, H, W,
                     G, p0, mm, out_f, f_kind, out_u8);
}

extern "C" int spnet_bandpass_apply(const void* x, int x_kind, const int* sel, int n_src, int N, int H, int W,
                                    const float* table, int n_table, const int* row, const float* s, float* out_f,
                                    int f_kind, unsigned char* out_u8, float* ws, void* stream) {
  if (!bp_dims_ok(N, H, W) || x_kind < 0 || x_kind > 2 || f_kind < 0 || f_kind > 1 || !x || !table || n_table < 1 ||
      !row || !s || !ws || (!out_f && !out_u8) || (sel && n_src < 1))
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  const float2* t = reinterpret_cast<const float2*>(table);
  hipStream_t st = (hipStream_t)stream;
  if (x_kind == 0) bp_launch_apply<0>(x, sel, n_src, N, H, W, t, n_table, row, s, out_f, f_kind, out_u8, ws, st);
  else if (x_kind == 1) bp_launch_apply<1>(x, sel, n_src, N, H, W, t, n_table, row, s, out_f, f_kind, out_u8, ws, st);
  else bp_launch_apply<2>(x, sel, n_src, N, H, W, t, n_table, row, s, out_f, f_kind, out_u8, ws, st);
  SPNET_RETURN_LAUNCH_STATUS();
}
