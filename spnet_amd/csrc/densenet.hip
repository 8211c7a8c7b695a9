// keras.applications.densenet.DenseNet121(include_top=False) (Keras 2.1.3; call site spnet/models.py:357-359 with
// cf.basemodel = 'DenseNet121'): the pieces around the fp32 MFMA GEMMs of gemm.hip.
//
// Every pre-activation BatchNorm of a dense block reads a column prefix [0, c) of the block's Concatenate buffer
// x [M][ldx].  The batch statistics (mean, invstd) of a concat channel are a property of the channel, computed once per
// step; consumer l has its own gamma_l / beta_l (and, in inference, its own moving statistics), so its affine is
// scale = gamma_l*invstd, shift = beta_l - mean*scale.  The consumer's 1x1 convolution applies relu(scale*x + shift) on
// load (spnet_gemm_f32_bnrelu, gemm.hip).  In backward the consumers' BatchNorm backward shares x^ and invstd, so the
// sum over the consumers of a channel is invstd*(G - u/M - x^*v/M) with G = sum_l gamma_l*g_l, u = sum_l gamma_l*sum(g_l),
// v = sum_l gamma_l*sum(g_l*x^): one accumulation per consumer (spnet_dense_consumer_bwd + _fin) and one elementwise pass
// per producer (spnet_dense_producer_fin).  Every reduction runs in a fixed order: identical steps give identical bits.
#include "common.h"

// pixels per partial row of the column sums (spnet_dense_colsums_ld, spnet_dense_consumer_bwd): 64 rows = 16 per thread,
// so that block 1's M = 98,304 pixels at batch 32 spread over 1,536 workgroups (256 rows left the consumer backward
// latency-bound at 384 workgroups: 194 us for c = 224, against 70 us of compulsory traffic)
#define DN_ROWS 64

// ------------------------------------------------------------------ explicit zero padding (ZeroPadding2D)
// backward = 0: out [B][H+pt+pb][W+pl+pr][C] = x zero-padded; backward = 1: out [B][H][W][C] = the interior of
// in [B][H+pt+pb][W+pl+pr][C] (the gradient of the padding).  C % 4 == 0.
__global__ __launch_bounds__(256) void dn_pad_kernel(const float* __restrict__ in, float* __restrict__ out, int Bn, int H,
                                                     int W, int C, int pt, int pl, int PH, int PW, int backward) {
  const int c4n = C >> 2;
  const long total = backward ? (long)Bn * H * W * c4n : (long)Bn * PH * PW * c4n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    long t = i / c4n;
    if (backward) {
      const int w = (int)(t % W);
      t /= W;
      const int h = (int)(t % H);
      const int b = (int)(t / H);
      const long src = (((long)b * PH + h + pt) * PW + w + pl) * C + c4 * 4;
      *reinterpret_cast<float4*>(out + i * 4) = *reinterpret_cast<const float4*>(in + src);
    } else {
      const int pw = (int)(t % PW);
      t /= PW;
      const int ph = (int)(t % PH);
      const int b = (int)(t / PH);
      const int h = ph - pt, w = pw - pl;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (h >= 0 && h < H && w >= 0 && w < W) v = *reinterpret_cast<const float4*>(in + (((long)b * H + h) * W + w) * C + c4 * 4);
      *reinterpret_cast<float4*>(out + i * 4) = v;
    }
  }
}

extern "C" int spnet_pad_nhwc(const float* in, float* out, int B, int H, int W, int C, int pt, int pb, int pl, int pr,
                              int backward, void* stream) {
  if (!in || !out || B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || pt < 0 || pb < 0 || pl < 0 || pr < 0)
    return (int)hipErrorInvalidValue;
  const int PH = H + pt + pb, PW = W + pl + pr;
  const long total = backward ? (long)B * H * W * (C / 4) : (long)B * PH * PW * (C / 4);
  const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
  hipLaunchKernelGGL(dn_pad_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, out, B, H, W, C, pt, pl, PH, PW,
                     backward);
  SPNET_RETURN_LAUNCH_STATUS();
}

// ------------------------------------------------------------------ conv1/conv: ZeroPadding2D(3) + Conv2D(64, 7, 2)
// on the 3-channel stem output.  x [B][H][W][3], w HWIO [7][7][3][64], y [B][OH][OW][64], OH = (H + 6 - 7)/2 + 1.
// Taps are summed in (kh, kw, ci) order -- the order of the patch matrix.
#define DN_CO 64
#define DN_K 147
__global__ __launch_bounds__(256) void dn_conv7_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           float* __restrict__ y, int Bn, int H, int W, int OH, int OW) {
  __shared__ float ws[DN_K * DN_CO];
  for (int i = threadIdx.x; i < DN_K * DN_CO; i += 256) ws[i] = w[i];
  __syncthreads();
  const int co4 = threadIdx.x & 15;                  // 4 output channels per thread
  const long npix = (long)Bn * OH * OW;
  for (long p = (long)blockIdx.x * 16 + (threadIdx.x >> 4); p < npix; p += (long)gridDim.x * 16) {
    const int ow = (int)(p % OW);
    const long t = p / OW;
    const int oh = (int)(t % OH);
    const int b = (int)(t / OH);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int kh = 0; kh < 7; ++kh) {
      const int h = oh * 2 - 3 + kh;
      if (h < 0 || h >= H) continue;
      for (int kw = 0; kw < 7; ++kw) {
        const int ww = ow * 2 - 3 + kw;
        if (ww < 0 || ww >= W) continue;
        const float* xp = x + (((long)b * H + h) * W + ww) * 3;
        const float* wp = ws + ((kh * 7 + kw) * 3) * DN_CO + co4 * 4;
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) {
          const float xv = xp[ci];
          acc.x = fmaf(xv, wp[ci * DN_CO + 0], acc.x);
          acc.y = fmaf(xv, wp[ci * DN_CO + 1], acc.y);
          acc.z = fmaf(xv, wp[ci * DN_CO + 2], acc.z);
          acc.w = fmaf(xv, wp[ci * DN_CO + 3], acc.w);
        }
      }
    }
    *reinterpret_cast<float4*>(y + p * DN_CO + co4 * 4) = acc;
  }
}

// dx[b,h,w,ci] = sum over the (oh, ow, kh, kw) that read (h, w) of dy . w   (gather form: no atomics)
__global__ __launch_bounds__(256) void dn_conv7_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                             float* __restrict__ dx, int Bn, int H, int W, int OH, int OW) {
  __shared__ float ws[DN_K * DN_CO];
  for (int i = threadIdx.x; i < DN_K * DN_CO; i += 256) ws[i] = w[i];
  __syncthreads();
  const long npix = (long)Bn * H * W;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long)gridDim.x * 256) {
    const int xw = (int)(p % W);
    const long t = p / W;
    const int xh = (int)(t % H);
    const int b = (int)(t / H);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int kh = 0; kh < 7; ++kh) {
      const int th = xh + 3 - kh;                  // = oh*2
      if (th < 0 || (th & 1) || (th >> 1) >= OH) continue;
      const int oh = th >> 1;
      for (int kw = 0; kw < 7; ++kw) {
        const int tw = xw + 3 - kw;
        if (tw < 0 || (tw & 1) || (tw >> 1) >= OW) continue;
        const int ow = tw >> 1;
        const float* g = dy + (((long)b * OH + oh) * OW + ow) * DN_CO;
        const float* wp = ws + ((kh * 7 + kw) * 3) * DN_CO;
        for (int co = 0; co < DN_CO; co += 4) {
          const float4 gv = *reinterpret_cast<const float4*>(g + co);
          a0 = fmaf(gv.x, wp[co], a0); a0 = fmaf(gv.y, wp[co + 1], a0); a0 = fmaf(gv.z, wp[co + 2], a0); a0 = fmaf(gv.w, wp[co + 3], a0);
          a1 = fmaf(gv.x, wp[DN_CO + co], a1); a1 = fmaf(gv.y, wp[DN_CO + co + 1], a1);
          a1 = fmaf(gv.z, wp[DN_CO + co + 2], a1); a1 = fmaf(gv.w, wp[DN_CO + co + 3], a1);
          a2 = fmaf(gv.x, wp[2 * DN_CO + co], a2); a2 = fmaf(gv.y, wp[2 * DN_CO + co + 1], a2);
          a2 = fmaf(gv.z, wp[2 * DN_CO + co + 2], a2); a2 = fmaf(gv.w, wp[2 * DN_CO + co + 3], a2);
        }
      }
    }
    dx[p * 3 + 0] = a0;
    dx[p * 3 + 1] = a1;
    dx[p * 3 + 2] = a2;
  }
}

// Weight gradient partials: slab s sums the output pixels [s*chunk, (s+1)*chunk) -> ws[s][147][64]; the slabs are then
// added in slab order (spnet_reduce_slabs).  Thread layout: 16 float4 output-channel groups x 16 tap rows.
#define DN_WG_PIX 32
__global__ __launch_bounds__(256) void dn_conv7_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                             float* __restrict__ ws, int Bn, int H, int W, int OH, int OW,
                                                             long chunk) {
  __shared__ float xs[DN_WG_PIX][DN_K + 1];
  __shared__ float4 gs[DN_WG_PIX][DN_CO / 4];
  const int co4 = threadIdx.x & 15, kr = threadIdx.x >> 4;      // taps kr, kr+16, ...
  constexpr int NK = (DN_K + 15) / 16;                          // 10
  float4 acc[NK];
#pragma unroll
  for (int j = 0; j < NK; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
  const long npix = (long)Bn * OH * OW;
  const long p0 = (long)blockIdx.x * chunk;
  const long p1 = p0 + chunk < npix ? p0 + chunk : npix;
  for (long pb = p0; pb < p1; pb += DN_WG_PIX) {
    __syncthreads();
    for (int i = threadIdx.x; i < DN_WG_PIX * DN_K; i += 256) {
      const int q = i / DN_K, k = i % DN_K;
      const long p = pb + q;
      float v = 0.f;
      if (p < p1) {
        const int ow = (int)(p % OW);
        const long t = p / OW;
        const int oh = (int)(t % OH);
        const int b = (int)(t / OH);
        const int kh = k / 21, kw = (k / 3) % 7, ci = k % 3;
        const int h = oh * 2 - 3 + kh, w = ow * 2 - 3 + kw;
        if (h >= 0 && h < H && w >= 0 && w < W) v = x[(((long)b * H + h) * W + w) * 3 + ci];
      }
      xs[q][k] = v;
    }
    for (int i = threadIdx.x; i < DN_WG_PIX * (DN_CO / 4); i += 256) {
      const int q = i / (DN_CO / 4), c4 = i % (DN_CO / 4);
      const long p = pb + q;
      gs[q][c4] = p < p1 ? *reinterpret_cast<const float4*>(dy + p * DN_CO + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    for (int q = 0; q < DN_WG_PIX; ++q) {
      const float4 g = gs[q][co4];
#pragma unroll
      for (int j = 0; j < NK; ++j) {
        const int k = kr + 16 * j;
        const float xv = k < DN_K ? xs[q][k] : 0.f;
        acc[j].x = fmaf(xv, g.x, acc[j].x);
        acc[j].y = fmaf(xv, g.y, acc[j].y);
        acc[j].z = fmaf(xv, g.z, acc[j].z);
        acc[j].w = fmaf(xv, g.w, acc[j].w);
      }
    }
  }
  float* out = ws + (long)blockIdx.x * DN_K * DN_CO;
#pragma unroll
  for (int j = 0; j < NK; ++j) {
    const int k = kr + 16 * j;
    if (k < DN_K) *reinterpret_cast<float4*>(out + k * DN_CO + co4 * 4) = acc[j];
  }
}

extern "C" int spnet_reduce_slabs(const float* ws, int nslab, int M, int N, float* out, int ldc, void* stream);  // gemm.hip

extern "C" long spnet_dense_conv7_ws(int B, int H, int W) {
  const long OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  const long npix = (long)B * OH * OW;
  long slabs = (npix + 2047) / 2048;
  if (slabs > 512) slabs = 512;
  if (slabs < 1) slabs = 1;
  return slabs * DN_K * DN_CO;
}

// op 0 fwd (a = x, b = w, out = y) | 1 data gradient (a = dy, b = w, out = dx) | 2 weight gradient (a = x, b = dy,
// out = dw; workspace >= spnet_dense_conv7_ws(B, H, W) floats).  H, W: the input plane.
extern "C" int spnet_dense_conv7(int op, const float* a, const float* b, float* out, int B, int H, int W, float* workspace,
                                 long ws_floats, void* stream) {
  if (!a || !b || !out || B < 1 || H < 1 || W < 1) return (int)hipErrorInvalidValue;
  hipStream_t st = (hipStream_t)stream;
  const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
  if (op == 0) {
    const long npix = (long)B * OH * OW;
    const long g = (npix + 15) / 16;
    hipLaunchKernelGGL(dn_conv7_fwd_kernel, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(256), 0, st, a, b, out, B, H, W, OH, OW);
  } else if (op == 1) {
    const long npix = (long)B * H * W;
    const long g = (npix + 255) / 256;
    hipLaunchKernelGGL(dn_conv7_dgrad_kernel, dim3((unsigned)(g < 8192 ? g : 8192)), dim3(256), 0, st, a, b, out, B, H, W, OH, OW);
  } else if (op == 2) {
    const long need = spnet_dense_conv7_ws(B, H, W);
    if (!workspace || ws_floats < need) return (int)hipErrorInvalidValue;
    const int slabs = (int)(need / (DN_K * DN_CO));
    const long npix = (long)B * OH * OW;
    const long chunk = (npix + slabs - 1) / slabs;
    hipLaunchKernelGGL(dn_conv7_wgrad_kernel, dim3(slabs), dim3(256), 0, st, a, b, workspace, B, H, W, OH, OW, chunk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return spnet_reduce_slabs(workspace, slabs, DN_K, DN_CO, out, DN_CO, stream);
  } else {
    return (int)hipErrorInvalidValue;
  }
  SPNET_RETURN_LAUNCH_STATUS();
}

// ------------------------------------------------------------------ statistics of a block's input channels
// partial[p][0|1][c] = sum / sum of squares of x[r][c] over the rows r of slab p (DN_ROWS rows each), the layout of the
// GEMM epilogues' column sums (spnet_bn_finalize_fwd reads it).  x pixels ldx floats apart; C % 4 == 0.
__global__ __launch_bounds__(256) void dn_colsums_kernel(const float* __restrict__ x, long ldx, long M, int C,
                                                         float* __restrict__ partial) {
  const int c4n = C >> 2;
  const int c4 = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rq = threadIdx.x >> 6;                   // 4 row lanes
  __shared__ float4 red[2][4][64];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
  const long r0 = (long)blockIdx.y * DN_ROWS;
  if (c4 < c4n) {
    for (int i = rq; i < DN_ROWS; i += 4) {
      const long r = r0 + i;
      if (r >= M) break;
      const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + c4 * 4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
      q.x = fmaf(v.x, v.x, q.x); q.y = fmaf(v.y, v.y, q.y); q.z = fmaf(v.z, v.z, q.z); q.w = fmaf(v.w, v.w, q.w);
    }
  }
  red[0][rq][threadIdx.x & 63] = s;
  red[1][rq][threadIdx.x & 63] = q;
  __syncthreads();
  if (rq < 2 && c4 < c4n) {
    float4 t = red[rq][0][threadIdx.x & 63];
    for (int k = 1; k < 4; ++k) {
      const float4 u = red[rq][k][threadIdx.x & 63];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    *reinterpret_cast<float4*>(partial + ((long)blockIdx.y * 2 + rq) * C + c4 * 4) = t;
  }
}

extern "C" long spnet_dense_rows(long M) { return (M + DN_ROWS - 1) / DN_ROWS; }

extern "C" int spnet_dense_colsums_ld(const float* x, long ldx, long M, int C, float* partial, void* stream) {
  if (!x || !partial || M < 1 || C < 4 || (C & 3) || (ldx & 3) || ldx < C) return (int)hipErrorInvalidValue;
  const long P = spnet_dense_rows(M);
  hipLaunchKernelGGL(dn_colsums_kernel, dim3((C / 4 + 63) / 64, (unsigned)P), dim3(256), 0, (hipStream_t)stream, x, ldx,
                     M, C, partial);
  SPNET_RETURN_LAUNCH_STATUS();
}

// ------------------------------------------------------------------ per-consumer affine
// coef = [scale | 0 | shift], cld floats each, zero from channel c on (the operand form of spnet_gemm_f32_bnrelu).
// training = 1: scale = gamma*invstd, shift = beta - mean*scale from the channels' shared batch statistics, and the
//   consumer's moving statistics move towards (bmean, bvar) (bvar: unbiased, as spnet_bn_finalize_fwd);
// training = 0: from the consumer's own moving statistics (keras inference).
__global__ __launch_bounds__(256) void dn_coeffs_kernel(int c, int cld, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, const float* __restrict__ bmean,
                                                        const float* __restrict__ bvar, float* __restrict__ mm,
                                                        float* __restrict__ mv, float* __restrict__ coef, float eps,
                                                        float momentum, int training) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= cld) return;
  float sc = 0.f, sh = 0.f;
  if (i < c) {
    if (training) {
      sc = __fmul_rn(gamma[i], invstd[i]);
      sh = bn_shift(beta[i], mean[i], sc);
      mm[i] = bn_moving_update(mm[i], momentum, bmean[i]);
      mv[i] = bn_moving_update(mv[i], momentum, bvar[i]);
    } else {
      const float is = (float)(1.0 / sqrt(__dadd_rn((double)mv[i], (double)eps)));
      sc = __fmul_rn(gamma[i], is);
      sh = bn_shift(beta[i], mm[i], sc);
    }
  }
  coef[i] = sc;
  coef[cld + i] = 0.f;
  coef[2 * cld + i] = sh;
}

extern "C" int spnet_dense_coeffs(int c, int cld, const float* gamma, const float* beta, const float* mean,
                                  const float* invstd, const float* bmean, const float* bvar, float* mm, float* mv,
                                  float* coef, float eps, float momentum, int training, void* stream) {
  if (c < 1 || cld < c || !gamma || !beta || !mm || !mv || !coef) return (int)hipErrorInvalidValue;
  if (training && (!mean || !invstd || !bmean || !bvar)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dn_coeffs_kernel, dim3((cld + 255) / 256), dim3(256), 0, (hipStream_t)stream, c, cld, gamma, beta,
                     mean, invstd, bmean, bvar, mm, mv, coef, eps, momentum, training);
  SPNET_RETURN_LAUNCH_STATUS();
}

// y[r*ldy + j] = act(scale[j]*x[r*ldx + j] + shift[j]) for j < C (act: 0 none, 1 ReLU); coef as spnet_dense_coeffs.
__global__ __launch_bounds__(256) void dn_apply_kernel(const float* __restrict__ x, long ldx, long M, int C,
                                                       const float* __restrict__ coef, int cld, int relu,
                                                       float* __restrict__ y, long ldy) {
  const int c4n = C >> 2;
  const long total = M * c4n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % c4n) * 4;
    const long r = i / c4n;
    const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + c);
    const float4 a = *reinterpret_cast<const float4*>(coef + c);
    const float4 s = *reinterpret_cast<const float4*>(coef + 2 * cld + c);
    float4 o;
    o.x = fmaf(a.x, v.x, s.x); o.y = fmaf(a.y, v.y, s.y); o.z = fmaf(a.z, v.z, s.z); o.w = fmaf(a.w, v.w, s.w);
    if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
    *reinterpret_cast<float4*>(y + r * ldy + c) = o;
  }
}

extern "C" int spnet_dense_apply_ld(const float* x, long ldx, long M, int C, const float* coef, int cld, int relu, float* y,
                                    long ldy, void* stream) {
  if (!x || !coef || !y || M < 1 || C < 4 || (C & 3) || (ldx & 3) || (ldy & 3) || (cld & 3) || cld < C || ldx < C || ldy < C)
    return (int)hipErrorInvalidValue;
  const long total = M * (C / 4);
  const long g = (total + 255) / 256;
  hipLaunchKernelGGL(dn_apply_kernel, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, (hipStream_t)stream, x, ldx, M,
                     C, coef, cld, relu, y, ldy);
  SPNET_RETURN_LAUNCH_STATUS();
}

// ------------------------------------------------------------------ consumer backward
// dz [M][ldz] = the gradient of consumer l's BN(+ReLU) output (its 1x1 conv's data gradient, or the head's gradient for
// the closing BatchNorm).  g = dz * [scale*x + shift > 0] (relu) | dz;  G[:, :c] += gamma * g  (one fixed accumulation
// per consumer, in the engine's backward order); partial[p][0|1][j] = sums of g and g*x^ over the rows of slab p
// (x^ = (x - mean)*invstd, the channel's shared batch statistics).
__global__ __launch_bounds__(256) void dn_consumer_bwd_kernel(const float* __restrict__ dz, long ldz,
                                                              const float* __restrict__ x, long ldx, long M, int c,
                                                              const float* __restrict__ coef, int cld,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd,
                                                              const float* __restrict__ gamma, int relu,
                                                              float* __restrict__ G, long ldg,
                                                              float* __restrict__ partial) {
  const int c4n = c >> 2;
  const int c4 = blockIdx.x * 64 + (threadIdx.x & 63);
  const int rq = threadIdx.x >> 6;
  __shared__ float4 red[2][4][64];
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), q = s;
  const long r0 = (long)blockIdx.y * DN_ROWS;
  if (c4 < c4n) {
    const int j = c4 * 4;
    const float4 a = *reinterpret_cast<const float4*>(coef + j);
    const float4 b = *reinterpret_cast<const float4*>(coef + 2 * cld + j);
    const float4 mu = *reinterpret_cast<const float4*>(mean + j);
    const float4 is = *reinterpret_cast<const float4*>(invstd + j);
    const float4 ga = *reinterpret_cast<const float4*>(gamma + j);
    for (int i = rq; i < DN_ROWS; i += 4) {
      const long r = r0 + i;
      if (r >= M) break;
      const float4 v = *reinterpret_cast<const float4*>(x + r * ldx + j);
      float4 g = *reinterpret_cast<const float4*>(dz + r * ldz + j);
      if (relu) {
        g.x = fmaf(a.x, v.x, b.x) > 0.f ? g.x : 0.f;
        g.y = fmaf(a.y, v.y, b.y) > 0.f ? g.y : 0.f;
        g.z = fmaf(a.z, v.z, b.z) > 0.f ? g.z : 0.f;
        g.w = fmaf(a.w, v.w, b.w) > 0.f ? g.w : 0.f;
      }
      float4 xh;
      xh.x = (v.x - mu.x) * is.x; xh.y = (v.y - mu.y) * is.y; xh.z = (v.z - mu.z) * is.z; xh.w = (v.w - mu.w) * is.w;
      s.x += g.x; s.y += g.y; s.z += g.z; s.w += g.w;
      q.x = fmaf(g.x, xh.x, q.x); q.y = fmaf(g.y, xh.y, q.y); q.z = fmaf(g.z, xh.z, q.z); q.w = fmaf(g.w, xh.w, q.w);
      float4* gp = reinterpret_cast<float4*>(G + r * ldg + j);
      float4 acc = *gp;
      acc.x = fmaf(ga.x, g.x, acc.x); acc.y = fmaf(ga.y, g.y, acc.y); acc.z = fmaf(ga.z, g.z, acc.z); acc.w = fmaf(ga.w, g.w, acc.w);
      *gp = acc;
    }
  }
  red[0][rq][threadIdx.x & 63] = s;
  red[1][rq][threadIdx.x & 63] = q;
  __syncthreads();
  if (rq < 2 && c4 < c4n) {
    float4 t = red[rq][0][threadIdx.x & 63];
    for (int k = 1; k < 4; ++k) {
      const float4 u = red[rq][k][threadIdx.x & 63];
      t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
    }
    *reinterpret_cast<float4*>(partial + ((long)blockIdx.y * 2 + rq) * c + c4 * 4) = t;
  }
}

extern "C" int spnet_dense_consumer_bwd(const float* dz, long ldz, const float* x, long ldx, long M, int c, const float* coef,
                                        int cld, const float* mean, const float* invstd, const float* gamma, int relu,
                                        float* G, long ldg, float* partial, void* stream) {
  if (!dz || !x || !coef || !mean || !invstd || !gamma || !G || !partial || M < 1 || c < 4 || (c & 3) || cld < c ||
      (cld & 3) || (ldz & 3) || (ldx & 3) || (ldg & 3) || ldz < c || ldx < c || ldg < c)
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dn_consumer_bwd_kernel, dim3((c / 4 + 63) / 64, (unsigned)spnet_dense_rows(M)), dim3(256), 0,
                     (hipStream_t)stream, dz, ldz, x, ldx, M, c, coef, cld, mean, invstd, gamma, relu, G, ldg, partial);
  SPNET_RETURN_LAUNCH_STATUS();
}

// dbeta_l = sum g, dgamma_l = sum g*x^; u += gamma*dbeta, v += gamma*dgamma.  Workgroup = 8 channels x 32 slab lanes:
// lane q adds slabs q, q+32, ... in double, then lane 0 adds the 32 lane sums in lane order (fixed order throughout).
__global__ __launch_bounds__(256) void dn_consumer_fin_kernel(const float* __restrict__ partial, int P, int c,
                                                              const float* __restrict__ gamma, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, float* __restrict__ u,
                                                              float* __restrict__ v) {
  __shared__ double red[2][32][8];
  const int jl = threadIdx.x & 7, q = threadIdx.x >> 3;
  const int j = blockIdx.x * 8 + jl;
  double s = 0.0, t = 0.0;
  if (j < c) {
#pragma unroll 4
    for (int p = q; p < P; p += 32) {
      s += (double)partial[(long)p * 2 * c + j];
      t += (double)partial[((long)p * 2 + 1) * c + j];
    }
  }
  red[0][q][jl] = s;
  red[1][q][jl] = t;
  __syncthreads();
  if (q == 0 && j < c) {
    for (int k = 1; k < 32; ++k) {
      s += red[0][k][jl];
      t += red[1][k][jl];
    }
    const float fs = (float)s, fq = (float)t;
    dbeta[j] = fs;
    dgamma[j] = fq;
    u[j] = fmaf(gamma[j], fs, u[j]);
    v[j] = fmaf(gamma[j], fq, v[j]);
  }
}

extern "C" int spnet_dense_consumer_fin(const float* partial, int P, int c, const float* gamma, float* dgamma, float* dbeta,
                                        float* u, float* v, void* stream) {
  if (!partial || P < 1 || c < 1 || !gamma || !dgamma || !dbeta || !u || !v) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(dn_consumer_fin_kernel, dim3((c + 7) / 8), dim3(256), 0, (hipStream_t)stream, partial, P, c, gamma,
                     dgamma, dbeta, u, v);
  SPNET_RETURN_LAUNCH_STATUS();
}

// ------------------------------------------------------------------ producer finalize
// out[r*ldo + (j - c0)] = invstd_j * (G[r][j] - u_j/M - x^_rj * v_j/M) for c0 <= j < c1: the gradient of the channels a
// layer wrote, once every consumer of them has been back-propagated.
__global__ __launch_bounds__(256) void dn_producer_fin_kernel(const float* __restrict__ G, long ldg,
                                                              const float* __restrict__ u, const float* __restrict__ v,
                                                              const float* __restrict__ x, long ldx,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, long M, int c0, int n,
                                                              float* __restrict__ out, long ldo) {
  const int c4n = n >> 2;
  const long total = M * c4n;
  const float rM = (float)(1.0 / (double)M);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int j = c0 + (int)(i % c4n) * 4;
    const long r = i / c4n;
    const float4 g = *reinterpret_cast<const float4*>(G + r * ldg + j);
    const float4 xv = *reinterpret_cast<const float4*>(x + r * ldx + j);
    const float4 uu = *reinterpret_cast<const float4*>(u + j), vv = *reinterpret_cast<const float4*>(v + j);
    const float4 mu = *reinterpret_cast<const float4*>(mean + j), is = *reinterpret_cast<const float4*>(invstd + j);
    float4 o;
    o.x = is.x * (g.x - uu.x * rM - (xv.x - mu.x) * is.x * (vv.x * rM));
    o.y = is.y * (g.y - uu.y * rM - (xv.y - mu.y) * is.y * (vv.y * rM));
    o.z = is.z * (g.z - uu.z * rM - (xv.z - mu.z) * is.z * (vv.z * rM));
    o.w = is.w * (g.w - uu.w * rM - (xv.w - mu.w) * is.w * (vv.w * rM));
    *reinterpret_cast<float4*>(out + r * ldo + (j - c0)) = o;
  }
}

extern "C" int spnet_dense_producer_fin(const float* G, long ldg, const float* u, const float* v, const float* x, long ldx,
                                        const float* mean, const float* invstd, long M, int c0, int c1, float* out,
                                        long ldo, void* stream) {
  const int n = c1 - c0;
  if (!G || !u || !v || !x || !mean || !invstd || !out || M < 1 || c0 < 0 || n < 4 || (n & 3) || (c0 & 3) ||
      (ldg & 3) || (ldx & 3) || (ldo & 3) || ldg < c1 || ldx < c1 || ldo < n)
    return (int)hipErrorInvalidValue;
  const long total = M * (n / 4);
  const long g = (total + 255) / 256;
  hipLaunchKernelGGL(dn_producer_fin_kernel, dim3((unsigned)(g < 16384 ? g : 16384)), dim3(256), 0, (hipStream_t)stream, G,
                     ldg, u, v, x, ldx, mean, invstd, M, c0, n, out, ldo);
  SPNET_RETURN_LAUNCH_STATUS();
}
