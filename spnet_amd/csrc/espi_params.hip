// The random PARAMETERS of fake-ESPI frames drawn on the device: what spnet_amd/fake_espi.py draw_params draws on the host,
// one frame at a time (the reference's draw_waves, gen_fake_espi.py:60-80, and draw_antinodes :145-206 with its non-overlap
// rejection loop of up to 2000 tries per antinode), as one kernel that writes the three arrays spnet_fake_espi reads.
// The stream is this kernel's own (counter based; the recipe is in include/spnet_hip.h), not the reference's interleaved
// `random` / numpy order: same distributions, other frames.
//
// One wave per frame.  The antinodes of a frame are placed one after the other (each must miss the boxes accepted before
// it); the candidates of ONE antinode are independent draws, so they are tried 64 at a time: lane l of round r evaluates
// try t = 64 r + l, and the candidate with the smallest passing t wins (ballot, lowest set bit, broadcast) -- exactly what
// the sequential loop accepts.  The one quantity the sequential loop carries from try to try, the ring count (clamped to
// b / 4 at every try, never raised again), is a running minimum: a prefix minimum over the lanes plus a carry between
// rounds.  Accepted boxes live in registers (wave-uniform); no LDS, no atomics, no scratch buffer.
//
// The box test is reproducible in numpy float32: every product and sum is rounded on its own -- this file is compiled with
// floating-point contraction OFF (the pragma below; hipcc's __fmul_rn / __fadd_rn are plain operators that the default
// contraction mode still fuses into v_fmac_f32, so they do not pin a rounding) -- cos^2 / sin^2 come from a host table, and
// the square root is taken in double and rounded to float, which is the correctly rounded float root (53 >= 2 * 24 + 2
// bits: the double rounding is harmless).
#include "common.h"
#include "counter_rng.h"
#include "espi_layout.h"
#pragma clang fp contract(off)

#define ESPI_MAX_TRIES 2000   // candidates per antinode: try 0 (the first draw) and 1999 retries
#define ESPI_MIN_LINE_WIDTH 4

// key of one (frame, slot, try): slot 0 = the frame's own draws, slot j + 1 = antinode j
__device__ __forceinline__ unsigned espi_key(unsigned frame_key, int slot, int t) {
  return rng_mix(frame_key + (((unsigned)slot << 12) | (unsigned)t));
}
__device__ __forceinline__ float espi_sqrt_rn(float v) { return (float)sqrt((double)v); }

struct EspiBox {
  float x0, y0, x1, y1;
};

__global__ __launch_bounds__(256) void fake_espi_params_kernel(long first_frame, int N, int H, int W, unsigned seed,
                                                               int count_lo, int count_hi,
                                                               const float* __restrict__ trig2, float* __restrict__ waves,
                                                               float* __restrict__ nodes, int* __restrict__ nnode,
                                                               int* __restrict__ tries) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (f >= N) return;                                   // the whole wave leaves together
  const unsigned long long g = (unsigned long long)(first_frame + f);
  const unsigned fkey = rng_mix(rng_mix(rng_mix(seed ^ 0x9e3779b9u) + (unsigned)g) ^ (unsigned)(g >> 32));

  // ---- the wave train and the antinode count (slot 0; every lane computes the same values)
  const unsigned k0 = espi_key(fkey, 0, 0);
  const int amp = rng_randint(rng_draw(k0, 0), 10, 200);
  const int wavelength = rng_randint(rng_draw(k0, 1), 100, W / 2);
  const int thick = rng_randint(rng_draw(k0, 2), 15, 40);
  const float u01 = rng_u01(rng_draw(k0, 3));
  const float slope = 3.f * (u01 - 0.5f);
  const int steep = (int)fabsf(1.5f * slope);
  const int spacing = rng_randint(rng_draw(k0, 4), thick + thick * steep, H / 3);
  const int count = rng_randint(rng_draw(k0, 5), count_lo, count_hi);
  if (lane < ESPI_WAVE_STRIDE) {
    const float v = lane == 0 ? (float)amp : lane == 1 ? (float)wavelength : lane == 2 ? (float)thick
                  : lane == 3 ? slope : (float)spacing;
    waves[(long)f * ESPI_WAVE_STRIDE + lane] = v;
  }

  EspiBox box[ESPI_MAX_NODES];
#pragma unroll
  for (int i = 0; i < ESPI_MAX_NODES; ++i) box[i] = EspiBox{0.f, 0.f, 0.f, 0.f};
  int nacc = 0;
  const float fW = (float)W, fH = (float)H;
  float* const nd = nodes + (long)f * ESPI_MAX_NODES * ESPI_NODE_STRIDE;

#pragma unroll 1
  for (int j = 0; j < ESPI_MAX_NODES; ++j) {
    int accepted_t = j < count ? -1 : -2;
    if (j < count) {
      const int start = (int)(rng_draw(espi_key(fkey, j + 1, 0), 6) >> 31);
      int carry = 0x7fffffff;                           // running minimum of the ring count over the tries so far
#pragma unroll 1
      for (int r = 0; r < (ESPI_MAX_TRIES + 63) / 64; ++r) {
        const int t = 64 * r + lane;
        const unsigned key = espi_key(fkey, j + 1, t);
        const bool first = (t == 0);
        const int a1 = first ? rng_randint(rng_draw(key, 0), 15, (2 * W) / 7) : rng_randint(rng_draw(key, 0), 25, W / 3);
        const int a2 = first ? rng_randint(rng_draw(key, 1), 15, (2 * H) / 7) : rng_randint(rng_draw(key, 1), 25, H / 3);
        const int a = max(a1, a2), b = min(a1, a2);
        // ring count: drawn with the first candidate, then min(rings, b / 4) at every retry (b / rings >= 4)
        int rmin = b / ESPI_MIN_LINE_WIDTH;
        if (first) rmin = min(rmin, rng_randint(rng_draw(key, 2), 1, min(b / 8, 11)));
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_up(rmin, off, 64);
          if (lane >= off) rmin = min(rmin, o);
        }
        const int rings = min(carry, rmin);
        const int cx = rng_randint(rng_draw(key, 3), a, W - a);
        const int cy = rng_randint(rng_draw(key, 4), b, H - b);
        const int ang = rng_randint(rng_draw(key, 5), 1, first ? 179 : 180);
        const float c2 = trig2[2 * ang], s2 = trig2[2 * ang + 1];
        const float fa2 = (float)a * (float)a, fb2 = (float)b * (float)b;
        const float dx = espi_sqrt_rn(fa2 * c2 + fb2 * s2);
        const float dy = espi_sqrt_rn(fa2 * s2 + fb2 * c2);
        EspiBox c;
        c.x0 = (float)cx - dx; c.y0 = (float)cy - dy;
        c.x1 = (float)cx + dx; c.y1 = (float)cy + dy;
        bool bad = c.x0 < 0.f || c.x1 > fW || c.y0 < 0.f || c.y1 > fH;
#pragma unroll
        for (int i = 0; i < ESPI_MAX_NODES; ++i)
          if (i < nacc) bad = bad || !(c.x1 < box[i].x0 || c.x0 > box[i].x1 || c.y1 < box[i].y0 || c.y0 > box[i].y1);
        const unsigned long long pass = __ballot(!bad && t < ESPI_MAX_TRIES);
        if (pass) {                                     // wave-uniform
          const int src = __ffsll((long long)pass) - 1;
          accepted_t = 64 * r + src;
          EspiBox w;
          w.x0 = __shfl(c.x0, src, 64); w.y0 = __shfl(c.y0, src, 64);
          w.x1 = __shfl(c.x1, src, 64); w.y1 = __shfl(c.y1, src, 64);
          const int wcx = __shfl(cx, src, 64), wcy = __shfl(cy, src, 64), wa = __shfl(a, src, 64), wb = __shfl(b, src, 64);
          const int wang = __shfl(ang, src, 64), wrings = __shfl(rings, src, 64);
#pragma unroll
          for (int i = 0; i < ESPI_MAX_NODES; ++i)
            if (i == nacc) box[i] = w;
          if (lane < ESPI_NODE_STRIDE) {
            const int v = lane == 0 ? wcx : lane == 1 ? wcy : lane == 2 ? wa : lane == 3 ? wb : lane == 4 ? wang
                        : lane == 5 ? wrings : lane == 6 ? start : 1;
            nd[nacc * ESPI_NODE_STRIDE + lane] = (float)v;
          }
          ++nacc;
          break;
        }
        carry = min(carry, __shfl(rmin, 63, 64));
      }
    }
    if (tries && lane == 0) tries[(long)f * ESPI_MAX_NODES + j] = accepted_t;
  }
  // the unused slots are zeros (valid = 0), so every element of the three arrays is defined
  if (lane < ESPI_MAX_NODES * ESPI_NODE_STRIDE && lane >= nacc * ESPI_NODE_STRIDE) nd[lane] = 0.f;
  if (lane == 0) nnode[f] = nacc;
}

extern "C" int spnet_fake_espi_params(long first_frame, int N, int H, int W, unsigned seed, int count_lo, int count_hi,
                                      const float* trig2, float* waves, float* nodes, int* nnode, int* tries, void* stream) {
  if (N < 0 || first_frame < 0 || H < 64 || H > 2048 || W < 64 || W > 2048 || count_lo < 0 || count_lo > count_hi ||
      count_hi > ESPI_MAX_NODES || !trig2 || !waves || !nodes || !nnode)
    return (int)hipErrorInvalidValue;
  if (N == 0) return 0;
  hipLaunchKernelGGL(fake_espi_params_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, first_frame, N, H, W,
                     seed, count_lo, count_hi, trig2, waves, nodes, nnode, tries);
  SPNET_RETURN_LAUNCH_STATUS();
}
