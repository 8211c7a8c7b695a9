// The random PARAMETERS of the on-the-fly augmentation drawn on the device: what DeviceAugmenter._draw (draw_cutout,
// draw_saltpepper, draw_blur_gate) and DeviceWarper.draw_into (draw_warp, warp_minv, warp_fwd) draw on the host one frame at
// a time, as one kernel that writes the arrays spnet_cutout, spnet_saltpepper, spnet_gaussian_blur, spnet_warp_chain_u8 and
// spnet_encode_targets read, in their layouts.  The stream is this kernel's own (counter based; the recipe is in
// include/spnet_hip.h): the reference's distributions, other values -- every value a function of (seed, epoch, sample index,
// draw slot) only.
//
// One wave per sample, four samples per workgroup.  The scalar draws are wave-uniform (every lane computes the same value,
// the lanes that own an output element store it); the salt-and-pepper points are divided over the lanes, lane l taking
// points l, l + 64, ...  No LDS, no atomics.
//
// The matrices are rotation_matrix_2d((W/2, H/2), angle) and invert_affine_cv2 of it (spnet_amd/augmentation.py) in double,
// in their order of operations, from the host's cos / sin of the quantised angle: every product and sum rounded on its own,
// so this file is compiled with floating-point contraction OFF (see espi_params.hip for why the pragma and not __dmul_rn).
#include "common.h"
#include "counter_rng.h"
#pragma clang fp contract(off)

#define AUGP_MAX_RECTS 6
#define AUGP_SLOT_FRAME 0     // the frame's scalar draws; slots 1 .. 6 = rectangle 0 .. 5
#define AUGP_SLOT_WARP 7
#define AUGP_SLOT_POINTS 8
#define AUGP_ANGLE_MID 2048   // angle index k in 0 .. 4096, angle = (k - 2048) * (20 / 2048) degrees

__global__ __launch_bounds__(256) void augment_params_kernel(unsigned seed, unsigned epoch, const int* __restrict__ sample,
                                                             int B, int H, int W, int n_salt, int n_pepper,
                                                             const float* __restrict__ mm, int n_frames,
                                                             int* __restrict__ rects, float* __restrict__ vals,
                                                             int* __restrict__ nrect, int* __restrict__ coords,
                                                             int* __restrict__ flag, int* __restrict__ ksize, int Hw, int Ww,
                                                             const double* __restrict__ trig, double* __restrict__ records,
                                                             double* __restrict__ fwd) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;                                   // the whole wave leaves together
  const int s = sample[b];
  const unsigned skey = rng_mix(rng_mix(rng_mix(seed ^ 0x3c6ef372u) + epoch) ^ (unsigned)s);

  if (rects) {
    const unsigned k0 = rng_mix(skey + AUGP_SLOT_FRAME);
    const int n = rng_randint(rng_draw(k0, 0), 0, AUGP_MAX_RECTS);
    const int sp = (int)(rng_draw(k0, 1) >> 31);
    int ks = 0;
    if ((double)rng_u01(rng_draw(k0, 2)) < 0.4 && (double)rng_u01(rng_draw(k0, 3)) <= 0.3)
      ks = (rng_draw(k0, 4) >> 31) ? 7 : 3;
    // the fill range is the pristine frame's (the table row of the SAMPLE; an index outside the table reads its nearest row)
    const int row = min(max(s, 0), n_frames - 1);
    const float lo = mm[2 * row], hi = mm[2 * row + 1];
    int rv = 0;                                         // this lane's element of rects[b] (lanes 0 .. 23)
    float fv = 0.f;                                     // this lane's element of vals[b] (lanes 0 .. 5)
#pragma unroll
    for (int r = 0; r < AUGP_MAX_RECTS; ++r) {
      const unsigned kr = rng_mix(skey + (unsigned)(1 + r));
      const int r0 = rng_randint(rng_draw(kr, 0), 0, H - 12), c0 = rng_randint(rng_draw(kr, 1), 0, W - 12);
      const int dr = rng_randint(rng_draw(kr, 2), 11, 74), dc = rng_randint(rng_draw(kr, 3), 11, 74);
      const int r1 = min(r0 + dr, H - 1), c1 = min(c0 + dc, W - 1);
      const float fill = lo + rng_u01(rng_draw(kr, 4)) * (hi - lo);
      if (r < n) {
        if ((lane >> 2) == r) rv = (lane & 3) == 0 ? r0 : (lane & 3) == 1 ? r1 : (lane & 3) == 2 ? c0 : c1;
        if (lane == r) fv = fill;
      }
    }
    if (lane < AUGP_MAX_RECTS * 4) rects[(long)b * AUGP_MAX_RECTS * 4 + lane] = rv;
    if (lane < AUGP_MAX_RECTS) vals[(long)b * AUGP_MAX_RECTS + lane] = fv;
    if (lane == 0) {
      nrect[b] = n;
      flag[b] = sp;
      ksize[b] = ks;
    }
    // rows then columns, salt points first; a frame whose gate is off holds zeros (every element is defined)
    const int npts = n_salt + n_pepper;
    const unsigned kp = rng_mix(skey + AUGP_SLOT_POINTS);
    int* const cr = coords + (long)b * 2 * npts;
    for (int p = lane; p < npts; p += 64) {
      const int pr = rng_randint(rng_draw(kp, 2u * (unsigned)p), 0, H - 2);
      const int pc = rng_randint(rng_draw(kp, 2u * (unsigned)p + 1u), 0, W - 2);
      cr[p] = sp ? pr : 0;
      cr[npts + p] = sp ? pc : 0;
    }
  }

  if (records) {
    const unsigned kw = rng_mix(skey + AUGP_SLOT_WARP);
    const int flip = (int)(rng_draw(kw, 0) >> 30) - 2;
    const int k = rng_randint(rng_draw(kw, 1), 0, 2 * AUGP_ANGLE_MID);
    int xt = 0, yt = 0;
    if (rng_randint(rng_draw(kw, 2), 0, 9) != 0) {
      const double ux = rng_u01_double(rng_draw(kw, 3));
      const double uy = rng_u01_double(rng_draw(kw, 4));
      xt = (int)rint(40.0 * (2.0 * ux - 1.0));
      yt = (int)rint(40.0 * (2.0 * uy - 1.0));
    }
    const double angle = (double)(k - AUGP_ANGLE_MID) * (20.0 / 2048.0);
    double f00 = 1.0, f01 = 0.0, f02 = 0.0, f10 = 0.0, f11 = 1.0, f12 = 0.0;     // forward (rotation_matrix_2d)
    double i00 = 1.0, i01 = 0.0, i02 = 0.0, i10 = 0.0, i11 = 1.0, i12 = 0.0;     // inverted (invert_affine_cv2)
    if (k != AUGP_ANGLE_MID) {                          // angle 0: both stay the identity, as warp_minv / warp_fwd say
      const double a = trig[2 * k], bb = trig[2 * k + 1];
      const double cx = (double)Ww / 2.0, cy = (double)Hw / 2.0;
      f00 = a; f01 = bb; f02 = (1.0 - a) * cx - bb * cy;
      f10 = -bb; f11 = a; f12 = bb * cx + (1.0 - a) * cy;
      double D = f00 * f11 - f01 * f10;
      D = D != 0.0 ? 1.0 / D : 0.0;
      i00 = f11 * D;
      i11 = f00 * D;
      i01 = f01 * -D;
      i10 = f10 * -D;
      i02 = -i00 * f02 - i01 * f12;
      i12 = -i10 * f02 - i11 * f12;
    }
    // the 64-byte record { double m[6]; int flip, xt, yt, pad } and fwd[8] = forward matrix, angle, 0
    double* const rec = records + (long)b * 8;
    if (lane < 6) rec[lane] = lane == 0 ? i00 : lane == 1 ? i01 : lane == 2 ? i02 : lane == 3 ? i10 : lane == 4 ? i11 : i12;
    if (lane >= 6 && lane < 10) ((int*)(rec + 6))[lane - 6] = lane == 6 ? flip : lane == 7 ? xt : lane == 8 ? yt : 0;
    if (lane < 8)
      fwd[(long)b * 8 + lane] = lane == 0 ? f00 : lane == 1 ? f01 : lane == 2 ? f02 : lane == 3 ? f10 : lane == 4 ? f11
                              : lane == 5 ? f12 : lane == 6 ? angle : 0.0;
  }
}

extern "C" int spnet_augment_params(unsigned seed, unsigned epoch, const int* sample, int B, int H, int W, int n_salt,
                                    int n_pepper, const float* mm, int n_frames, int* rects, float* vals, int* nrect,
                                    int* coords, int* flag, int* ksize, int Hw, int Ww, const double* trig,
                                    void* warp_records, double* fwd, void* stream) {
  if (B < 0 || !sample || (!rects && !warp_records)) return (int)hipErrorInvalidValue;
  if (rects && (H < 12 || H > 2048 || W < 12 || W > 2048 || n_salt < 0 || n_pepper < 0 || n_frames < 1 || !mm || !vals ||
                !nrect || !flag || !ksize || (n_salt + n_pepper > 0 && !coords)))
    return (int)hipErrorInvalidValue;
  if (warp_records && (Hw < 1 || Hw > 2048 || Ww < 1 || Ww > 2048 || !trig || !fwd || ((uintptr_t)warp_records & 7) ||
                       ((uintptr_t)fwd & 7) || ((uintptr_t)trig & 7)))
    return (int)hipErrorInvalidValue;
  if (B == 0) return 0;
  hipLaunchKernelGGL(augment_params_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, seed, epoch, sample, B, H,
                     W, n_salt, n_pepper, mm, n_frames, rects, vals, nrect, coords, flag, ksize, Hw, Ww, trig,
                     (double*)warp_records, fwd);
  SPNET_RETURN_LAUNCH_STATUS();
}
