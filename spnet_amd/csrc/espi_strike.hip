// Strike sequences: the frame-0 parameters of a fake-ESPI frame (what spnet_fake_espi_params writes for one global frame)
// evolved over T frames, so that a movie has antinodes with KNOWN identities whose ring counts rise and fall -- the struck
// note at once, the sympathetic notes after an onset of their own.  The rule and its key recipe are stated beside the
// prototype in include/spnet_hip.h ("Strike sequences"); spnet_amd/fake_espi.py strike_params_host is the same rule in
// numpy, tests/helpers/track_score_ref.py restates it in Python integers.
//
// One thread per slot (s, t, j): the slot's four envelope draws and two jitter draws are functions of (seed, the GLOBAL
// sequence index, t, j) alone, so there is no state, no LDS and no atomics, and a frame does not depend on S, on
// first_sequence or on how a range of sequences is split into calls.  Thread j == 0 of a frame also copies the wave train
// and the slot count.  Integer-only apart from int -> float conversions of values below 2^24, which are exact.
//
// Bounds: the base slot count is clamped to 0 .. 7, the base ring count to 0 .. 255; the flat slot index runs below
// S * T * 7 < 2^34 in a long; nothing read from the base arrays is used as an address.
#include "common.h"
#include "counter_rng.h"
#include "espi_layout.h"

#define STRIKE_MAX_T 4096      // t fits the 12 low bits of a key, as a try does in espi_params.hip
#define STRIKE_MAX_J 8

// key of one (slot, t): slot 0 = the envelope draws of antinode t (t = j here), slot j + 1 = the jitter of antinode j at t
__device__ __forceinline__ unsigned strike_key(unsigned seq_key, int slot, int t) {
  return rng_mix(seq_key + (((unsigned)slot << 12) | (unsigned)t));
}

// The envelope in 0 .. 256 at time t.
__device__ __forceinline__ int strike_envelope(int t, int onset, int rise, int hold, int decay) {
  if (t < onset) return 0;
  const int peak = onset + rise;                        // the first frame at 256
  if (t < peak) return 256 * (t - onset + 1) / (rise + 1);
  const int after = peak + hold + 1;                    // the first frame of the decay
  if (t < after) return 256;
  return max(256 - 256 * (t - after + 1) / (decay + 1), 0);
}

__global__ __launch_bounds__(256) void fake_espi_strike_kernel(const float* __restrict__ waves0, const float* __restrict__ nodes0,
                                                               const int* __restrict__ nnode0, long first_sequence, int S,
                                                               int T, unsigned seed, int J, float* __restrict__ waves,
                                                               float* __restrict__ nodes, int* __restrict__ nnode,
                                                               int* __restrict__ ident) {
  const long total = (long)S * T * ESPI_MAX_NODES;
  for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
    const long frame = x / ESPI_MAX_NODES;
    const int j = (int)(x - frame * ESPI_MAX_NODES);
    const int s = (int)(frame / T), t = (int)(frame - (long)s * T);
    const unsigned long long g = (unsigned long long)(first_sequence + s);
    const unsigned skey = rng_mix(rng_mix(rng_mix(seed ^ 0x51ed270bu) + (unsigned)g) ^ (unsigned)(g >> 32));
    const int nn = min(max(nnode0[s], 0), ESPI_MAX_NODES);
    const float* base = nodes0 + (long)s * ESPI_MAX_NODES * ESPI_NODE_STRIDE;

    int struck = ESPI_MAX_NODES;                        // the first valid slot of the base frame
    for (int i = nn - 1; i >= 0; --i)
      if (base[i * ESPI_NODE_STRIDE + 7] != 0.f) struck = i;
    const float* b = base + j * ESPI_NODE_STRIDE;
    const bool valid = j < nn && b[7] != 0.f;

    int rings = 0;
    if (valid) {
      const unsigned ek = strike_key(skey, 0, j);
      const int onset = j == struck ? 0 : rng_randint(rng_draw(ek, 0), 0, T / 2);
      const int rise = j == struck ? 0 : rng_randint(rng_draw(ek, 1), 1, max(T / 4, 1));
      const int hold = rng_randint(rng_draw(ek, 2), 0, T / 4);
      const int decay = rng_randint(rng_draw(ek, 3), 1, T);
      const int R = (int)fminf(fmaxf(b[5], 0.f), 255.f);               // NaN gives 0
      rings = (R * strike_envelope(t, onset, rise, hold, decay) + 128) >> 8;
    }
    float* o = nodes + x * ESPI_NODE_STRIDE;
    if (rings >= 1) {
      const unsigned jk = strike_key(skey, j + 1, t);
      o[0] = b[0] + (float)rng_randint(rng_draw(jk, 0), -J, J);
      o[1] = b[1] + (float)rng_randint(rng_draw(jk, 1), -J, J);
      o[2] = b[2]; o[3] = b[3]; o[4] = b[4];
      o[5] = (float)rings;
      o[6] = b[6];
      o[7] = 1.f;
      ident[x] = (int)(1 + (long)g * ESPI_MAX_NODES + j);
    } else {
#pragma unroll
      for (int c = 0; c < ESPI_NODE_STRIDE; ++c) o[c] = 0.f;
      ident[x] = 0;
    }
    if (j == 0) {
#pragma unroll
      for (int c = 0; c < ESPI_WAVE_STRIDE; ++c) waves[frame * ESPI_WAVE_STRIDE + c] = waves0[(long)s * ESPI_WAVE_STRIDE + c];
      nnode[frame] = nn;
    }
  }
}

extern "C" int spnet_fake_espi_strike(const float* waves0, const float* nodes0, const int* nnode0, long first_sequence, int S,
                                      int T, unsigned seed, int J, float* waves, float* nodes, int* nnode, int* ident,
                                      void* stream) {
  if (!waves0 || !nodes0 || !nnode0 || !waves || !nodes || !nnode || !ident || S < 0 || T < 1 || T > STRIKE_MAX_T || J < 0 ||
      J > STRIKE_MAX_J || first_sequence < 0 || (long)S * T > 0x7fffffffL ||
      first_sequence + S > (0x7fffffffL - 1) / ESPI_MAX_NODES)
    return (int)hipErrorInvalidValue;
  if (S == 0) return 0;
  const long total = (long)S * T * ESPI_MAX_NODES;
  hipLaunchKernelGGL(fake_espi_strike_kernel, dim3(spnet_ew_grid(total, 256)), dim3(256), 0, (hipStream_t)stream, waves0, nodes0,
                     nnode0, first_sequence, S, T, seed, J, waves, nodes, nnode, ident);
  SPNET_RETURN_LAUNCH_STATUS();
}
