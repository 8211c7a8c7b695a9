// Note envelopes: a bank of single-frequency DFTs, one per pan note, on a window that starts at each video frame's
// instant.  The rule is stated beside the prototype in spnet_hip.h ("Note envelopes"); spnet_amd/audio.py is the host side
// and holds the same rule in numpy (note_envelopes_host), tests/helpers/audio_ref.py restates it in Python integers.
//
// note_envelopes_kernel: one workgroup per (recording, group of up to 8 consecutive frames) -- audio_core.h describes the
// group, its three LDS tables (24 + 16 + 16 KiB) and why a group's samples fit.  The tables are staged once, one barrier,
// then the four waves take the group's (frame, note) units round robin: a lane strides over the window, two 64-bit
// multiply-adds a term, and a shuffle reduction leaves the unit's two sums in lane 0, which stores them.  Integers only,
// no atomics, no readback; every (s, t, k) is written by exactly one lane, so the result does not depend on the grid.
//
// Bounds: len is clamped to 0 .. L before it guards a read of pcm; the span is at most SPAN_MAX by group_frames (a group
// that would exceed it -- none can -- writes nothing rather than past the table); a frame's window lies inside the span; a
// table position is 12 bits; t < T, k < K and s < S by the grid.
#include "common.h"
#include "audio_core.h"

namespace {

using namespace audio;

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__global__ __launch_bounds__(THREADS) void note_envelopes_kernel(const int16_t* __restrict__ pcm, const int* __restrict__ len,
                                                                 int s_base, long L, int T, long offset, long hop_num,
                                                                 long hop_den, const int16_t* __restrict__ win, int Wn,
                                                                 const uint32_t* __restrict__ step, int K,
                                                                 const int16_t* __restrict__ ctab, int frames,
                                                                 long long* __restrict__ re, long long* __restrict__ im) {
  __shared__ int16_t s_x[SPAN_MAX];
  __shared__ int16_t s_win[MAX_WN];
  __shared__ uint32_t s_trig[TAB];

  const long s = (long)s_base + blockIdx.y;
  const long t0 = (long)blockIdx.x * frames;
  const int nf = (int)((long)T - t0 < frames ? (long)T - t0 : frames);
  const int tid = threadIdx.x;
  const long n0 = start(t0, offset, hop_num, hop_den);
  const long span = group_span(t0, nf, offset, hop_num, hop_den, Wn);
  if (nf < 1 || span > SPAN_MAX) return;                   // uniform; neither happens (grid = ceil(T / frames); SPAN)

  const int16_t* row = pcm + s * L;
  const long ln = clamp_len(len[s], L);
  for (int j = tid; j < (int)span; j += THREADS) s_x[j] = sample(row, ln, n0 + j);
  for (int j = tid; j < Wn; j += THREADS) s_win[j] = win[j];
  for (int j = tid; j < TAB; j += THREADS) s_trig[j] = pack_trig(ctab, j);
  __syncthreads();

  const int wave = tid / WAVE, lane = tid % WAVE;
  for (int unit = wave; unit < nf * K; unit += WAVES) {     // wave-uniform
    const int f = unit / K, k = unit - f * K;
    const int off = (int)(start(t0 + f, offset, hop_num, hop_den) - n0);
    long long r, m;
    lane_sums(s_x + off, s_win, Wn, s_trig, step[k], lane, &r, &m);
    r = wave_sum_i64(r);
    m = wave_sum_i64(m);
    if (lane == 0) {
      const long o = ((s * T) + t0 + f) * K + k;
      re[o] = r;
      im[o] = m;
    }
  }
}

bool aligned(const void* p, uintptr_t a) { return p != nullptr && ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int spnet_note_envelopes(const int16_t* pcm, const int* len, int S, long L, int T, long offset, long hop_num,
                                    long hop_den, const int16_t* win, int Wn, const uint32_t* step, int K,
                                    const int16_t* ctab, long long* re, long long* im, void* stream) {
  if (!aligned(pcm, 2) || !aligned(len, 4) || !aligned(win, 2) || !aligned(step, 4) || !aligned(ctab, 2) || !aligned(re, 8) ||
      !aligned(im, 8) || !limits_ok(S, L, T, offset, hop_num, hop_den, Wn, K))
    return (int)hipErrorInvalidValue;
  if (S == 0) return 0;
  const int frames = group_frames(hop_num, hop_den, Wn);
  const int groups = spnet_cdiv(T, frames);
  spnet_for_grid_chunks(S, [&](int s0, int n) {
    hipLaunchKernelGGL(note_envelopes_kernel, dim3(groups, n), dim3(THREADS), 0, (hipStream_t)stream, pcm, len, s0, L, T,
                       offset, hop_num, hop_den, win, Wn, step, K, ctab, frames, re, im);
  });
  SPNET_RETURN_LAUNCH_STATUS();
}
