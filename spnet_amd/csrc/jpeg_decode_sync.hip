// Entropy decoding of restart intervals that are too long for one lane: a file of Pillow, of libjpeg with default settings
// or of a camera's Motion-JPEG stream carries no restart markers, so it is ONE interval and spnet_jpeg_entropy
// (jpeg_decode.hip) decodes it with one serial lane.  Huffman-coded data synchronises itself: a decoder that starts
// mid-stream in the wrong state usually falls in with the true symbol boundaries after a few dozen symbols.
// jpeg_sync_core.h builds an EXACT decoder on that (segments, ownership, the state, the FF 00 rule, the rounds and why
// their fixed point is the serial decode); tools/jpeg_sync_host_check.cpp runs the same functions under host sanitizers.
//
//   spnet_jpeg_entropy_sync  ONE WORKGROUP PER INTERVAL, ONE LANE PER SEGMENT of seg_bytes bytes.  The file's Huffman table
//       set sits in LDS (3,616 bytes) as in spnet_jpeg_entropy.  An interval of more segments than a batch holds is
//       worked off batch after batch (a batch: min(lanes, 32 KiB / seg_bytes) segments); lane 0 of a batch enters in the
//       previous batch's final exit state, which is true.  Per batch:
//         1. the batch's bytes (and SYNC_READ_AHEAD more) are copied into LDS with 16-byte loads; every decode reads there
//         2. every lane decodes its segment from its guess (scan_segment: writes nothing), its exit state goes to LDS
//         3. rounds, stepped with workgroup barriers: a lane whose predecessor's exit differs from the entry it last
//            used decodes again; the rounds end when __syncthreads_or finds no such lane
//         4. one workgroup-wide exclusive scan (wave shuffles, then the waves' totals through LDS) over the blocks that
//            finish in a segment, the three sums of DC differences and the error flag gives every lane the ordinal of
//            its block in progress, its predictors and whether the true decode failed before it
//         5. write_segment decodes once more and stores the coefficients (16-bit vector stores, natural order, the
//            layout of spnet_jpeg_entropy)
//       Nothing spins on global memory, workgroups do not cooperate, and the host launches once.  status is NOT cleared:
//       the kernel merges with atomicMax, so it runs behind spnet_jpeg_entropy (which clears) on the same array.
#include "common.h"
#include "jpeg_sync_core.h"

#ifndef SPNET_JPEG_SYNC_LANES
#define SPNET_JPEG_SYNC_LANES 256
#endif

namespace {

using namespace jpegdec;

constexpr int SY_T = SPNET_JPEG_SYNC_LANES;          // lanes of a workgroup
constexpr int SY_WAVES = SY_T / SPNET_WAVE;
constexpr int SY_WINDOW = 32768;                     // bytes of a batch's segments (tools/jpeg_sync_host_check.cpp: the same)
static_assert(SY_T % SPNET_WAVE == 0 && SY_T >= SPNET_WAVE && SY_T <= 1024, "whole waves");
// All LDS is one dynamic block (static arrays in front of it would shift its base off 16 bytes): the table set, the
// lanes' exit states, the waves' totals of the scan, then the window (16 bytes of slack for its alignment shift).
constexpr int SY_EXIT_AT = (int)sizeof(TableSet);
constexpr int SY_TOTAL_AT = SY_EXIT_AT + SY_T * (int)sizeof(SyncState);
constexpr int SY_WINDOW_AT = (SY_TOTAL_AT + SY_WAVES * 5 * 4 + 15) / 16 * 16;
static_assert(SY_EXIT_AT % 8 == 0 && SY_TOTAL_AT % 4 == 0, "natural alignment of the pieces");

__global__ __launch_bounds__(SY_T) void jpeg_entropy_sync_kernel(const unsigned char* __restrict__ blob, long blob_bytes,
                                                                 const int* __restrict__ intervals,
                                                                 const int* __restrict__ files, int n_files,
                                                                 const uint32_t* __restrict__ tables, int n_sets,
                                                                 int seg_bytes, int batch, int16_t* __restrict__ coef,
                                                                 long total_blocks, int* __restrict__ status) {
  extern __shared__ __align__(16) unsigned char s_lds[];                 // SY_WINDOW_AT + 16 + batch * seg_bytes + SYNC_READ_AHEAD
  const TableSet& s_set = *reinterpret_cast<const TableSet*>(s_lds);
  SyncState* s_exit = reinterpret_cast<SyncState*>(s_lds + SY_EXIT_AT);
  uint32_t(*s_total)[5] = reinterpret_cast<uint32_t(*)[5]>(s_lds + SY_TOTAL_AT);
  unsigned char* s_bytes = s_lds + SY_WINDOW_AT;
  const int t = threadIdx.x;
  const int* iv = intervals + (long)blockIdx.x * INTERVAL_INTS;
  const int fi = iv[2];
  if (fi < 0 || fi >= n_files) return;                                  // (uniform) no file to blame
  const int* f = files + (long)fi * FILE_INTS;
  const int ok = sync_interval_ok(blob_bytes, iv, f, n_sets, total_blocks);
  if (ok != OK) {                                                       // (uniform)
    if (t == 0) atomicMax(&status[fi], ok);
    return;
  }
  if (iv[4] == 0) return;                                               // (uniform) an empty interval, as decode_interval
  {
    uint32_t* dst = reinterpret_cast<uint32_t*>(s_lds);
    const uint32_t* src = tables + (long)f[F_TABLE_SET] * (4 * TABLE_WORDS);      // file_ok: the set exists
    for (int w = t; w < 4 * TABLE_WORDS; w += SY_T) dst[w] = src[w];
  }
  const int lo = iv[0], hi = iv[1];
  const int nseg = sync_segments(iv, seg_bytes);
  const long total = (long)iv[4] * sync_blocks_per_mcu(f);
  SyncState carry = sync_state(lo, 0, 0, 0);
  long ord_base = 0;
  uint32_t pred_base[3] = {0, 0, 0};

  for (int sb = 0; sb < nseg; sb += batch) {
    const int nl = min(batch, nseg - sb);                               // lanes with a segment
    const int org = (int)(lo + (long)sb * seg_bytes);                   // < hi, or lo of an empty interval
    const int wlen = (int)min((long)hi - org, (long)batch * seg_bytes + SYNC_READ_AHEAD);
    // the window keeps the source's position inside a 16-byte line, so that the body moves as aligned 16-byte pieces
    const unsigned char* src = blob + org;
    unsigned char* win = s_bytes + ((uintptr_t)src & 15);
    __syncthreads();                                                    // the batch before is done with window and tables
    {
      const int head = min(wlen, (int)((16 - ((uintptr_t)src & 15)) & 15));
      const int nvec = (wlen - head) >> 4;
      for (int i = t; i < head; i += SY_T) win[i] = src[i];
      for (int i = t; i < nvec; i += SY_T)
        *reinterpret_cast<uint4*>(win + head + 16 * i) = *reinterpret_cast<const uint4*>(src + head + 16 * i);
      for (int i = head + 16 * nvec + t; i < wlen; i += SY_T) win[i] = src[i];
    }
    __syncthreads();
    const bool active = t < nl;
    const int own_end = !active || sb + t == nseg - 1 ? SYNC_NOWHERE : org + (t + 1) * seg_bytes;
    SyncState used = carry;
    SegScan got;
    got.exit = carry;
    got.status = OK;
    got.blocks = got.dc[0] = got.dc[1] = got.dc[2] = 0;
    if (active) {
      if (t > 0) used = sync_guess(win, org, hi, org + t * seg_bytes);
      got = scan_segment(win, org, hi, own_end, f, s_set, used);
      s_exit[t] = got.exit;
    }
    // after round r the segments 0 .. r of the batch have true entries: at most nl rounds decode anything
    for (int round = 0; round <= nl; ++round) {
      __syncthreads();                                                  // the exits of the round before
      SyncState in = used;
      if (active && t > 0) in = s_exit[t - 1];
      const bool again = !sync_same(in, used);
      if (!__syncthreads_or(again)) break;                              // (also: every exit is read before one is replaced)
      if (again) {
        used = in;
        got = scan_segment(win, org, hi, own_end, f, s_set, used);
        s_exit[t] = got.exit;
      }
    }
    __syncthreads();
    carry = s_exit[nl - 1];
    // exclusive scan of (blocks, DC sums, failed) over the lanes
    uint32_t v[5] = {got.blocks, got.dc[0], got.dc[1], got.dc[2], got.status != OK ? 1u : 0u};
    const uint32_t own[5] = {v[0], v[1], v[2], v[3], v[4]};
    const int lane = t & (SPNET_WAVE - 1), wave = t / SPNET_WAVE;
#pragma unroll
    for (int off = 1; off < SPNET_WAVE; off <<= 1)
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const uint32_t o = (uint32_t)__shfl_up((int)v[j], off, SPNET_WAVE);
        if (lane >= off) v[j] += o;
      }
    if (lane == SPNET_WAVE - 1)
      for (int j = 0; j < 5; ++j) s_total[wave][j] = v[j];
    __syncthreads();
    uint32_t before[5], all[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      before[j] = v[j] - own[j];
      all[j] = 0;
      for (int w = 0; w < SY_WAVES; ++w) {
        if (w < wave) before[j] += s_total[w][j];
        all[j] += s_total[w][j];
      }
    }
    if (active && before[4] == 0) {
      const uint32_t pred[3] = {pred_base[0] + before[1], pred_base[1] + before[2], pred_base[2] + before[3]};
      const int st = write_segment(win, org, iv, own_end, f, s_set, used, ord_base + before[0], pred, coef);
      if (st != OK) atomicMax(&status[fi], st);                         // (at most one lane of the interval)
    }
    ord_base += all[0];
    pred_base[0] += all[1];
    pred_base[1] += all[2];
    pred_base[2] += all[3];
    if (all[4] != 0 || ord_base >= total) break;                        // (uniform) failed, or every block is written
  }
}

}  // namespace

extern "C" int spnet_jpeg_entropy_sync(const unsigned char* blob, long blob_bytes, const int* intervals, int n_intervals,
                                       const int* files, int n_files, const uint32_t* tables, int n_sets, int seg_bytes,
                                       int16_t* coef, long total_blocks, int* status, void* stream) {
  if (n_intervals < 0 || n_files < 0 || n_sets < 0 || blob_bytes < 0 || blob_bytes > JPEG_MAX_BLOB || total_blocks < 0 ||
      total_blocks > JPEG_MAX_BLOCKS || seg_bytes < SYNC_MIN_SEG || seg_bytes > SYNC_MAX_SEG || (seg_bytes & 3))
    return (int)hipErrorInvalidValue;
  if (n_files == 0 || n_intervals == 0) return 0;
  if (!blob || !intervals || !files || !tables || !coef || !status) return (int)hipErrorInvalidValue;
  if (((uintptr_t)intervals & 3) || ((uintptr_t)files & 3) || ((uintptr_t)tables & 3) || ((uintptr_t)status & 3) ||
      ((uintptr_t)coef & 15))
    return (int)hipErrorInvalidValue;
  const int batch = SY_T < SY_WINDOW / seg_bytes ? SY_T : SY_WINDOW / seg_bytes;           // >= 8
  const size_t lds = SY_WINDOW_AT + 16 + (size_t)batch * seg_bytes + SYNC_READ_AHEAD;
  hipLaunchKernelGGL(jpeg_entropy_sync_kernel, dim3((unsigned)n_intervals), dim3(SY_T), lds, (hipStream_t)stream, blob,
                     blob_bytes, intervals, files, n_files, tables, n_sets, seg_bytes, batch, coef, total_blocks, status);
  SPNET_RETURN_LAUNCH_STATUS();
}
