// The self-synchronising decode of spnet_amd/csrc/jpeg_sync_core.h over plain arrays: what csrc/jpeg_decode_sync.hip's
// workgroup does, with the lanes in a loop -- the same scan_segment / write_segment, the same batches, rounds, prefix sums
// and the same copy of a window of the blob that the lanes read (a heap block of its exact size, as every other array
// here is, so a read past the window, past an interval's bytes or a write past a file's blocks is an AddressSanitizer
// report).  The serial decode_interval of jpeg_decode_core.h runs beside it into a workspace of its own.
//
//   jpeg_sync_host_check PLAN SEG_BYTES LANES
//
// PLAN is tools/jpeg_decode_host_check.cpp's.  Every interval of the plan goes through the emulated workgroup of LANES
// lanes.  Prints, per file: "file N sync S serial T equal E" -- the two statuses (the largest code of the file's
// intervals) and whether the file's blocks of the two workspaces are the same -- and at the end "rounds R": the most
// rounds any batch took.
// Build (the test does): clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "jpeg_sync_core.h"

using namespace jpegdec;

namespace {

template <class T>
T* read_exact(FILE* f, size_t count) {
  T* p = (T*)malloc(count ? count * sizeof(T) : 1);
  if (count && fread(p, sizeof(T), count, f) != count) {
    fprintf(stderr, "plan cut short\n");
    exit(2);
  }
  return p;
}

constexpr int WINDOW_BYTES = 32768;          // the kernel's: a batch is min(lanes, WINDOW_BYTES / seg_bytes) segments

// One interval by `lanes` lanes; returns its status and the rounds of its slowest batch.
int sync_interval(const unsigned char* blob, const int* iv, const int* f, const TableSet& set, int seg_bytes, int lanes,
                  int16_t* coef, int* max_rounds) {
  const int lo = iv[0], hi = iv[1];
  const int nseg = sync_segments(iv, seg_bytes);
  const long total = (long)iv[4] * sync_blocks_per_mcu(f);
  const int batch = lanes < WINDOW_BYTES / seg_bytes ? lanes : WINDOW_BYTES / seg_bytes;
  SyncState* used = (SyncState*)malloc(sizeof(SyncState) * batch);
  SegScan* got = (SegScan*)malloc(sizeof(SegScan) * batch);
  SyncState carry = sync_state(lo, 0, 0, 0);
  long ord_base = 0;
  uint32_t pred_base[3] = {0, 0, 0};
  int status = OK;
  for (int sb = 0; sb < nseg; sb += batch) {
    const int nl = nseg - sb < batch ? nseg - sb : batch;
    const int org = (int)(lo + (long)sb * seg_bytes);
    long wlen = (long)batch * seg_bytes + SYNC_READ_AHEAD;
    if (wlen > hi - org) wlen = hi - org;
    unsigned char* win = (unsigned char*)malloc(wlen > 0 ? (size_t)wlen : 1);
    if (wlen > 0) memcpy(win, blob + org, (size_t)wlen);
    auto own_end = [&](int t) { return sb + t == nseg - 1 ? SYNC_NOWHERE : org + (t + 1) * seg_bytes; };
    for (int t = 0; t < nl; ++t) {
      used[t] = t == 0 ? carry : sync_guess(win, org, hi, org + t * seg_bytes);
      got[t] = scan_segment(win, org, hi, own_end(t), f, set, used[t]);
    }
    int rounds = 0;
    for (; rounds <= nl; ++rounds) {
      bool any = false;
      SyncState before = got[0].exit;                                   // lane t - 1's exit of the round before
      for (int t = 1; t < nl; ++t) {
        const SyncState in = before;
        before = got[t].exit;
        if (sync_same(in, used[t])) continue;
        any = true;
        used[t] = in;
        got[t] = scan_segment(win, org, hi, own_end(t), f, set, in);
      }
      if (!any) break;
    }
    if (rounds > nl) {
      fprintf(stderr, "the chain of %d segments did not settle in %d rounds\n", nl, nl);
      exit(3);
    }
    if (rounds > *max_rounds) *max_rounds = rounds;
    long ord = ord_base;
    uint32_t pred[3] = {pred_base[0], pred_base[1], pred_base[2]};
    bool failed = false;                                                // the true decode, in an earlier lane
    for (int t = 0; t < nl; ++t) {
      if (!failed) {
        const int st = write_segment(win, org, iv, own_end(t), f, set, used[t], ord, pred, coef);
        if (st > status) status = st;
      }
      failed = failed || got[t].status != OK;
      ord += got[t].blocks;
      for (int c = 0; c < 3; ++c) pred[c] += got[t].dc[c];
    }
    carry = got[nl - 1].exit;
    ord_base = ord;
    for (int c = 0; c < 3; ++c) pred_base[c] = pred[c];
    free(win);
    if (failed || ord_base >= total) break;
  }
  free(used);
  free(got);
  return status;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    fprintf(stderr, "usage: %s PLAN SEG_BYTES LANES\n", argv[0]);
    return 2;
  }
  const int seg_bytes = atoi(argv[2]), lanes = atoi(argv[3]);
  if (seg_bytes < SYNC_MIN_SEG || seg_bytes > SYNC_MAX_SEG || seg_bytes % 4 || lanes < 1) {
    fprintf(stderr, "SEG_BYTES is a multiple of 4 in 4 .. 4096, LANES at least 1\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  long long head[8];
  if (fread(head, 8, 8, f) != 8) return 2;
  const long blob_bytes = head[0], total_blocks = head[5];
  const int n_intervals = (int)head[1], n_files = (int)head[2], n_sets = (int)head[3], n_quant = (int)head[4];
  int* intervals = read_exact<int>(f, (size_t)n_intervals * INTERVAL_INTS);
  int* files = read_exact<int>(f, (size_t)n_files * FILE_INTS);
  TableSet* tables = read_exact<TableSet>(f, (size_t)n_sets);
  uint16_t* quant = read_exact<uint16_t>(f, (size_t)n_quant * 64);
  unsigned char* blob = read_exact<unsigned char>(f, (size_t)blob_bytes);
  fclose(f);
  const size_t words = total_blocks ? (size_t)total_blocks * 64 : 1;
  int16_t* coef = (int16_t*)calloc(words, sizeof(int16_t));
  int16_t* serial = (int16_t*)calloc(words, sizeof(int16_t));
  int* status = (int*)calloc(n_files ? n_files : 1, sizeof(int));
  int* serial_status = (int*)calloc(n_files ? n_files : 1, sizeof(int));
  int max_rounds = 0;

  for (int i = 0; i < n_intervals; ++i) {
    const int* iv = intervals + (long)i * INTERVAL_INTS;
    const int fi = iv[2];
    if (fi < 0 || fi >= n_files) continue;
    const int* fr = files + (long)fi * FILE_INTS;
    const int set = fr[F_TABLE_SET];
    int st = BAD_ARGS, ss = BAD_ARGS;
    if (set >= 0 && set < n_sets) {
      ss = decode_interval(blob, blob_bytes, iv, files, n_files, n_sets, tables[set], serial, total_blocks);
      st = sync_interval_ok(blob_bytes, iv, fr, n_sets, total_blocks);
      if (st == OK && iv[4] > 0) st = sync_interval(blob, iv, fr, tables[set], seg_bytes, lanes, coef, &max_rounds);
    }
    if (st > status[fi]) status[fi] = st;
    if (ss > serial_status[fi]) serial_status[fi] = ss;
  }

  for (int n = 0; n < n_files; ++n) {
    const int* fr = files + (long)n * FILE_INTS;
    int equal = 1;
    if (file_ok(fr, n_sets, total_blocks)) {
      const long blocks = (long)fr[F_MCU_W] * fr[F_MCU_H] * sync_blocks_per_mcu(fr);
      equal = memcmp(coef + (long)fr[F_BLOCK0] * 64, serial + (long)fr[F_BLOCK0] * 64, (size_t)blocks * 128) == 0;
    }
    printf("file %d sync %d serial %d equal %d\n", n, status[n], serial_status[n], equal);
  }
  printf("rounds %d\n", max_rounds);
  free(intervals); free(files); free(tables); free(quant); free(blob); free(coef); free(serial); free(status);
  free(serial_status);
  return 0;
}
