// The decoder of spnet_amd/csrc/jpeg_decode_core.h over plain arrays: the same bit reader, Huffman decoding, rejection rules,
// inverse DCT, upsampling and colour rule that csrc/jpeg_decode.hip runs on the GPU, as a stand-alone program that host
// sanitizers can watch.  Every array is a heap block of its exact size, so a read past an interval's bytes or a write past a
// file's blocks is an AddressSanitizer report.
//
//   jpeg_decode_host_check PLAN OUT
//
// PLAN is what spnet_amd.jpeg.plan_decode builds, as tests/test_jpeg_decode_cpu.py writes it: int64 [8] (blob bytes,
// intervals, files, table sets, quantisation tables, blocks, H, W), then intervals, files, tables, quant and blob as the
// kernels take them.  OUT receives, per file, its status (int32) and, where that is 0, its pixels [H][W][components].
// Build (the test does): clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "jpeg_decode_core.h"

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

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s PLAN OUT\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  FILE* o = fopen(argv[2], "wb");
  if (!f || !o) {
    fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    return 2;
  }
  long long head[8];
  if (fread(head, 8, 8, f) != 8) return 2;
  const long blob_bytes = head[0], total_blocks = head[5];
  const int n_intervals = (int)head[1], n_files = (int)head[2], n_sets = (int)head[3], n_quant = (int)head[4];
  const int H = (int)head[6], W = (int)head[7];
  int* intervals = read_exact<int>(f, (size_t)n_intervals * INTERVAL_INTS);
  int* files = read_exact<int>(f, (size_t)n_files * FILE_INTS);
  TableSet* tables = read_exact<TableSet>(f, (size_t)n_sets);
  uint16_t* quant = read_exact<uint16_t>(f, (size_t)n_quant * 64);
  unsigned char* blob = read_exact<unsigned char>(f, (size_t)blob_bytes);
  fclose(f);
  int16_t* coef = (int16_t*)calloc(total_blocks ? (size_t)total_blocks * 64 : 1, sizeof(int16_t));
  int* status = (int*)calloc(n_files ? n_files : 1, sizeof(int));

  for (int i = 0; i < n_intervals; ++i) {
    const int* iv = intervals + (long)i * INTERVAL_INTS;
    const int fi = iv[2];
    if (fi < 0 || fi >= n_files) continue;
    const int set = files[(long)fi * FILE_INTS + F_TABLE_SET];
    int st = BAD_ARGS;
    if (set >= 0 && set < n_sets)
      st = decode_interval(blob, blob_bytes, iv, files, n_files, n_sets, tables[set], coef, total_blocks);
    if (st > status[fi]) status[fi] = st;
  }

  for (int n = 0; n < n_files; ++n) {
    const int* fr = files + (long)n * FILE_INTS;
    bool ok = status[n] == 0 && file_ok(fr, n_sets, total_blocks);
    const int nc = fr[F_COMPONENTS], hs = fr[F_HS], vs = fr[F_VS], mw = fr[F_MCU_W], mh = fr[F_MCU_H];
    if (ok) ok = mw == (W + 8 * hs - 1) / (8 * hs) && mh == (H + 8 * vs - 1) / (8 * vs);
    for (int c = 0; ok && c < nc; ++c) ok = fr[F_QUANT + c] >= 0 && fr[F_QUANT + c] < n_quant;
    if (!ok && status[n] == 0) status[n] = BAD_ARGS;
    fwrite(&status[n], 4, 1, o);
    if (status[n] != 0) continue;
    unsigned char* plane[3] = {nullptr, nullptr, nullptr};
    int pitch[3] = {0, 0, 0};
    long base = fr[F_BLOCK0];
    for (int c = 0; c < nc; ++c) {
      const int bw = mw * (c == 0 ? hs : 1), bh = mh * (c == 0 ? vs : 1);
      pitch[c] = bw * 8;
      plane[c] = (unsigned char*)malloc((size_t)bw * bh * 64);
      const uint16_t* q = quant + (long)fr[F_QUANT + c] * 64;
      for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
          const int16_t* src = coef + (base + (long)by * bw + bx) * 64;
          int ws[64];
          for (int u = 0; u < 8; ++u) {
            int x[8], out[8];
            for (int v = 0; v < 8; ++v) x[v] = (int)src[v * 8 + u] * (int)q[v * 8 + u];
            idct_1d(x, out, 11);
            for (int v = 0; v < 8; ++v) ws[v * 8 + u] = out[v];
          }
          for (int y = 0; y < 8; ++y) {
            int out[8];
            idct_1d(&ws[y * 8], out, 18);
            for (int x = 0; x < 8; ++x) plane[c][(long)(by * 8 + y) * pitch[c] + bx * 8 + x] = (unsigned char)clamp255(out[x] + 128);
          }
        }
      base += (long)bw * bh;
    }
    unsigned char* px = (unsigned char*)malloc((size_t)H * W * nc);
    const int dw = (W + hs - 1) / hs, dh = (H + vs - 1) / vs;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const int Y = plane[0][(long)y * pitch[0] + x];
        if (nc == 1) {
          px[(long)y * W + x] = (unsigned char)Y;
          continue;
        }
        const unsigned char *p1 = plane[1], *p2 = plane[2];
        const int pc = pitch[1];
        const int cb = chroma_at([&](int r, int c) { return (int)p1[(long)r * pc + c]; }, hs, vs, y, x, dh, dw) - 128;
        const int cr = chroma_at([&](int r, int c) { return (int)p2[(long)r * pc + c]; }, hs, vs, y, x, dh, dw) - 128;
        unsigned char* d = px + ((long)y * W + x) * 3;
        d[0] = (unsigned char)red_of(Y, cr);
        d[1] = (unsigned char)green_of(Y, cb, cr);
        d[2] = (unsigned char)blue_of(Y, cb);
      }
    fwrite(px, 1, (size_t)H * W * nc, o);
    free(px);
    for (int c = 0; c < nc; ++c) free(plane[c]);
  }
  fclose(o);
  free(intervals); free(files); free(tables); free(quant); free(blob); free(coef); free(status);
  return 0;
}
