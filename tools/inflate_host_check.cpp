// The decode core of spnet_amd/csrc/inflate_core.h over plain arrays: the same state machine and bounds rules that
// csrc/png_decode.hip runs over LDS, as a stand-alone program that host sanitizers can watch.  Buffers are allocated at
// their exact sizes, so a read past a stream's end or a write past its output is an AddressSanitizer report.
//
//   inflate_host_check DIR
//
// DIR/manifest.txt holds one line per stream: "<file> <expected output length>".  For every line the program inflates
// DIR/<file>, prints "<file> <status>" (inflate::Status) and, where the status is 0, writes the bytes to DIR/<file>.out.
// Build (tests/test_png_decode_cpu.py does): clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "inflate_core.h"

namespace {

struct ArrayIO {
  const uint8_t* in;
  int in_len;
  uint8_t* out;
  int out_len;

  uint32_t in32(int pos) {
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
      if (pos + k < in_len) v |= (uint32_t)in[pos + k] << (8 * k);
    return v;
  }
  void put(int op, unsigned byte) { out[op] = (uint8_t)byte; }
  void copy(int op, int dist, int len) {
    for (int k = 0; k < len; ++k) out[op + k] = out[op + k - dist];
  }
  void produced(int) {}
  uint32_t finish(int op) {
    uint32_t a = 1, b = 0;
    for (int i = 0; i < op; ++i) {
      a = (a + out[i]) % 65521u;
      b = (b + a) % 65521u;
    }
    return (b << 16) | a;
  }
};

bool read_file(const std::string& path, std::vector<uint8_t>& data) {
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  data.resize((size_t)(n > 0 ? n : 0));
  const bool ok = n <= 0 || fread(data.data(), 1, (size_t)n, f) == (size_t)n;
  fclose(f);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s DIR\n", argv[0]);
    return 2;
  }
  const std::string dir = argv[1];
  FILE* m = fopen((dir + "/manifest.txt").c_str(), "r");
  if (!m) {
    fprintf(stderr, "no manifest.txt in %s\n", dir.c_str());
    return 2;
  }
  char name[512];
  long want = 0;
  inflate::Tables* tables = new inflate::Tables;
  while (fscanf(m, "%511s %ld", name, &want) == 2) {
    std::vector<uint8_t> data;
    if (!read_file(dir + "/" + name, data) || want < 0 || want > (1L << 27)) {
      fprintf(stderr, "cannot read %s\n", name);
      return 2;
    }
    // exact-size heap blocks (not vectors, whose capacity may exceed their size)
    uint8_t* in = (uint8_t*)malloc(data.size() ? data.size() : 1);
    uint8_t* out = (uint8_t*)malloc(want ? (size_t)want : 1);
    memcpy(in, data.data(), data.size());
    memset(tables, 0, sizeof(*tables));
    ArrayIO io{in, (int)data.size(), out, (int)want};
    const int status = inflate::run(io, *tables, (int)data.size(), (int)want);
    printf("%s %d\n", name, status);
    if (status == 0) {
      FILE* o = fopen((dir + "/" + name + ".out").c_str(), "wb");
      if (!o || fwrite(out, 1, (size_t)want, o) != (size_t)want) {
        fprintf(stderr, "cannot write %s.out\n", name);
        return 2;
      }
      fclose(o);
    }
    free(in);
    free(out);
  }
  fclose(m);
  delete tables;
  return 0;
}
