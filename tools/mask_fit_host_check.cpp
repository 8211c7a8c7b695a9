// The labelling of spnet_amd/csrc/mask_fit.hip over plain arrays: what its three launches do, with the workgroups and lanes
// in loops -- the same tile_link_pixel / border_link / find_root / find_slot of csrc/mask_fit_core.h, the same tile, the same
// label form of the parent store (1 + parent, 0 background) -- over heap blocks of their exact size, so that a read or
// write outside a frame, a tile or the slot table is an AddressSanitizer report.  The border jobs of a frame run in a
// seeded random order (no order is promised on the device).  A plain flood fill beside it is the oracle: same labels.
//
//   mask_fit_host_check            the built-in battery; prints "case NAME HxW tol T components N equal 1" per case and
//                                  "all equal" at the end; exit status 1 on the first difference
// Build (the test does): clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -I spnet_amd/csrc
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mask_fit_core.h"

using namespace maskfit;

namespace {

struct LocalStore {                     // phase 1: index form
  int* p;
  int load(int i) const { return p[i]; }
  int fetch_min(int i, int v) const { const int old = p[i]; if (v < old) p[i] = v; return old; }
};

struct LabelStore {                     // phases 2 and 3: label form
  int* lab;
  int load(int i) const { return lab[i] - 1; }
  int fetch_min(int i, int v) const { const int old = lab[i]; if (v + 1 < old) lab[i] = v + 1; return old - 1; }
};

unsigned rng_state = 12345u;
unsigned rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

void label_as_the_device_does(const unsigned char* mask, int H, int W, int tol, int* labels) {
  const int tx_n = (W + TW - 1) / TW, ty_n = (H + TH - 1) / TH;
  // phase 1: every tile on its own
  for (int ty = 0; ty < ty_n; ++ty)
    for (int tx = 0; tx < tx_n; ++tx) {
      unsigned char* val = (unsigned char*)malloc(TILE);
      int* par = (int*)malloc(sizeof(int) * TILE);
      const int x0 = tx * TW, y0 = ty * TH;
      for (int i = 0; i < TILE; ++i) {
        const int x = x0 + i % TW, y = y0 + i / TW;
        val[i] = (x < W && y < H) ? mask[y * W + x] : 0;
        par[i] = i;
      }
      LocalStore st{par};
      for (int tid = 0; tid < TILE / 4; ++tid)
        for (int j = 0; j < 4; ++j) tile_link_pixel(val, st, (tid & 15) * 4 + j, tid >> 4, tol);
      for (int i = 0; i < TILE; ++i) {
        const int x = x0 + i % TW, y = y0 + i / TW;
        if (x < W && y < H) labels[y * W + x] = val[i] ? 1 + tile_to_frame(find_root(st, i, TILE), x0, y0, W) : 0;
      }
      free(val);
      free(par);
    }
  // phase 2: the border jobs of all tiles, shuffled
  const int n_jobs = tx_n * ty_n * BORDER_JOBS;
  int* order = (int*)malloc(sizeof(int) * n_jobs);
  for (int i = 0; i < n_jobs; ++i) order[i] = i;
  for (int i = n_jobs - 1; i > 0; --i) {
    const int j = (int)(rng() % (unsigned)(i + 1)), t = order[i];
    order[i] = order[j];
    order[j] = t;
  }
  LabelStore st{labels};
  for (int k = 0; k < n_jobs; ++k) {
    const int tile = order[k] / BORDER_JOBS, t = order[k] % BORDER_JOBS;
    border_link(mask, st, H, W, tile % tx_n, tile / tx_n, t, tol);
  }
  free(order);
  // phase 3: flatten in place
  for (int p = 0; p < H * W; ++p) {
    const int L = labels[p];
    if (L == 0) continue;
    const int root = find_root(st, L - 1, H * W);
    if (root + 1 != L) labels[p] = root + 1;
  }
}

int flood_fill(const unsigned char* mask, int H, int W, int tol, int* labels) {
  memset(labels, 0, sizeof(int) * H * W);
  int* stack = (int*)malloc(sizeof(int) * H * W);
  int n = 0;
  for (int s = 0; s < H * W; ++s) {
    if (!mask[s] || labels[s]) continue;
    ++n;
    int top = 0;
    stack[top++] = s;
    labels[s] = s + 1;
    while (top) {
      const int p = stack[--top], x = p % W, y = p / W;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = x + dx, yy = y + dy;
          if ((dx || dy) && xx >= 0 && xx < W && yy >= 0 && yy < H) {
            const int q = yy * W + xx;
            if (!labels[q] && joined(mask[p], mask[q], tol)) {
              labels[q] = s + 1;
              stack[top++] = q;
            }
          }
        }
    }
  }
  free(stack);
  return n;
}

// The slot table as mf_compact_kernel fills it and find_slot reads it: every root finds its own slot, nothing else does.
bool slots_ok(const int* labels, int HW, int C) {
  int* firsts = (int*)malloc(sizeof(int) * (C > 0 ? C : 1));
  int m = 0, total = 0;
  for (int p = 0; p < HW; ++p)
    if (labels[p] == p + 1) {
      if (m < C) firsts[m++] = p;
      ++total;
    }
  bool ok = true;
  int rank = 0;
  for (int p = 0; p < HW && ok; ++p) {
    if (labels[p] == 0) continue;
    const int slot = find_slot(firsts, m, labels[p] - 1);
    if (labels[p] == p + 1) {
      ok = slot == (rank < C ? rank : -1);
      ++rank;
    } else {
      ok = slot < 0 ? true : firsts[slot] == labels[p] - 1;
    }
  }
  free(firsts);
  return ok && rank == total;
}

bool run_case(const char* name, const unsigned char* src, int H, int W, int tol) {
  unsigned char* mask = (unsigned char*)malloc((size_t)H * W);          // exact size
  memcpy(mask, src, (size_t)H * W);
  int* got = (int*)malloc(sizeof(int) * H * W);
  int* want = (int*)malloc(sizeof(int) * H * W);
  memset(got, 0xA5, sizeof(int) * H * W);
  label_as_the_device_does(mask, H, W, tol, got);
  const int n = flood_fill(mask, H, W, tol, want);
  const bool equal = memcmp(got, want, sizeof(int) * H * W) == 0 && slots_ok(got, H * W, 128) && slots_ok(got, H * W, 1);
  printf("case %s %dx%d tol %d components %d equal %d\n", name, H, W, tol, n, equal ? 1 : 0);
  free(mask);
  free(got);
  free(want);
  return equal;
}

}  // namespace

int main() {
  static unsigned char buf[200 * 200];
  bool ok = true;
  const int sizes[][2] = {{1, 1}, {1, 200}, {200, 1}, {16, 64}, {33, 130}, {17, 65}, {48, 192}, {100, 200}};
  const int tols[] = {0, 10, 255};
  const int zero_share[] = {0, 50, 90};                  // percent of background
  for (const auto& hw : sizes)
    for (int tol : tols)
      for (int z : zero_share) {
        const int H = hw[0], W = hw[1];
        for (int i = 0; i < H * W; ++i) buf[i] = (int)(rng() % 100u) < z ? 0 : (unsigned char)(10 * (1 + rng() % 3u));
        char name[64];
        snprintf(name, sizeof name, "noise%d", z);
        ok = run_case(name, buf, H, W, tol) && ok;
      }
  {                                                       // a serpentine over every tile of 48 x 192
    const int H = 48, W = 192;
    memset(buf, 0, sizeof buf);
    for (int y = 0; y < H; y += 2) memset(buf + y * W, 60, W);
    for (int y = 1; y < H; y += 2) buf[y * W + ((y / 2) % 2 == 0 ? W - 1 : 0)] = 60;
    ok = run_case("serpentine", buf, H, W, 0) && ok;
  }
  {                                                       // columns, one pixel wide: every tile border is crossed downwards
    const int H = 100, W = 200;
    memset(buf, 0, sizeof buf);
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; x += 2) buf[y * W + x] = (unsigned char)(1 + x / 2);
    ok = run_case("columns", buf, H, W, 0) && ok;
    ok = run_case("columns", buf, H, W, 1) && ok;
  }
  {                                                       // diagonals across the tile corner (64, 16)
    const int H = 33, W = 130;
    memset(buf, 0, sizeof buf);
    buf[15 * W + 63] = buf[16 * W + 64] = 50;
    buf[15 * W + 66] = buf[16 * W + 65] = 50;
    ok = run_case("corners", buf, H, W, 0) && ok;
  }
  if (!ok) return 1;
  printf("all equal\n");
  return 0;
}
