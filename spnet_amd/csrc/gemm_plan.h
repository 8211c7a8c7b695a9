// Host side of the fp32 GEMM (gemm.hip), first half: WHAT will run for a problem -- every refusal, the operand form, the
// tile, the K split and the main loop -- decided here, before anything is launched.  Plain C++17: no HIP, no kernel, no
// device, so the CPU suite pins it through spnet_gemm_plan (tests/golden/gemm_plans.json).
#pragma once
#include <stdint.h>
#include <algorithm>

#ifndef SP_BK
#define SP_BK 32
#endif
#ifndef SP_PIPE
#define SP_PIPE 1        // 0: the compiler-scheduled main loop everywhere (A/B measurements)
#endif
#ifndef SP_SPLIT_BELOW_TILES
#define SP_SPLIT_BELOW_TILES 256
#define SP_SPLIT_MIN_K 2048
#endif
#ifndef SP_PIPE_MIN_TILES
#define SP_PIPE_MIN_TILES 32
#endif
enum { GEMM_K_MAJOR = 0, GEMM_OUT_MAJOR = 1 };      // = SP_K_MAJOR / SP_OUT_MAJOR of gemm_tile.h
constexpr int GEMM_REFUSED = 1;                     // = hipErrorInvalidValue
static inline int gemm_cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// THE tile table: tile id = row index + 1; BM x BN output tile, WM x WN waves.  gemm_tile(), the launch dispatch of gemm.hip
// and SP_NTILES all derive from it.  Ids outside 1..SP_NTILES ask for the cost model's choice, pick_tile() (C += A B: only 0 does, the others are refused).
struct GemmTile { int id, bm, bn, wm, wn; };
constexpr GemmTile GEMM_TILES[] = {
    {1, 128, 128, 2, 2},   // no pipelined main loop (16 MFMA tiles per wave: no room for a second fragment set)
    {2, 128, 64, 2, 2},
    {3, 64, 64, 2, 2},
    {4, 32, 128, 1, 4},    // problems of at most 32 rows (the Dense head)
    {5, 96, 96, 2, 2},
    {6, 96, 64, 2, 2},
    {7, 64, 128, 2, 2},
    {8, 128, 96, 2, 2},
    // 9 and 10 are never chosen by the cost model: spnet_amd/gemm_tiles.json names the shapes where they win in the step
    {9, 32, 64, 2, 2},     // few-row problems: M = 384 ... 4,096 rows of Inception-ResNet-v2 at batch 16, where 64-row tiles leave CUs empty
    {10, 32, 32, 2, 2},    // the same problems with few columns as well: twice the workgroups, half the MFMA chain per K tile
};
constexpr int SP_NTILES = (int)(sizeof(GEMM_TILES) / sizeof(GEMM_TILES[0]));
constexpr bool gemm_tile_ids_are_dense(int i = 0) { return i == SP_NTILES || (GEMM_TILES[i].id == i + 1 && gemm_tile_ids_are_dense(i + 1)); }
static_assert(gemm_tile_ids_are_dense(), "tile id = row index + 1");
static inline const GemmTile& gemm_tile(int id) { return GEMM_TILES[id - 1]; }      // id in 1..SP_NTILES
// the pipelined main loop exists for tiles of fewer than 16 MFMA tiles per wave (see gemm_f32_kernel)
constexpr bool gemm_can_pipe(int bm, int bn, int wm, int wn) { return SP_PIPE && (bm / wm / 16) * (bn / wn / 16) < 16; }

struct ConvGeom;           // gemm.hip: the geometry of a gathered (implicit-GEMM) A operand
// One GEMM as an entry point states it; every member has the value of "not used".
struct GemmProblem {
  const float *A = nullptr, *B = nullptr;
  float* C = nullptr;
  int a_major = GEMM_K_MAJOR, lda = 0, b_major = GEMM_OUT_MAJOR, ldb = 0, ldc = 0, M = 0, N = 0, K = 0;
  int split_k = 1;                        // K slices; <= 0: auto_split()
  int tile = 0, nbatch = 0, xf = 0, cld = 0, accumulate = 0;      // accumulate: C += A B
  float* workspace = nullptr;             // ws_floats floats for the fp32 slabs of a K split
  long ws_floats = 0;
  const float* bias = nullptr;
  float* colstats = nullptr;              // BatchNorm column sums of C, [*stat_rows][2][N]; stat_rows: host
  int* stat_rows = nullptr;
  const long long* batch = nullptr;       // nbatch problems of this shape: operand offsets {A, B, C} from problem 0
                                          // xf, the                    // A transform: 1 = a*A + b*X2 + c (BatchNorm backward), 2 = relu(a*A + c)
  const float *X2 = nullptr, *coef = nullptr;       // coef = [a | b | c], cld floats each
  float* dy_out = nullptr;                // xf 1: the blended operand, written once
  const ConvGeom* cg = nullptr;           // A is the patch matrix of this convolution, gathered from the NHWC tensor
};
// What runs.  rc != 0: refused, nothing else is meaningful.  form: 0 = K/OUT (forward), 1 = K/K (dgrad), 2 = OUT/OUT
// (wgrad).  nsplit K slices of k_chunk; kslices = the kernel's per-problem slice count (batched problems; else 1).
// to_workspace: the kernel writes nsplit (x nbatch) slabs of `slab` floats, which a reduce launch sums into C.
struct GemmPlan {
  int rc = GEMM_REFUSED, form = 0, tile = 0, bm = 0, bn = 0, nsplit = 1, k_chunk = 0, kslices = 1, pipe = 0, to_workspace = 0, stat_rows = 0;
  long slab = 0;
};

// Automatic K split of one tile shape: enough workgroups for ~2 per CU, slices at least 4 K-tiles deep -- but only
// while the unsplit launch leaves CUs empty: from one workgroup per CU on, the slabs and their reduce launch cost more
// than the second workgroup buys (exit-flow shapes, tile / split sweep: 1536x1024x728 32.8 -> 26.7 us, 1536x1536x1024
// 51.5 -> 43.9, 1536x1536x2048 in the data-gradient form 87.8 -> 74.4), and not below 64 K tiles, where even a launch
// that fills three quarters of the CUs beats its split form (1536x728x1024, data-gradient form: 35.9 -> 29.3 us).
// (weight-gradient form: few output tiles and a long pixel axis by nature; the original rule -- split below two
// workgroups per CU -- measures better there: 1024x1536x1536 53.2 vs 56.7 us)
static int auto_split(long tiles, int M, int N, int K, bool have_ws, long ws_floats, int form) {
  if (!have_ws) return 1;
  if (form == 2 ? tiles >= 512 : (tiles >= SP_SPLIT_BELOW_TILES || K < SP_SPLIT_MIN_K)) return 1;
  const long want = std::min({(512 + tiles - 1) / tiles, std::max(1L, (long)K / (SP_BK * 4)), ws_floats / ((long)M * N)});
  return want > 1 ? (int)want : 1;
}

// Tile choice: cost ~ (workgroups on the busiest CU) x (work per workgroup + a fixed prologue/epilogue worth
// K0 reduction steps) / (measured efficiency of that tile's main loop for this operand form), plus the
// slab traffic of a K split.  The efficiencies were fitted on MI355X to the network's GEMM shapes
// (tools/gemm_sweep.py; every shape of the 512x384 batch-32 step gets its measured-fastest tile) but the
// model itself is shape-agnostic.
static int pick_tile(int form, int M, int N, int K, int split_k, bool have_ws, long ws_floats, int nbatch = 1) {
  if (M <= 32) return 4;
  const int cand[7] = {1, 2, 3, 5, 6, 7, 8};
  static const double eff[3][7] = {{1.00, 0.95, 0.93, 0.93, 0.97, 1.00, 0.93},
                                   {0.95, 0.93, 0.97, 0.97, 1.00, 0.90, 0.99},
                                   {0.80, 0.85, 0.95, 1.00, 0.90, 0.85, 0.80}};
  int best = 1;
  double best_cost = 1e300;
  for (int c = 0; c < 7; ++c) {
    const int bm = gemm_tile(cand[c]).bm, bn = gemm_tile(cand[c]).bn;
    const long tiles = (long)gemm_cdiv(M, bm) * gemm_cdiv(N, bn);
    int ns = split_k > 0 ? split_k : auto_split(tiles, M, N, K, have_ws, ws_floats, form);
    const int kc = gemm_cdiv(gemm_cdiv(K, ns), SP_BK) * SP_BK;
    ns = gemm_cdiv(K, kc);
    const double rounds = (double)((tiles * ns * nbatch + 255) / 256) / nbatch;
    double cost = rounds * bm * bn * ((double)kc + 128.0) / eff[form][c];
    if (ns > 1) cost += 2.0 * ns * (double)M * N / 256.0;
    if (cost < best_cost) { best_cost = cost; best = cand[c]; }
  }
  return best;
}
// The slice count (about three workgroups per CU, slices at least four K tiles deep, at most 64) and the tile that
// spnet_gemm_f32_batched_splitk is meant to be called with for nbatch weight gradients of one shape; 1 = no split.
static long gemm_batched_ksplit(int M, int N, int K, int nbatch, int* tile_out) {
  const GemmTile& t = gemm_tile(N <= 64 ? 6 : 5);    // 96x64 | 96x96
  const long tiles = (long)gemm_cdiv(M, t.bm) * gemm_cdiv(N, t.bn) * (nbatch < 1 ? 1 : nbatch);
  if (tile_out) *tile_out = t.id;
  return std::max(1L, std::min({(768 + tiles - 1) / tiles, std::max(1L, (long)K / (SP_BK * 4)), 64L}));
}
static inline bool gemm_misaligned(const void* a, const void* b = nullptr, const void* c = nullptr) { return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) != 0; }

static GemmPlan gemm_plan(const GemmProblem& p) {
  GemmPlan pl;                       // refused until the last line
  const int M = p.M, N = p.N, K = p.K;
  const bool fwd_form = p.a_major == GEMM_K_MAJOR && p.b_major == GEMM_OUT_MAJOR;
  const bool kk_form = p.a_major == GEMM_K_MAJOR && p.b_major == GEMM_K_MAJOR, oo_form = p.a_major == GEMM_OUT_MAJOR && p.b_major == GEMM_OUT_MAJOR;
  int split_k = p.split_k;           // (the caller's wish, the workspace it comes with: both may be overruled below)
  bool have_ws = p.workspace != nullptr;
  long ws_floats = p.ws_floats;
  if (p.cg && (p.batch || p.xf || p.accumulate || !fwd_form || split_k != 1)) return pl;   // gathered A: one whole forward-form problem
  if (p.accumulate && (p.batch || p.colstats || p.xf || p.tile < 0 || p.tile > SP_NTILES)) return pl;   // C += A B in the epilogue: one plain problem, tile 0 or a row
  if (p.accumulate || p.colstats) split_k = 1;      // ... of whole dot products (no slabs); statistics are taken from such, too
  if (p.batch) {                     // nbatch whole problems side by side; a K split only when the caller asks for one
    if (p.nbatch < 1 || p.bias || p.colstats) return pl;
    if (split_k <= 1 || !have_ws) { split_k = 1; have_ws = false; ws_floats = 0; }
    else if (p.ldc != N) return pl;  // the slab reduce writes dense M x N outputs
  }
  if (M <= 0 || N <= 0 || K <= 0 || (p.lda & 3) || (p.ldb & 3) || (N & 3) || (p.ldc & 3) || gemm_misaligned(p.A, p.B, p.C)) return pl;
  if ((p.a_major == GEMM_K_MAJOR || p.b_major == GEMM_K_MAJOR) && (K & 3)) return pl;      // float4 fetches along the contiguous axis
  if (p.a_major == GEMM_OUT_MAJOR && (M & 3)) return pl;
  // a row stride below the extent it strides over: rows overlap, and for ldc < N workgroups race on their stores
  // (gathered A: lda is the pixel stride of the NHWC tensor, K spans KH*KW pixels -- spnet_conv_gemm_f32 checks ldx >= C)
  if (!p.cg && p.lda < (p.a_major == GEMM_K_MAJOR ? K : M)) return pl;
  if (p.ldb < (p.b_major == GEMM_K_MAJOR ? K : N) || p.ldc < N) return pl;
  if (p.xf) {   // blended A operand: second tensor + [a|b|c] coefficients, zero-padded to whole K tiles; forward form, no K split
    if ((p.xf != 1 && p.xf != 2) || !fwd_form || p.batch || (p.xf == 1 && !p.X2) || !p.coef ||
        gemm_misaligned(p.X2, p.coef, p.dy_out) || (p.cld & 3) || (p.xf == 2 && p.dy_out) || p.cld < gemm_cdiv(K, SP_BK) * SP_BK)
      return pl;
    split_k = 1;
  }
  if (!fwd_form && !kk_form && !oo_form) return pl;               // (no OUT/K kernel)
  pl.form = fwd_form ? 0 : (kk_form ? 1 : 2);
  const int nprob = p.batch ? p.nbatch : 1;
  pl.tile = p.tile;
  if (pl.tile <= 0 || pl.tile > SP_NTILES) {
    pl.tile = pick_tile(pl.form, M, N, K, split_k, have_ws, ws_floats, nprob);
    // the two-tensor blended 128x128 kernel does not fit the register file (it spills); the one-tensor BN+ReLU form (xf 2:
    // 248 VGPRs, no scratch) keeps it -- a 128x96 tile would waste a third of every N = 128 problem of DenseNet
    if (p.xf == 1 && pl.tile == 1) pl.tile = 8;
  }
  const GemmTile& t = gemm_tile(pl.tile);
  pl.bm = t.bm; pl.bn = t.bn; pl.stat_rows = gemm_cdiv(M, t.bm);
  pl.nsplit = split_k > 0 ? split_k : auto_split((long)gemm_cdiv(M, t.bm) * gemm_cdiv(N, t.bn), M, N, K, have_ws, ws_floats, pl.form);
  pl.k_chunk = gemm_cdiv(gemm_cdiv(K, pl.nsplit), SP_BK) * SP_BK;
  pl.nsplit = gemm_cdiv(K, pl.k_chunk);
  if (pl.nsplit > 1) {
    if (!have_ws || (long)pl.nsplit * nprob * M * N > ws_floats || gemm_misaligned(p.workspace)) return pl;
    pl.to_workspace = 1; pl.slab = (long)M * N;
  }
  pl.kslices = p.batch ? pl.nsplit : 1;
  // the pipelined main loop from 32 K tiles per workgroup (see the kernel's header comment)
  pl.pipe = gemm_can_pipe(t.bm, t.bn, t.wm, t.wn) && !p.xf && gemm_cdiv(K < pl.k_chunk ? K : pl.k_chunk, SP_BK) >= SP_PIPE_MIN_TILES;
  pl.rc = 0;
  return pl;
}
