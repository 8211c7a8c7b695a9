// fp32 MFMA GEMM for the pointwise (1x1) convolutions, the stride-2 residual convs and the Dense head
// (block1_conv2 runs the same tile machinery as implicit GEMMs in conv_gemm.hip):  C[M,N] = sum_k A(m,k) * B(k,n)
//
// Replaces the TensorFlow/cuDNN kernels behind keras SeparableConv2D's pointwise step, Conv2D(1x1)
// and Dense (call sites spnet/models.py:357-359, 388).  Arithmetic is exact f32: the
// v_mfma_f32_16x16x4_f32 instruction is a k-ordered fmaf chain (one rounding per product), so the
// result equals a plain f32 dot product evaluated in k order.
//
// Operand layouts ("major" = which index is contiguous in memory):
//   A  K_MAJOR   : A(m,k) = A[m*lda + k]      (activations [pixels][Cin]: forward, dgrad)
//      OUT_MAJOR : A(m,k) = A[k*lda + m]      (wgrad: A = X^T, read without a transpose pass)
//   B  OUT_MAJOR : B(k,n) = B[k*ldb + n]      (weights [Cin][Cout]: forward; dY in wgrad)
//      K_MAJOR   : B(k,n) = B[n*ldb + k]      (dgrad: B = W^T read in place)
// Each operand's LDS image keeps its own major (see TileStage): no staging pass transposes, and operand
// fetches are conflict-free wide ds_reads (one read feeds up to four MFMAs).
//
// Split-K: grid.z slices write fp32 slabs to a workspace, a second kernel sums them in slice order
// (deterministic; no float atomics).
#include "gemm_tile.h"
#include "gemm_plan.h"
#include <utility>

// 4 waves (WM x WN), each wave owns a (BM/WM) x (BN/WN) block built from 16x16 MFMA tiles
// (v_mfma_f32_16x16x4_f32: D col = l&15, row = 4*(l>>4)+reg).  Tile t+1 travels global -> registers while
// tile t is multiplied, and is written to the idle LDS buffer in the MIDDLE of the MFMA stream (nobody
// reads that buffer during this iteration), so one barrier per K tile suffices.
// AX = 1: the A operand is the blend a[k]*A_ + b[k]*X2_ + c[k] of two tensors (TileStage XF): the BatchNorm-backward
// output dy built on the fly from the incoming gradient g (= A_) and the saved pre-normalisation tensor yp (= X2_),
// coef = [a|b|c] with cld floats each.  dy_out (or NULL): the blended operand is also written to memory once (the
// weight-gradient GEMM of the same layer reads it): K tile t of a row tile is written by the workgroup of column
// tile t % tiles_n, so the extra stores are spread evenly over the workgroups that stage that row tile.
// (blended kernels of the small tiles are held to 3 workgroups per CU like their plain counterparts: the middle
// flow's 768-workgroup launches are exactly one resident wave of 3 per CU)
// AX = 2: the A operand is relu(a[k]*A_ + c[k]) of ONE tensor (TileStage::xform_relu; X2 unused, coefficient row b
// unused): BatchNorm + ReLU applied while the tile is staged, the pre-activation 1x1 convolution of keras DenseNet.

// N x { one MFMA, PER instructions of class MASK } for the instruction scheduler
template <int N, int MASK, int PER>
__device__ __forceinline__ void sp_interleave() {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(MASK, PER, 0);
  }
}

// AG = 1: the A operand is not a matrix in memory but the patch matrix of a convolution, gathered from the NHWC tensor
// while the tile is staged (implicit GEMM): A[m][k] = X[b][oh*s + kh - pt][ow*s + kw - pl][c] with m = (b, oh, ow) and
// k = (kh*KW + kw)*C + c, zero outside the image.  C is a multiple of the K tile (32), so a K tile lies inside ONE tap: the
// tile's fetch is the plain K-major fetch from a shifted base pointer (the row offsets are those of the tap-(0,0) pixels,
// computed once) with the rows whose tap falls outside the image zeroed -- TileStage::load_gather, the same loads in the
// same pipeline slots as the matrix form, no patch matrix, no gather launch.  k runs in the order of the patch matrix,
// so the result has the bits of spnet_patches + spnet_gemm_f32 on the same tile.
struct ConvGeom {
  int H, W, C, KW, stride, pt, pl, OH, OW;      // C == 0: not a convolution
};

// PIPE = 1: the explicitly software-pipelined main loop (below) instead of the compiler-scheduled one.  It needs four
// K tiles of lead-in and pays from about 32 K tiles per workgroup (the weight gradients, the exit flow): measured per
// shape with tools/gemm_table.py, +3..8 % there, -10..20 % on the 2-8-tile GEMMs of the entry flow, equal at 23 tiles.
template <int BM, int BN, int BK, int WM, int WN, int AMAJ, int BMAJ, int AX = 0, int PIPE = 0, int AG = 0>
__global__ __launch_bounds__(256, (AX && BM * BN <= 96 * 64) ? 3 : 2) void gemm_f32_kernel(const float* __restrict__ A_, int lda,
                                                       const float* __restrict__ B_, int ldb,
                                                       float* __restrict__ C_, int ldc, int M, int N,
                                                       int K, int k_chunk, long slab_stride,
                                                       int tiles_m, int tiles_n, int nsplit,
                                                       const float* __restrict__ bias,
                                                       float* __restrict__ colstats,
                                                       const long long* __restrict__ batch,
                                                       const float* __restrict__ X2,
                                                       const float* __restrict__ coef, int cld,
                                                       float* __restrict__ dy_out, int kslices, int accumulate,
                                                       const ConvGeom cg) {
  static_assert(WM * WN == 4, "4 waves per workgroup");
  static_assert(!AG || (!AX && AMAJ == SP_K_MAJOR), "gathered A operands are plain and K-major");
  static_assert(!AX || AMAJ == SP_K_MAJOR, "blended A operands are K-major");
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;
  static_assert(TM >= 1 && TN >= 1 && (BM % (WM * 16)) == 0 && (BN % (WN * 16)) == 0, "wave tile");
  typedef TileStage<BM, BK, AMAJ, TM, 0, AX> SA;
  typedef TileStage<BN, BK, BMAJ, TN, (BMAJ == SP_K_MAJOR)> SB;
  constexpr int STAGE = SA::SIZE + SB::SIZE;
  constexpr int NCH = BK / 16;
  // (+ a two-slot ring of blend coefficients: [a | b | c] x BK floats per K tile)
  constexpr int CFS = 3 * BK;
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE + (AX ? 2 * CFS : 0)];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;

  const int nblk = tiles_m * tiles_n * nsplit;
  int lid = xcd_remap(blockIdx.x, nblk);
  const int gwg = blockIdx.x;
  const int tn = lid % tiles_n;
  lid /= tiles_n;
  const int tm = lid % tiles_m;
  const int z = lid / tiles_m;

  const int m0 = tm * BM, n0 = tn * BN;
  // batch != NULL: grid.z-like index z selects one of nsplit / kslices independent problems of identical shape
  // (operand pointers from the table {A0,B0,C0,A1,B1,C1,...}) and one of its `kslices` K slices; otherwise z is the
  // K slice.  (the table holds element OFFSETS from problem 0's operands, which arrive as kernel arguments: pointers
  // read from memory would be generic and turn every operand fetch into a flat_load, which also counts on
  // lgkmcnt and serialises with the LDS traffic)
  // Batched problems with a K split (kslices > 1) write fp32 slabs: C_ is then the slab workspace, slab z.
  const int bz = batch ? z / kslices : 0;
  const int ks = batch ? z - bz * kslices : z;
  const float* __restrict__ A = batch ? A_ + batch[3 * bz] : A_;
  const float* __restrict__ B = batch ? B_ + batch[3 * bz + 1] : B_;
  float* __restrict__ C = (batch && kslices == 1) ? C_ + batch[3 * bz + 2] : C_;
  const int kbeg = ks * k_chunk;
  const int kend = min(K, kbeg + k_chunk);
  const int nt = (kend - kbeg + BK - 1) / BK;
  const int zs = batch ? (kslices > 1 ? z : 0) : z;     // slab index

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  static_assert(!PIPE || (!AX && TM * TN < 16), "no pipelined form of the blended kernels and of the 128x128 tiles "
                                                "(a second fragment set does not fit their register budget)");
  // Two register stages: while tile t is multiplied, tile t+1 waits in one stage (it is written to the
  // idle LDS buffer in the middle of the MFMA stream) and tile t+2 is already being fetched into the
  // other, so a global load has one and a half K tiles of MFMA time to arrive.
  SA sa[2];
  SB sb[2];
  sa[0].init(lda, m0, M, tid);
  sb[0].init(ldb, n0, N, tid);
#pragma unroll
  for (int i = 0; i < SA::NV; ++i) sa[1].off[i] = sa[0].off[i];
#pragma unroll
  for (int i = 0; i < SB::NV; ++i) sb[1].off[i] = sb[0].off[i];
  // Gathered A: per slot, the element offset of the slot's output pixel at tap (0,0) without padding (lda = the pixel
  // stride of X) and that pixel's input row / column, from which a tap's validity follows.
  int goff[AG ? SA::NV : 1], gh[AG ? SA::NV : 1], gw[AG ? SA::NV : 1];
  if constexpr (AG) {
    static_assert(SA::TOTAL % 256 == 0, "whole float4 slots per thread");
#pragma unroll
    for (int i = 0; i < SA::NV; ++i) {
      const int f = tid + i * 256;
      const int r = min(m0 + f / (BK / 4), M - 1);
      const int ow = r % cg.OW, t2 = r / cg.OW;
      const int oh = t2 % cg.OH, b = t2 / cg.OH;
      gh[i] = oh * cg.stride;
      gw[i] = ow * cg.stride;
      goff[i] = ((b * cg.H + gh[i]) * cg.W + gw[i]) * lda + (f % (BK / 4)) * 4;
    }
  }
  // The K tiles of a problem are fetched in order (prologue: tiles 0, 1 (, 2, 3); step t: tile t+2 or t+4), so the tap
  // of the next tile is running state -- a few scalar adds per tile; dividing k0 by C and KW on every fetch costs as
  // much as the gather launch it replaces.
  int g_c0 = 0, g_kw = 0, g_dh = -cg.pt, g_dw = -cg.pl;
  auto gather_a = [&](auto& stA, int k0) {          // the next K tile of the patch matrix (inside one tap)
    if constexpr (AG) {
      const int shift = (g_dh * cg.W + g_dw) * lda + g_c0;
      unsigned ok = 0;
#pragma unroll
      for (int i = 0; i < SA::NV; ++i)
        ok |= (unsigned)((unsigned)(gh[i] + g_dh) < (unsigned)cg.H && (unsigned)(gw[i] + g_dw) < (unsigned)cg.W) << i;
      stA.load_gather(A, goff, shift, k0 < kend ? ok : 0u);
      g_c0 += BK;
      if (g_c0 == cg.C) {
        g_c0 = 0;
        ++g_kw;
        ++g_dw;
        if (g_kw == cg.KW) {
          g_kw = 0;
          g_dw = -cg.pl;
          ++g_dh;
        }
      }
    }
  };

  // Blended A operand: tile t+1 waits in its register stage as TWO raw tensors (v = g, w = yp); it is blended -- and,
  // by the column tile whose turn it is, written out as dy -- at the START of step t, before tile t+2's fetch
  // reuses the one shared w set.  The blend coefficients of a K tile (3 x BK floats) travel like the tile itself:
  // fetched by 3*BK/4 threads two tiles ahead, parked in a two-slot LDS ring in the middle of the step, read back
  // (three broadcast ds_read_b128 per thread) one barrier later -- a global load right in front of the blend
  // would put an L2 round trip on every wave's critical path once per K tile.
  float4 wsh[AX ? SA::NV : 1];
  float4 cfreg = make_float4(0.f, 0.f, 0.f, 0.f);
  constexpr int CFT = 3 * BK / 4;                      // coefficient float4 per K tile
  float* cfs = smem + 2 * STAGE;
  auto cf_fetch = [&](int k0) {                        // this thread's share of tile k0's coefficients
    if constexpr (AX)
      if (tid < CFT) cfreg = *reinterpret_cast<const float4*>(coef + (tid / (BK / 4)) * cld + k0 + (tid % (BK / 4)) * 4);
  };
  auto cf_park = [&](int slot) {
    if constexpr (AX)
      if (tid < CFT) *reinterpret_cast<float4*>(cfs + slot * CFS + tid * 4) = cfreg;
  };
  auto fetch = [&](auto& stA, auto& stB, int k0, auto& wreg) {      // any tile: predicated
    if constexpr (AX == 1) stA.load2(A, X2, lda, m0, M, k0, kend, tid, wreg);
    else if constexpr (AG) gather_a(stA, k0);
    else stA.load(A, lda, m0, M, k0, kend, tid);
    stB.load(B, ldb, n0, N, k0, kend, tid);
  };
  auto blend = [&](auto& stA, int k0, auto& wreg, const float4 a, const float4 b, const float4 c) {
    if constexpr (AX == 2) {
      stA.xform_relu(a, c);
    } else if constexpr (AX) {
      stA.xform(a, b, c, wreg);
      if (dy_out && ((k0 - kbeg) / BK) % tiles_n == tn) stA.store_global(dy_out, K, m0, M, k0, kend, tid);      // dense [M][K], whatever lda
    }
  };
  if (nt > 0) {
    if constexpr (AX) {
      float4 w0[SA::NV];
      const int kq4 = (tid % (BK / 4)) * 4;
      fetch(sa[0], sb[0], kbeg, w0);
      if (nt > 1) {
        fetch(sa[1], sb[1], kbeg + BK, wsh);
        cf_fetch(kbeg + BK);
      }
      blend(sa[0], kbeg, w0, *reinterpret_cast<const float4*>(coef + kbeg + kq4),
            *reinterpret_cast<const float4*>(coef + cld + kbeg + kq4),
            *reinterpret_cast<const float4*>(coef + 2 * cld + kbeg + kq4));
      if (nt > 1) cf_park(1);
    } else {
      fetch(sa[0], sb[0], kbeg, wsh);
      if (nt > 1) fetch(sa[1], sb[1], kbeg + BK, wsh);
    }
    sa[0].store(smem, tid);
    sb[0].store(smem + SA::SIZE, tid);
    if constexpr (PIPE) {                          // tiles 0 and 1 in LDS, tiles 2 and 3 on their way into the stages
      if (nt > 1) {
        sa[1].store(smem + STAGE, tid);
        sb[1].store(smem + STAGE + SA::SIZE, tid);
      }
      if (nt > 2) fetch(sa[0], sb[0], kbeg + 2 * BK, wsh);
      if (nt > 3) fetch(sa[1], sb[1], kbeg + 3 * BK, wsh);
    }
  }
  __syncthreads();

  // PAR = t & 1: tile t sits in LDS buffer PAR, tile t+1 in register stage 1-PAR, stage PAR is free.
  // FULL: tile t+2 exists and lies completely below kend -> its fetch is branch-free, the whole step is one
  // basic block and the compiler interleaves loads, LDS writes and MFMAs.
  const long aoff = (AMAJ == SP_K_MAJOR ? (long)kbeg : (long)kbeg * lda) + (PIPE ? 4 : 2) * SA::kstep(lda);
  const long boff = (BMAJ == SP_K_MAJOR ? (long)kbeg : (long)kbeg * ldb) + (PIPE ? 4 : 2) * SB::kstep(ldb);
  const float* Ak = A + aoff;
  const float* Bk = B + boff;
  const float* Xk = (AX == 1) ? X2 + aoff : nullptr;      // second tensor of the blended operand
  // Plain (AX = 0) kernels: the main loop is an explicit software pipeline over the two 16-deep chunks of a K tile.
  // Per step t (LDS buffer cur = t & 1 holds tile t; two register stages, stage t & 1 holds tile t+2):
  //   first half    fragments of chunk 1 (cur) -> set 1  |  MFMAs of chunk 0 on set 0
  //   barrier       (every wave has its last fragments of cur; tile t+1 is complete in nxt)
  //   second half   fragments of chunk 0 of tile t+1 (nxt) -> set 0 | stage (tile t+2) -> cur | global loads of tile
  //                 t+4 -> the same stage  |  MFMAs of chunk 1 on set 1
  // Every LDS fragment read is issued a chunk (>= 16 MFMAs) ahead of its first use, the stage is written to LDS TWO
  // steps after its global loads were issued (measured with the loads, the stage stores or the fragment reads knocked
  // out: with ONE step of cover the waves stall 0.5 us per step in front of the stage stores, waiting for
  // first-touch lines of the A operand) and a full step before the barrier that publishes it, so a wave
  // reaches the barrier with nothing outstanding and leaves it with a chunk of MFMAs ready to issue.  The
  // sched_group_barrier sequences pin that order in the branch-free FULL step and spread the LDS / global
  // instructions one per MFMA (an MFMA occupies the SIMD's issue port for 8 of its 32 cycles): left alone, hipcc
  // issues every fragment read directly in front of its first MFMA and sinks the global loads to the end of a step.
  static_assert(NCH == 2, "the pipelined step is written for two chunks per K tile");
  float fa[2][TM][4], fb[2][TN][4];
  constexpr int NMF = TM * TN * 4;                   // MFMAs per chunk
  constexpr int NLD = SA::NV + SB::NV;               // global loads = LDS stores per tile and thread
  constexpr int NFR = SA::NFR + SB::NFR;             // fragment reads per chunk (before ds_read2 merging)
  constexpr int PER = (NFR + 2 * NLD <= NMF) ? 1 : 2;   // LDS / global instructions per MFMA in the interleave
  auto frd0 = [&](const float* buf, int c) {
    SA::frags(buf, wm * (TM * 16), lane, c, fa[0]);
    SB::frags(buf + SA::SIZE, wn * (TN * 16), lane, c, fb[0]);
  };
  auto frd1 = [&](const float* buf, int c) {
    SA::frags(buf, wm * (TM * 16), lane, c, fa[1]);
    SB::frags(buf + SA::SIZE, wn * (TN * 16), lane, c, fb[1]);
  };
  auto mma0 = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[0][i][q], fb[0][j][q], acc[i][j], 0, 0, 0);
  };
  auto mma1 = [&]() {
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[1][i][q], fb[1][j][q], acc[i][j], 0, 0, 0);
  };
  auto pstep = [&](auto par, auto full, int t) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool FULL = decltype(full)::value;   // tile t+4 exists and lies completely below kend
    float* cur = smem + PAR * STAGE;
    const float* nxt = smem + (1 - PAR) * STAGE;
    frd1(cur, 1);
    mma0();
    if (FULL) {
      sp_interleave<(NFR + PER - 1) / PER, 0x100, PER>();
      __builtin_amdgcn_sched_group_barrier(0x008, NMF, 0);
      __builtin_amdgcn_sched_barrier(0);           // nothing crosses: chunk 0 is multiplied in front of the barrier
    }
    __syncthreads();
    if (FULL) __builtin_amdgcn_sched_barrier(0);
    if (FULL || t + 1 < nt) frd0(nxt, 0);
    if (FULL || t + 2 < nt) {
      sa[PAR].store(cur, tid);
      sb[PAR].store(cur + SA::SIZE, tid);
    }
    if (FULL) {
      if constexpr (AG) gather_a(sa[PAR], kbeg + (t + 4) * BK);
      else sa[PAR].load_full(Ak);
      sb[PAR].load_full(Bk);
      Ak += SA::kstep(lda);
      Bk += SB::kstep(ldb);
    } else if (t + 4 < nt) {
      fetch(sa[PAR], sb[PAR], kbeg + (t + 4) * BK, wsh);
    }
    mma1();
    if (FULL) {
      sp_interleave<(NFR + PER - 1) / PER, 0x100, PER>();
      sp_interleave<(NLD + PER - 1) / PER, 0x200, PER>();
      sp_interleave<(NLD + PER - 1) / PER, 0x020, PER>();
      __builtin_amdgcn_sched_group_barrier(0x008, NMF, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  auto step = [&](auto par, auto full, int t) {
    constexpr int PAR = decltype(par)::value;
    constexpr bool FULL = decltype(full)::value;
    const float* cur = smem + PAR * STAGE;
    float* nxt = smem + (1 - PAR) * STAGE;
    const bool more = FULL || (t + 1 < nt);
    if constexpr (AX) {
      if (more) {
        const float4* cs = reinterpret_cast<const float4*>(cfs + (1 - PAR) * CFS) + tid % (BK / 4);
        blend(sa[1 - PAR], kbeg + (t + 1) * BK, wsh, cs[0], cs[BK / 4], cs[2 * (BK / 4)]);
      }
      if (FULL || t + 2 < nt) cf_fetch(kbeg + (t + 2) * BK);
    }
    if (FULL) {
      if constexpr (AX == 1) sa[PAR].load_full2(Ak, Xk, wsh);
      else if constexpr (AG) gather_a(sa[PAR], kbeg + (t + 2) * BK);
      else sa[PAR].load_full(Ak);
      sb[PAR].load_full(Bk);
      Ak += SA::kstep(lda);
      Bk += SB::kstep(ldb);
      if constexpr (AX == 1) Xk += SA::kstep(lda);
    } else if (t + 2 < nt) {
      fetch(sa[PAR], sb[PAR], kbeg + (t + 2) * BK, wsh);
    }
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      if (c == NCH / 2 && more) {
        sa[1 - PAR].store(nxt, tid);
        sb[1 - PAR].store(nxt + SA::SIZE, tid);
        if (FULL || t + 2 < nt) cf_park(PAR);          // coefficients of tile t+2 (slot parity of t+2 = PAR)
      }
      float a[TM][4], b[TN][4];
      SA::frags(cur, wm * (TM * 16), lane, c, a);
      SB::frags(cur + SA::SIZE, wn * (TN * 16), lane, c, b);
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i][q], b[j][q], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  };
  typedef std::integral_constant<int, 0> P0;
  typedef std::integral_constant<int, 1> P1;
  const int nfull = (kend - kbeg) / BK;            // complete K tiles of this slice
  int t = 0;
  if constexpr (PIPE)
    if (nt > 0) frd0(smem, 0);                     // fragments of tile 0, chunk 0
  if constexpr (!PIPE) {
    for (; t + 3 < nfull; t += 2) {                // tiles t+2 and t+3 are complete
      step(P0(), std::true_type(), t);
      step(P1(), std::true_type(), t + 1);
    }
    for (; t < nt; t += 2) {
      step(P0(), std::false_type(), t);
      if (t + 1 < nt) step(P1(), std::false_type(), t + 1);
    }
  } else {
    for (; t + 5 < nfull; t += 2) {                // tiles t+4 and t+5 are complete
      pstep(P0(), std::true_type(), t);
      pstep(P1(), std::true_type(), t + 1);
    }
    for (; t < nt; t += 2) {
      pstep(P0(), std::false_type(), t);
      if (t + 1 < nt) pstep(P1(), std::false_type(), t + 1);
    }
  }

  gemm_epilogue<SA, SB, BM, BN, WM, WN, TM, TN>(acc, smem, C, ldc, M, N, m0, n0, tm, zs, slab_stride, bias, colstats,
                                                tid, lane, wm, wn, accumulate);
}

// out[row*ldc + col] = sum_z ws[z*M*N + row*N + col] (+ bias[col]); N % 4 == 0, ldc % 4 == 0.
// Workgroup = (256 / sl) output float4 x sl slab lanes (sl = 1..16, a power of two chosen from the slab count):
// lane g adds slabs g, g+sl, g+2sl, ... (up to 4 loads in flight), then the sl lane sums are added in lane
// order -- a fixed order, and a K split into hundreds of slabs (the weight gradients of the entry flow:
// K = 372,000 pixels) is no longer one long serial chain per output element.
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const float* __restrict__ ws, int nslab,
                                                           int M, int N, float* __restrict__ out,
                                                           int ldc, const float* __restrict__ bias, int sl) {
  __shared__ float4 red[256];
  const long total4 = (long)M * N / 4;
  const long mn = (long)M * N;
  const int per = 256 / sl;                         // outputs per workgroup
  const int lane = threadIdx.x % per, g = threadIdx.x / per;
  const long i = (long)blockIdx.x * per + lane;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < total4) {
#pragma unroll 4
    for (int zz = g; zz < nslab; zz += sl) {
      const float4 t = *reinterpret_cast<const float4*>(ws + (long)zz * mn + i * 4);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
  }
  red[g * per + lane] = s;
  __syncthreads();
  if (g == 0 && i < total4) {
    float4 t = red[lane];
    for (int k = 1; k < sl; ++k) {
      const float4 v = red[k * per + lane];
      t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    const long e = i * 4;
    const int row = (int)(e / N), col = (int)(e % N);
    if (bias) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + col);
      t.x += bv.x; t.y += bv.y; t.z += bv.z; t.w += bv.w;
    }
    *reinterpret_cast<float4*>(out + (long)row * ldc + col) = t;
  }
}

static void launch_reduce_slabs(const float* ws, int nslab, int M, int N, float* out, int ldc, const float* bias,
                                hipStream_t st) {
  const long total4 = (long)M * N / 4;
  int sl = 1;
  while (sl < 16 && sl * 4 <= nslab) sl <<= 1;      // >= 4 slabs per lane before another lane pays off
  const int per = 256 / sl;
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((total4 + per - 1) / per)), dim3(256), 0, st, ws, nslab, M, N,
                     out, ldc, bias, sl);
}

// out[M][ldc] = sum of nslab slabs of M*N floats (slice order); shared with conv_gemm.hip
extern "C" int spnet_reduce_slabs(const float* ws, int nslab, int M, int N, float* out, int ldc, void* stream) {
  if ((N & 3) || (ldc & 3) || nslab < 1) return (int)hipErrorInvalidValue;
  launch_reduce_slabs(ws, nslab, M, N, out, ldc, nullptr, (hipStream_t)stream);
  SPNET_RETURN_LAUNCH_STATUS();
}

// out_j[i] = sum over the kslices slabs of problem j, slice order (deterministic); out_j = C0 + offsets[3j + 2].
__global__ __launch_bounds__(256) void reduce_slabs_batched_kernel(const float* __restrict__ ws, int kslices, long mn,
                                                                   float* __restrict__ C0,
                                                                   const long long* __restrict__ offsets) {
  const int j = blockIdx.y;
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= mn) return;
  const float* p = ws + (long)j * kslices * mn + i;
  float4 s = *reinterpret_cast<const float4*>(p);
  for (int k = 1; k < kslices; ++k) {
    const float4 t = *reinterpret_cast<const float4*>(p + (long)k * mn);
    s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
  }
  *reinterpret_cast<float4*>(C0 + offsets[3 * j + 2] + i) = s;
}

static_assert((int)GEMM_K_MAJOR == (int)SP_K_MAJOR && (int)GEMM_OUT_MAJOR == (int)SP_OUT_MAJOR && GEMM_REFUSED == (int)hipErrorInvalidValue,
              "gemm_plan.h restates the majors of gemm_tile.h and hipErrorInvalidValue");

// Launch: executes the GemmPlan of a GemmProblem (gemm_plan.h), where every refusal and every choice has been made.
// launch_form: one operand form of one tile; PIPE from the plan, where the tile and the form have a pipelined kernel.
template <int BM, int BN, int WM, int WN, int AMAJ, int BMAJ, int AX, int AG>
static void launch_form(const GemmProblem& p, const GemmPlan& pl, hipStream_t st) {
  const ConvGeom cg = p.cg ? *p.cg : ConvGeom{0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int tm = spnet_cdiv(p.M, BM), tn = spnet_cdiv(p.N, BN);
  const int nz = p.batch ? p.nbatch * pl.kslices : pl.nsplit;      // the kernel's slice index selects (problem, K slice)
  const bool ws = pl.to_workspace;                                 // slabs: dense M x N, the reduce launch adds the bias
  auto launch = [&](auto pipe) {
    hipLaunchKernelGGL((gemm_f32_kernel<BM, BN, SP_BK, WM, WN, AMAJ, BMAJ, AX, decltype(pipe)::value, AG>), dim3(tm * tn * nz),
                       dim3(256), 0, st, p.A, p.lda, p.B, p.ldb, ws ? p.workspace : p.C, ws ? p.N : p.ldc, p.M, p.N, p.K,
                       pl.k_chunk, pl.slab, tm, tn, nz, ws ? nullptr : p.bias, p.colstats, p.batch, p.X2, p.coef, p.cld,
                       p.dy_out, pl.kslices, p.accumulate, cg);
  };
  if constexpr (gemm_can_pipe(BM, BN, WM, WN) && !AX) {
    if (pl.pipe) return launch(std::integral_constant<int, 1>());
  }
  launch(std::integral_constant<int, 0>());
}

// gathered (AG) and transformed (AX) A operands exist in the forward operand form only
template <int BM, int BN, int WM, int WN>
static void launch_tile(const GemmProblem& p, const GemmPlan& pl, hipStream_t st) {
  if (p.cg) launch_form<BM, BN, WM, WN, SP_K_MAJOR, SP_OUT_MAJOR, 0, 1>(p, pl, st);
  else if (p.xf == 1) launch_form<BM, BN, WM, WN, SP_K_MAJOR, SP_OUT_MAJOR, 1, 0>(p, pl, st);
  else if (p.xf == 2) launch_form<BM, BN, WM, WN, SP_K_MAJOR, SP_OUT_MAJOR, 2, 0>(p, pl, st);
  else if (pl.form == 0) launch_form<BM, BN, WM, WN, SP_K_MAJOR, SP_OUT_MAJOR, 0, 0>(p, pl, st);
  else if (pl.form == 1) launch_form<BM, BN, WM, WN, SP_K_MAJOR, SP_K_MAJOR, 0, 0>(p, pl, st);
  else launch_form<BM, BN, WM, WN, SP_OUT_MAJOR, SP_OUT_MAJOR, 0, 0>(p, pl, st);
}

template <size_t... I>     // launch_tile<BM, BN, WM, WN> of the plan's row of GEMM_TILES
static void launch_planned_tile(const GemmProblem& p, const GemmPlan& pl, hipStream_t st, std::index_sequence<I...>) {
  ((pl.tile == GEMM_TILES[I].id
        ? launch_tile<GEMM_TILES[I].bm, GEMM_TILES[I].bn, GEMM_TILES[I].wm, GEMM_TILES[I].wn>(p, pl, st) : void()), ...);
}

static int gemm_impl(const GemmProblem& p, void* stream) {
  const GemmPlan pl = gemm_plan(p);
  if (pl.rc) return pl.rc;
  hipStream_t st = (hipStream_t)stream;
  if (p.stat_rows) *p.stat_rows = pl.stat_rows;
  launch_planned_tile(p, pl, st, std::make_index_sequence<SP_NTILES>());
  if (pl.to_workspace && !p.batch) launch_reduce_slabs(p.workspace, pl.nsplit, p.M, p.N, p.C, p.ldc, p.bias, st);
  if (pl.to_workspace && p.batch)
    hipLaunchKernelGGL(reduce_slabs_batched_kernel, dim3((unsigned)((pl.slab / 4 + 255) / 256), p.nbatch), dim3(256), 0, st,
                       p.workspace, pl.kslices, pl.slab, p.C, p.batch);
  SPNET_RETURN_LAUNCH_STATUS();
}

// Entry points (documented in include/spnet_hip.h).  gemm_problem: the operands each of them has; the rest it sets by name.
static GemmProblem gemm_problem(const float* A, int a_major, int lda, const float* B, int b_major, int ldb, float* C, int ldc, int M, int N, int K, int tile) {
  GemmProblem p;
  p.A = A; p.a_major = a_major; p.lda = lda; p.B = B; p.b_major = b_major; p.ldb = ldb; p.C = C; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K; p.tile = tile;
  return p;
}

extern "C" int spnet_gemm_f32(const float* A, int a_major, int lda, const float* B, int b_major, int ldb, float* C, int ldc, int M,
                              int N, int K, int split_k, float* workspace, long ws_floats, const float* bias, int tile, void* stream) {
  GemmProblem p = gemm_problem(A, a_major, lda, B, b_major, ldb, C, ldc, M, N, K, tile);
  p.split_k = split_k; p.workspace = workspace; p.ws_floats = ws_floats; p.bias = bias;
  return gemm_impl(p, stream);
}

// plan[10] = {form, tile, bm, bn, nsplit, k_chunk, kslices, pipe, to_workspace, stat_rows} for dense, aligned operands
extern "C" int spnet_gemm_plan(int a_major, int b_major, int M, int N, int K, int split_k, int have_workspace, long ws_floats,
                               int have_colstats, int have_batch, int nbatch, int xf, int accumulate, int conv, int tile, int* plan) {
  float* const mem = reinterpret_cast<float*>(64);         // tested for NULL and alignment, never dereferenced
  GemmProblem p = gemm_problem(mem, a_major, a_major == SP_K_MAJOR ? K : M, mem, b_major, b_major == SP_K_MAJOR ? K : N, mem, N, M, N, K, tile);
  p.split_k = split_k; p.workspace = have_workspace ? mem : nullptr; p.ws_floats = ws_floats;
  p.batch = have_batch ? reinterpret_cast<const long long*>(mem) : nullptr; p.nbatch = nbatch;
  p.xf = xf; p.X2 = xf == 1 ? mem : nullptr; p.coef = xf ? mem : nullptr; p.cld = spnet_cdiv(K, SP_BK) * SP_BK;
  p.accumulate = accumulate; p.colstats = have_colstats ? mem : nullptr;
  p.cg = conv ? reinterpret_cast<const ConvGeom*>(mem) : nullptr;
  const GemmPlan pl = gemm_plan(p);
  const int v[10] = {pl.form, pl.tile, pl.bm, pl.bn, pl.nsplit, pl.k_chunk, pl.kslices, pl.pipe, pl.to_workspace, pl.stat_rows};
  for (int i = 0; i < 10 && !pl.rc; ++i) plan[i] = v[i];
  return pl.rc;
}

// C += A B (no K split: the sum is formed in the epilogue, read-modify-write of C by the workgroup that owns the tile)
// instead of a GEMM into a scratch tensor + an accumulation pass
extern "C" int spnet_gemm_f32_accumulate(const float* A, int a_major, int lda, const float* B, int b_major, int ldb,
                                         float* C, int ldc, int M, int N, int K, int tile, void* stream) {
  GemmProblem p = gemm_problem(A, a_major, lda, B, b_major, ldb, C, ldc, M, N, K, tile);
  p.accumulate = 1;
  return gemm_impl(p, stream);
}

// nbatch problems of one shape in ONE launch: the weight gradients of the eight middle-flow blocks, each too small to fill the chip
extern "C" int spnet_gemm_f32_batched(const float* A0, const float* B0, float* C0, const long long* offsets, int nbatch, int a_major,
                                      int lda, int b_major, int ldb, int ldc, int M, int N, int K, int tile, void* stream) {
  if (!offsets || !A0 || !B0 || !C0) return (int)hipErrorInvalidValue;
  GemmProblem p = gemm_problem(A0, a_major, lda, B0, b_major, ldb, C0, ldc, M, N, K, tile);
  p.batch = offsets; p.nbatch = nbatch;
  return gemm_impl(p, stream);
}

// The same with every problem's K axis cut into `ksplit` slices (fp32 slabs, summed per problem in slice order by one more launch):
// weight gradients too small to fill the chip even side by side -- the repeated blocks of Inception-ResNet-v2 at batch 16
extern "C" long spnet_gemm_batched_ksplit(int M, int N, int K, int nbatch, int* tile_out) { return gemm_batched_ksplit(M, N, K, nbatch, tile_out); }
extern "C" int spnet_gemm_f32_batched_splitk(const float* A0, const float* B0, float* C0, const long long* offsets, int nbatch,
                                             int a_major, int lda, int b_major, int ldb, int ldc, int M, int N, int K, int tile,
                                             int ksplit, float* workspace, long ws_floats, void* stream) {
  if (!offsets || !A0 || !B0 || !C0) return (int)hipErrorInvalidValue;
  if (ksplit > 1 && (!workspace || (((uintptr_t)workspace) & 15))) return (int)hipErrorInvalidValue;
  GemmProblem p = gemm_problem(A0, a_major, lda, B0, b_major, ldb, C0, ldc, M, N, K, tile);
  p.batch = offsets; p.nbatch = nbatch;
  p.split_k = ksplit > 1 ? ksplit : 1; p.workspace = workspace; p.ws_floats = ws_floats;
  return gemm_impl(p, stream);
}

// dX = dY B with dY = a[k]*g + b[k]*yp + c[k], the BatchNorm-backward output, blended while the A tile is staged (AX = 1;
// forward operand form: B = W^T kept by the engine).
extern "C" int spnet_gemm_f32_bnblend(const float* g, const float* yp, const float* coef, int cld, int lda, const float* B, int ldb,
                                      float* C, int ldc, int M, int N, int K, int tile, float* dy_out, void* stream) {
  GemmProblem p = gemm_problem(g, SP_K_MAJOR, lda, B, SP_OUT_MAJOR, ldb, C, ldc, M, N, K, tile);
  p.xf = 1; p.X2 = yp; p.coef = coef; p.cld = cld; p.dy_out = dy_out;
  return gemm_impl(p, stream);
}

// Y = relu(x[:, :K]*scale + shift) W with the BatchNorm + ReLU of every input channel applied while the A tile is staged (AX = 2):
// keras DenseNet121's 1x1 convolutions read the first K channels of their block's Concatenate buffer (pixels ldx floats apart)
extern "C" int spnet_gemm_f32_bnrelu(const float* x, int ldx, const float* coef, int cld, const float* W, int ldw, float* Y, int ldy,
                                     int M, int N, int K, int tile, float* colstats, int* stat_rows, void* stream) {
  if (!x || !W || !Y || (!colstats) != (!stat_rows) || ldx < K) return (int)hipErrorInvalidValue;
  GemmProblem p = gemm_problem(x, SP_K_MAJOR, ldx, W, SP_OUT_MAJOR, ldw, Y, ldy, M, N, K, tile);
  p.xf = 2; p.coef = coef; p.cld = cld; p.colstats = colstats; p.stat_rows = stat_rows;
  return gemm_impl(p, stream);
}

extern "C" int spnet_gemm_f32_colstats(const float* A, int a_major, int lda, const float* B, int b_major, int ldb, float* C, int ldc,
                                       int M, int N, int K, int tile, float* colstats, int* stat_rows, void* stream) {
  if (!colstats || !stat_rows) return (int)hipErrorInvalidValue;
  GemmProblem p = gemm_problem(A, a_major, lda, B, b_major, ldb, C, ldc, M, N, K, tile);
  p.colstats = colstats; p.stat_rows = stat_rows;
  return gemm_impl(p, stream);
}

// The forward convolution of an NHWC tensor as an implicit GEMM on the same kernel: y[B*OH*OW][Cout] = patches(x) * Wk,
// Wk = the HWIO kernel read as [KH*KW*C][Cout], the patch matrix never written (AG = 1 above).  x pixels are ldx floats
// apart (ldx >= C: x may be a column block of a wider tensor); C % 32 == 0; stride 1 or 2; `same` = TF SAME padding, else
// VALID.  bias (or NULL) is added in the epilogue; colstats / stat_rows (or NULL / NULL) as spnet_gemm_f32_colstats.
// Bit-identical to spnet_patches + spnet_gemm_f32(_colstats) with the same tile.
extern "C" int spnet_conv_gemm_f32(const float* x, long ldx, const float* Wk, float* y, int ldy, int B, int H, int W,
                                   int C, int Cout, int KH, int KW, int stride, int same, const float* bias, int tile,
                                   float* colstats, int* stat_rows, void* stream) {
  if (!x || !Wk || !y || B < 1 || H < 1 || W < 1 || KH < 1 || KW < 1 || (stride != 1 && stride != 2)) return (int)hipErrorInvalidValue;
  if (C < SP_BK || (C % SP_BK) || (ldx & 3) || ldx < C || (!colstats) != (!stat_rows)) return (int)hipErrorInvalidValue;
  if ((long)B * H * W * ldx >= (1L << 31)) return (int)hipErrorInvalidValue;       // 32-bit element offsets in the gather
  // (the gathered fetch carries its tap as running state from k = 0 on: gemm_impl refuses a K split for it; taps beyond a
  // 16 x 16 window, an output row stride below Cout or a K of 2^31 are not convolutions this entry point serves)
  if (KH > 16 || KW > 16 || Cout < 4 || (Cout & 3) || ldy < Cout || (ldy & 3) || (long)KH * KW * C >= (1L << 31))
    return (int)hipErrorInvalidValue;
  ConvGeom cg;
  cg.H = H; cg.W = W; cg.C = C; cg.KW = KW; cg.stride = stride;
  if (same) {
    cg.OH = (H + stride - 1) / stride; cg.OW = (W + stride - 1) / stride;
    int th = (cg.OH - 1) * stride + KH - H, tw = (cg.OW - 1) * stride + KW - W;
    cg.pt = (th < 0 ? 0 : th) / 2; cg.pl = (tw < 0 ? 0 : tw) / 2;
  } else {
    cg.OH = spnet_valid_out(H, KH, stride); cg.OW = spnet_valid_out(W, KW, stride);
    cg.pt = cg.pl = 0;
  }
  if (cg.OH < 1 || cg.OW < 1) return (int)hipErrorInvalidValue;
  GemmProblem p = gemm_problem(x, SP_K_MAJOR, (int)ldx, Wk, SP_OUT_MAJOR, Cout, y, ldy, B * cg.OH * cg.OW, Cout, KH * KW * C, tile);
  p.bias = bias; p.colstats = colstats; p.stat_rows = stat_rows; p.cg = &cg;
  return gemm_impl(p, stream);
}

// ------------------------------------------------------------------------------------------------
// Stride-2 row gather / scatter of the 1x1 residual convs (TF SAME on a 1x1/s2 conv samples the even pixels).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_s2_kernel(const float* __restrict__ x,
                                                        float* __restrict__ xs, int Bn, int H, int W,
                                                        int C, int OH, int OW) {
  const int c4n = C / 4;
  const long total = (long)Bn * OH * OW * c4n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    long t = i / c4n;
    const int ow = (int)(t % OW);
    t /= OW;
    const int oh = (int)(t % OH);
    const int b = (int)(t / OH);
    *reinterpret_cast<float4*>(xs + i * 4) = *reinterpret_cast<const float4*>(
        x + (((long)b * H + 2 * oh) * W + 2 * ow) * C + c4 * 4);
  }
}

// dx[b, 2oh, 2ow, :] += dxs[b, oh, ow, :]   (each destination touched by exactly one thread)
__global__ __launch_bounds__(256) void scatter_add_s2_kernel(const float* __restrict__ dxs,
                                                             float* __restrict__ dx, int Bn, int H,
                                                             int W, int C, int OH, int OW) {
  const int c4n = C / 4;
  const long total = (long)Bn * OH * OW * c4n;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c4 = (int)(i % c4n);
    long t = i / c4n;
    const int ow = (int)(t % OW);
    t /= OW;
    const int oh = (int)(t % OH);
    const int b = (int)(t / OH);
    float4* d = reinterpret_cast<float4*>(dx + (((long)b * H + 2 * oh) * W + 2 * ow) * C + c4 * 4);
    const float4 g = *reinterpret_cast<const float4*>(dxs + i * 4);
    float4 v = *d;
    v.x += g.x; v.y += g.y; v.z += g.z; v.w += g.w;
    *d = v;
  }
}

// Transposes of many small matrices in one launch: job j writes dst_j[c][r] = src_j[r][c] for an R_j x C_j
// row-major matrix.  jobs (device memory) = njobs x {src pointer, dst pointer, R, C} as four 64-bit words.
// 32x32 tiles through a padded LDS tile: both the global read and the global write are 128-byte row segments.
__global__ __launch_bounds__(256) void transpose_batched_kernel(const long long* __restrict__ jobs) {
  __shared__ float t[32][33];
  const long long* jb = jobs + 4 * blockIdx.z;
  const float* __restrict__ src = reinterpret_cast<const float*>(jb[0]);
  float* __restrict__ dst = reinterpret_cast<float*>(jb[1]);
  const int R = (int)jb[2], C = (int)jb[3];
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  if (r0 >= R || c0 >= C) return;                    // whole workgroup leaves together
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = r0 + ty + 8 * i, c = c0 + tx;
    t[ty + 8 * i][tx] = (r < R && c < C) ? src[(long)r * C + c] : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = c0 + ty + 8 * i, r = r0 + tx;
    if (c < C && r < R) dst[(long)c * R + r] = t[tx][ty + 8 * i];
  }
}

extern "C" int spnet_transpose_batched(const void* jobs, int njobs, int max_rows, int max_cols, void* stream) {
  if (!jobs || njobs < 1 || max_rows < 1 || max_cols < 1) return (int)hipErrorInvalidValue;
  if (njobs > 65535 || max_rows > 65535 * 32) return (int)hipErrorInvalidValue;   // the grid's z and y extents
  hipLaunchKernelGGL(transpose_batched_kernel, dim3((max_cols + 31) / 32, (max_rows + 31) / 32, njobs), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const long long*>(jobs));
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_gather_s2(const float* x, float* xs, int B, int H, int W, int C, void* stream) {
  if (!x || !xs || B < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return (int)hipErrorInvalidValue;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const long total = (long)B * OH * OW * (C / 4);
  hipLaunchKernelGGL(gather_s2_kernel, dim3(spnet_ew_grid(total, 256)), dim3(256), 0,
                     (hipStream_t)stream, x, xs, B, H, W, C, OH, OW);
  SPNET_RETURN_LAUNCH_STATUS();
}

extern "C" int spnet_scatter_add_s2(const float* dxs, float* dx, int B, int H, int W, int C,
                                    void* stream) {
  if (!dxs || !dx || B < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return (int)hipErrorInvalidValue;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const long total = (long)B * OH * OW * (C / 4);
  hipLaunchKernelGGL(scatter_add_s2_kernel, dim3(spnet_ew_grid(total, 256)), dim3(256), 0,
                     (hipStream_t)stream, dxs, dx, B, H, W, C, OH, OW);
  SPNET_RETURN_LAUNCH_STATUS();
}
