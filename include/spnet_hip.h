/* C ABI of libspnet_hip.so -- the MI355X (gfx950) kernels of the SPNet detection hot path.
 *
 * The reference (drscotthawley/SPNet) has no native code and no FFI: its hot path runs inside
 * Keras 2.1.3 / TensorFlow 1.14 / numpy.  Each entry point below names the reference call site whose
 * arithmetic it replaces (paths relative to the reference root).  A maintainer binds these with ctypes
 * (see INTEGRATION.md and spnet_amd/_lib.py).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 data unless noted; tensors are NHWC, row-major
 *   - pointers passed to vectorised kernels must be 16-byte aligned, channel counts multiples of 4
 *     unless the entry says otherwise
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work, they never
 *     synchronise, allocate or free, so a sequence of calls can be captured in a hipGraph
 *   - return value: 0 on success, otherwise a hipError_t (hipErrorInvalidValue for shape/alignment
 *     violations)
 */
#ifndef SPNET_HIP_H
#define SPNET_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense contractions (MFMA fp32) ---------------------------------------------------------- */
/* C[M,N] = sum_k A(m,k) B(k,n) (+ bias[n]).  Replaces the pointwise half of SeparableConv2D, the
 * 1x1/stride-2 residual Conv2D and Dense('FinalOutput')
 * (spnet/models.py:357-359, 388), forward, data-gradient and weight-gradient forms.
 * a_major / b_major: 0 = reduction index contiguous (A[m*lda+k], B[n*ldb+k]),
 *                    1 = output index contiguous    (A[k*lda+m], B[k*ldb+n]).
 * Supported pairs: (0,1) forward, (0,0) dgrad, (1,1) wgrad.
 * lda / ldb / ldc: row strides in floats, multiples of 4; an operand may be a column block of a wider tensor, and nothing
 * outside the block is read or written.  A stride below the extent it strides over is refused by every entry point of this
 * family (hipErrorInvalidValue, nothing launched): ld < K for a K-contiguous operand, lda < M / ldb < N for an
 * output-contiguous one, ldc < N -- rows would overlap, and workgroups would race on the stores of an overlapping C.
 * split_k: 0 = choose automatically, >1 = that many K slices summed deterministically through
 * `workspace` (>= split_k*M*N floats).  tile (BM x BN): 0 auto (cost model over ids 1-8), 1 128x128, 2 128x64, 3 64x64,
 * 4 32x128, 5 96x96, 6 96x64, 7 64x128, 8 128x96, 9 32x64, 10 32x32 (9 and 10: few-row problems, chosen only through
 * spnet_amd/gemm_tiles.json, where tools/autotune_gemm.py measured them faster inside the step); any other id = 0.  The table
 * itself: GEMM_TILES in csrc/gemm_plan.h. */
int spnet_gemm_f32(const float* A, int a_major, int lda, const float* B, int b_major, int ldb, float* C,
                   int ldc, int M, int N, int K, int split_k, float* workspace, long ws_floats,
                   const float* bias, int tile, void* stream);
/* What spnet_gemm_f32 and its siblings (_accumulate, _batched(_splitk), _bnblend / _bnrelu = xf 1 / 2, _colstats,
 * spnet_conv_gemm_f32) would run for a problem of this shape with dense, aligned operands: no launch, no device.  The have_* /
 * accumulate / conv flags say which optional operands the call carries.  plan (HOST int[10]) = {form (0 K/OUT, 1 K/K,
 * 2 OUT/OUT), tile id, BM, BN, K slices, floats of K per slice, slices per problem in the kernel (batched; else 1), pipelined
 * main loop, slabs go to the workspace, colstats rows}; the tile ids are the rows of GEMM_TILES in csrc/gemm_plan.h.
 * Returns non-zero, and leaves plan untouched, where the launch would be refused. */
int spnet_gemm_plan(int a_major, int b_major, int M, int N, int K, int split_k, int have_workspace, long ws_floats,
                    int have_colstats, int have_batch, int nbatch, int xf, int accumulate, int conv, int tile, int* plan);
/* ---- fp32 GEMM on the bf16 matrix cores by operand splitting (csrc/gemm_bf16x3.hip): the forward, data-gradient and
 * weight-gradient GEMMs of the pointwise convolutions (keras SeparableConv2D pointwise step / 1x1 Conv2D;
 * spnet/models.py:346-359).  Every fp32 operand is the exact sum of three bf16 pieces; six bf16 MFMAs with fp32 accumulation
 * per product block; error against float64 no larger than spnet_gemm_f32's, not the same bits.
 * "planes" of a matrix X[R][K]: 3 * spnet_bf16x3_plane_elems(R, K) bf16 (high, middle, low piece) in 1-KiB pieces of 16 rows
 * x 32 columns (layout: csrc/x3t.h), 16-byte aligned, allocated ZEROED (pad rows / columns are never written), at most 2 GiB.
 *   spnet_split_bf16x3           planes of a Keras pointwise kernel W[K][N] in the forward form (rows = output channels)
 *   spnet_split_rows_bf16x3      planes of an fp32 matrix A[R][K] (row stride lda)
 *   spnet_split_bf16x3_batched   all splits of a step in one launch, job = {src, planes, K, N, sn, sk} as six 64-bit words in
 *                                device memory, element (row n, column k) = src[n*sn + k*sk] (forward form of W[cin][cout]:
 *                                K = cin, N = cout, sn 1, sk cout; data gradient dX = dY W^T: K = cout, N = cin, sn cout,
 *                                sk 1); max_elems = the largest plane_elems(N, K) of the batch
 *   spnet_gemm_bf16x3_fwd        C[M][N] = A B^T, A [M][K] fp32 split inside the kernel (lda % 4 == 0, K % 4 == 0, 16-byte
 *                                aligned, lda >= K, ldc >= N), B = planes of [N][K]
 *   spnet_gemm_bf16x3_pp         the same with A given as planes of [M][K] (written by the producing kernel:
 *                                spnet_dwconv3x3_*_x3, spnet_bn_bwd_*_x3): no split, no stage registers, LDS-DMA only
 *   _colstats / colstats != NULL BatchNorm column sums of C as [*stat_rows][2][N] partial rows, *stat_rows = ceil(M/96)
 *                                (stat_rows: HOST int)
 *   spnet_gemm_bf16x3_wgrad_batched  nbatch weight gradients dW[cin][cout] = z^T dy of ONE shape in one launch, from the
 *                                planes of z [M][cin] and dy [M][cout]; jobs = DEVICE array of {z planes, dy planes, dst}
 *                                (three 64-bit words each); ksplit == 1: dst = dW; ksplit > 1: dst = ksplit slabs of
 *                                cin*cout floats in slice order (add them with spnet_reduce_slabs); deterministic.
 *                                spnet_gemm_bf16x3_wgrad_ksplit: the slice count this library would choose. */
long spnet_bf16x3_kp(int K);
long spnet_bf16x3_plane_elems(long R, int K);
int spnet_split_bf16x3(const float* W, void* planes, int K, int N, void* stream);
int spnet_split_rows_bf16x3(const float* A, long lda, void* planes, long R, int K, void* stream);
int spnet_split_bf16x3_batched(const void* jobs, int njobs, long max_elems, void* stream);
int spnet_gemm_bf16x3_fwd(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K, void* stream);
int spnet_gemm_bf16x3_fwd_colstats(const float* A, int lda, const void* planes, float* C, int ldc, int M, int N, int K,
                                   float* colstats, int* stat_rows, void* stream);
int spnet_gemm_bf16x3_pp(const void* a_planes, const void* b_planes, float* C, int ldc, int M, int N, int K, float* colstats,
                         int* stat_rows, void* stream);
long spnet_gemm_bf16x3_wgrad_ksplit(int cin, int cout, int M, int nbatch);
/* The data-gradient GEMM of a SeparableConv2D's pointwise step with the backward of its DEPTHWISE step fused into the
 * epilogue (keras SeparableConv2D inside Xception's middle / exit flow; spnet/models.py:357-359): dz = dy W^T stays in LDS.
 * dy_planes = planes of dL/d(pointwise output) [B*H*W][cout], w_planes = planes of W as stored ([cin][cout]); the plane must
 * satisfy spnet_gemm_bf16x3_dwbwd_ok(H, W, cin) (192 % (H*W) == 0, W <= 16: a 192-pixel tile holds whole images).  Every
 * other argument and every output is spnet_dwconv3x3_tiled_bwd's (x_fwd = the depthwise input, w = its [3][3][cin] kernel,
 * dx bit-identical to the two-launch path; the dw / BatchNorm partial sums in spnet_gemm_bf16x3_dwbwd_rows(B*H*W) rows).
 * spnet_gemm_bf16x3_dwbwd_ok returns 1 | 0 (a predicate, not a launch status). */
/* Inference counterpart: the FORWARD pointwise GEMM (z_planes [B*H*W][cin] x w_planes in the forward form) with, in its
 * epilogue, the folded BatchNormalization (scale_shift[2*cout] or NULL) + ReLU (relu_next) of its output and the depthwise
 * 3x3 of the NEXT SeparableConv2D (w_next [3][3][cout]); out_planes = planes of [B*H*W][cout], bit-identical to
 * spnet_gemm_bf16x3_pp followed by spnet_dwconv3x3_stream_fwd_x3 -- the pointwise output never reaches HBM (keras Xception
 * middle flow, sepconv -> BN -> relu -> sepconv chains; spnet/models.py:357-359; predict_spnet.py:84-87). */
int spnet_gemm_bf16x3_pp_dwfwd(const void* z_planes, const void* w_planes, int B, int H, int W, int cin, int cout,
                               const float* scale_shift, int relu_next, const float* w_next, void* out_planes, void* stream);
long spnet_gemm_bf16x3_dwbwd_rows(long M);
long spnet_gemm_bf16x3_dwbwd_ok(int H, int W, int cin);
int spnet_gemm_bf16x3_pp_dwbwd(const void* dy_planes, const void* w_planes, int B, int H, int W, int cin, int cout,
                               const float* x_fwd, const float* w, float* dx, int relu_in, const float* add, float* partial,
                               const float* in_scale, const float* in_shift, const float* bn_mean, const float* bn_invstd,
                               float* bn_partial, const float* bn_x, void* stream);
int spnet_gemm_bf16x3_wgrad_batched(const void* jobs, int nbatch, int cin, int cout, int M, int ksplit, void* stream);
/* C += A B, formed in the epilogue (no K split): a data gradient added onto what another consumer of the same tensor
 * has already left in C (the branch convolutions of an inception block; call site spnet/models.py:357-359).  tile: 0 or an
 * id of spnet_gemm_f32's list; any other id is refused (hipErrorInvalidValue, C untouched), not read as 0. */
int spnet_gemm_f32_accumulate(const float* A, int a_major, int lda, const float* B, int b_major, int ldb, float* C,
                              int ldc, int M, int N, int K, int tile, void* stream);

/* ---- fp32 MFMA contractions with fused epilogues / operand forms (product path) ------------------------------------ */
/* spnet_gemm_f32's contraction (no split-K, no bias) that also emits BatchNorm column statistics of C from the
 * accumulators: colstats[rows][2][N] per row-tile (sum, sum of squares), *stat_rows (HOST int) = rows.
 * colstats must hold ceil(M/32)*2*N floats. */
int spnet_gemm_f32_colstats(const float* A, int a_major, int lda, const float* B, int b_major, int ldb,
                            float* C, int ldc, int M, int N, int K, int tile, float* colstats,
                            int* stat_rows, void* stream);
/* nbatch independent problems of ONE shape in one launch, no K split.  A0/B0/C0: operands of problem 0;
 * offsets: DEVICE array {A_b - A0, B_b - B0, C_b - C0} in floats (multiples of 4), b = 0..nbatch-1
 * (the engine's deferred middle-flow weight gradients). */
int spnet_gemm_f32_batched(const float* A0, const float* B0, float* C0, const long long* offsets, int nbatch,
                           int a_major, int lda, int b_major, int ldb, int ldc, int M, int N, int K, int tile,
                           void* stream);
/* ... with every problem's K axis cut into `ksplit` slices: fp32 slabs in `workspace` (nbatch * ksplit * M * N floats),
 * summed per problem in slice order by one more launch (deterministic).  ldc == N.  For many same-shaped weight
 * gradients whose outputs are too small to fill the chip even side by side (the repeated blocks of keras
 * InceptionResNetV2 at batch 16; call site spnet/models.py:357-359).  spnet_gemm_batched_ksplit: the slice count (and
 * tile id) this library would choose for such a batch; 1 = no split. */
long spnet_gemm_batched_ksplit(int M, int N, int K, int nbatch, int* tile_out);
int spnet_gemm_f32_batched_splitk(const float* A0, const float* B0, float* C0, const long long* offsets, int nbatch,
                                  int a_major, int lda, int b_major, int ldb, int ldc, int M, int N, int K, int tile,
                                  int ksplit, float* workspace, long ws_floats, void* stream);

/* dX[M,N] = dY[M,K] B[K,N] where dY = a[k]*g + b[k]*yp + c[k] is the output of a BatchNormalization backward
 * (keras BatchNormalization behind every SeparableConv2D / Conv2D of Xception), blended from the incoming gradient
 * g and the saved pre-normalisation tensor yp while the A tile is staged: dY never makes a pass of its own.
 * coef = [a | b | c], cld floats each (from spnet_bn_bwd_coeffs*; zero beyond channel K-1; cld % 32 == 0,
 * cld >= K rounded up to 32).  B is W^T in the output-major form (spnet_transpose_batched).  dy_out (or NULL)
 * receives dY once, as a dense [M][K] matrix whatever lda (the row stride of g and yp), for the layer's weight-gradient
 * GEMM. */
int spnet_gemm_f32_bnblend(const float* g, const float* yp, const float* coef, int cld, int lda, const float* B,
                           int ldb, float* C, int ldc, int M, int N, int K, int tile, float* dy_out, void* stream);

/* block1_conv2 of keras Xception (3x3 VALID stride 1) as implicit GEMMs that gather their operand tiles from the NHWC tensors (no patch matrix):
 * x [B][H][W][cin], w / dw HWIO [3][3][cin][cout], y / dy [B][H-2][W-2][cout].  (cin, cout) = (32, 64).
 * wgrad splits the pixels over workgroups: workspace >= spnet_conv3x3_wgrad_ws() floats. */
int spnet_conv3x3_fwd(const float* x, const float* w, float* y, int B, int H, int W, int cin, int cout,
                      void* stream);
int spnet_conv3x3_dgrad(const float* dy, const float* w, float* dx, int B, int H, int W, int cin, int cout,
                        void* stream);
long spnet_conv3x3_wgrad_ws(int B, int H, int W, int cin, int cout);
int spnet_conv3x3_wgrad(const float* x, const float* dy, float* dw, int B, int H, int W, int cin, int cout,
                        float* workspace, long ws_floats, void* stream);
/* njobs matrix transposes in one launch: dst_j[c][r] = src_j[r][c]; jobs: DEVICE array of {src, dst, R, C}
 * (four 64-bit words per job).  The engine keeps W^T of the pointwise kernels whose data-gradient product
 * dX = dY W^T (keras SeparableConv2D / Conv2D(1x1), call site spnet/models.py:357-359) runs through
 * spnet_gemm_f32_bnblend, which takes B in the forward (output-major) form; refreshed once per optimizer step.
 * max_rows / max_cols: the largest R / C of the table (they size the grid; tiles beyond a job's own extent write nothing).
 * hipErrorInvalidValue, nothing launched: jobs NULL, njobs < 1 or > 65535, max_rows < 1 or > 65535 * 32, max_cols < 1. */
int spnet_transpose_batched(const void* jobs, int njobs, int max_rows, int max_cols, void* stream);
/* out[M][ldc] = sum over nslab slabs of M*N floats, in slab order (the second stage of every K split). */
int spnet_reduce_slabs(const float* ws, int nslab, int M, int N, float* out, int ldc, void* stream);
/* Even-pixel gather / scatter-add: TF 'same' 1x1 stride-2 residual convs of Xception blocks 2,3,4,13.
 * xs[b][oh][ow][:] = x[b][2oh][2ow][:] and dx[b][2oh][2ow][:] += dxs[b][oh][ow][:] over ceil(H/2) x ceil(W/2) pixels; the
 * other pixels of dx are neither read nor written.  hipErrorInvalidValue, nothing launched: a NULL pointer, B, H or W < 1,
 * C < 4 or C % 4. */
int spnet_gather_s2(const float* x, float* xs, int B, int H, int W, int C, void* stream);
int spnet_scatter_add_s2(const float* dxs, float* dx, int B, int H, int W, int C, void* stream);

/* ---- depthwise 3x3 / SAME (34 stride-1 layers per Xception forward: keras SeparableConv2D depthwise step;
 *      MobileNet's DepthwiseConv2D, stride 1 | 2).  w is [3][3][C]. ---- */
/* out[l] = sum over p < P of in[p][l], in a fixed order.  hipErrorInvalidValue, nothing launched: in or out NULL,
 * P < 1, L < 1. */
int spnet_reduce_rows(const float* in, int P, int L, float* out, void* stream);
/* ... with 32*L floats of scratch: many rows (a Conv2D bias gradient: keras InceptionResNetV2's block convs,
 * spnet/models.py:357-359) are folded in 32 parallel slices first (P > 128).  scratch NULL with scratch_floats == 0: one
 * pass, as spnet_reduce_rows.  Refused like spnet_reduce_rows, and: scratch with scratch_floats < 32 * L, scratch NULL
 * with scratch_floats != 0. */
int spnet_reduce_rows_ws(const float* in, int P, int L, float* out, float* scratch, long scratch_floats, void* stream);
/* njobs independent row reductions in one launch; jobs: DEVICE array of {in, out, P, L} (four 64-bit words
 * per job), max_L = largest L.  (All depthwise weight gradients of a step: spnet_dwconv3x3_tiled_bwd with
 * dw == NULL leaves its partial sums in the workspace.)  A job whose L is below max_L leaves the surplus workgroups
 * idle.  hipErrorInvalidValue, nothing launched: jobs NULL, njobs < 1 or > 65535, max_L < 1. */
int spnet_reduce_rows_batched(const void* jobs, int njobs, int max_L, void* stream);
/* Strided depthwise 3x3 / TF-SAME (keras.applications.mobilenet DepthwiseConv2D, strides 1 or 2; spnet/models.py:346-355).
 * op 0: out = y [B][ceil(H/s)][ceil(W/s)][C] from a = x, b = w;  op 1: out = dx [B][H][W][C] from a = dy, b = w;
 * op 2: out = dw [3][3][C] from a = x, b = dy (workspace: spnet_dwconv3x3_strided_ws floats).  H, W: input extent. */
long spnet_dwconv3x3_strided_ws(int B, int H, int W, int C, int stride);
int spnet_dwconv3x3_strided(int op, const float* a, const float* b, float* out, int B, int H, int W, int C, int stride,
                            float* workspace, void* stream);
/* LDS-tiled forms used by the engine: forward, and the FUSED backward (data + weight gradient in one
 * pass over x and dy).  workspace: spnet_dwconv3x3_tiled_bwd_ws(B,H,W,C) floats.  Every tiled and streaming entry point
 * returns hipErrorInvalidValue, and launches nothing, for C % 4 != 0 or B, H or W < 1. */
int spnet_dwconv3x3_tiled_fwd(const float* x, const float* w, float* y, int B, int H, int W, int C,
                              int relu_in, const float* in_scale, const float* in_shift, void* stream);
/* The same with the PRODUCER BatchNorm's training-forward finalize folded into the prologue (one dependent launch less
 * per SeparableConv2D -> BatchNormalization -> SeparableConv2D chain inside keras Xception; spnet/models.py:357-359):
 * partial [rows][2][C] = column sums of x left by spnet_gemm_f32_colstats (rows <= 128), M = pixels they were taken
 * over; the kernel applies relu?(x*scale + shift) with the coefficients it derives (bit-identical to
 * spnet_bn_finalize_fwd), writes save_mean / save_invstd / scale_shift[2C] and updates the moving statistics. */
int spnet_dwconv3x3_tiled_fwd_bnfin(const float* x, const float* w, float* y, int B, int H, int W, int C, int relu_in,
                                    const float* partial, int rows, long M, const float* gamma, const float* beta,
                                    float* moving_mean, float* moving_var, float* save_mean, float* save_invstd,
                                    float* scale_shift, float eps, float momentum, void* stream);
/* The three forward forms with the output written as the bf16x3 planes of the [B*H*W][C] matrix (see the bf16x3 GEMM
 * block above; y_planes: zeroed allocation of 3 * spnet_bf16x3_plane_elems(B*H*W, C) bf16): the depthwise step of a
 * SeparableConv2D hands its result to the pointwise GEMMs (spnet_gemm_bf16x3_pp forward, spnet_gemm_bf16x3_wgrad_batched)
 * in the form they read, 6 bytes per element, no fp32 copy.  Same arithmetic as the fp32 forms. */
int spnet_dwconv3x3_tiled_fwd_x3(const float* x, const float* w, void* y_planes, int B, int H, int W, int C,
                                 int relu_in, const float* in_scale, const float* in_shift, void* stream);
int spnet_dwconv3x3_tiled_fwd_bnfin_x3(const float* x, const float* w, void* y_planes, int B, int H, int W, int C, int relu_in,
                                       const float* partial, int rows, long M, const float* gamma, const float* beta,
                                       float* moving_mean, float* moving_var, float* save_mean, float* save_invstd,
                                       float* scale_shift, float eps, float momentum, void* stream);
int spnet_dwconv3x3_stream_fwd_x3(const float* x, const float* w, void* y_planes, int B, int H, int W, int C, int relu_in,
                                  const float* in_scale, const float* in_shift, int rows_per_seg, void* stream);
long spnet_dwconv3x3_tiled_bwd_ws(int B, int H, int W, int C);
long spnet_dwconv3x3_tiled_rows(int B, int H, int W, int C);
/* in_scale/in_shift (or NULL): the producer BatchNorm's affine applied on load (x_fwd is then the PRE-BN
 * tensor); bn_partial (or NULL): also emit that BatchNorm's backward sums [rows][2][C]; bn_x (or NULL =
 * x_fwd): the pre-BN tensor those sums refer to when x_fwd is not it (a block output BN(yp)+residual).
 * dw == NULL: the [rows][9][C] weight-gradient partial sums stay in `workspace` for a later reduction. */
int spnet_dwconv3x3_tiled_bwd(const float* dy, const float* x_fwd, const float* w, float* dx, float* dw,
                              int B, int H, int W, int C, int relu_in, const float* add, float* workspace,
                              const float* in_scale, const float* in_shift, const float* bn_mean,
                              const float* bn_invstd, float* bn_partial, const float* bn_x, void* stream);
/* The same two operations as STREAMING kernels for planes large enough to be pure bandwidth (entry flow at batch 32,
 * every plane of the batch-128 inference plan; call site spnet/models.py:357-359): a wave owns 8 columns x 32 channels
 * and marches down its rows with its loads 3-4 rows ahead in registers; no LDS tile, no barrier, no row halo.
 * rows_per_seg: rows per wave (<= 0: the library's choice); the backward's partial buffers have
 * spnet_dwconv3x3_stream_rows() rows.  H*W*C*4 < 2^31 per image (32-bit buffer offsets).  y and dx are bit-identical
 * to the tiled kernels' (same fmaf order).  spnet_dwconv3x3_prefers_stream: 1 where the streaming form is the faster
 * one for this plane (the engine asks once per layer). */
long spnet_dwconv3x3_prefers_stream(int B, int H, int W, int C, int backward);
long spnet_dwconv3x3_stream_rows(int B, int H, int W, int C, int rows_per_seg);
long spnet_dwconv3x3_stream_bwd_ws(int B, int H, int W, int C, int rows_per_seg);
int spnet_dwconv3x3_stream_fwd(const float* x, const float* w, float* y, int B, int H, int W, int C, int relu_in,
                               const float* in_scale, const float* in_shift, int rows_per_seg, void* stream);
int spnet_dwconv3x3_stream_bwd(const float* dy, const float* x_fwd, const float* w, float* dx, float* dw, int B, int H,
                               int W, int C, int relu_in, const float* add, float* workspace, const float* in_scale,
                               const float* in_shift, const float* bn_mean, const float* bn_invstd, float* bn_partial,
                               const float* bn_x, int rows_per_seg, void* stream);

/* ---- BatchNormalization(axis=-1, momentum .99, eps 1e-3) (spnet/models.py:326-336 + 40 in Xception) --- */
/* act: 0 none, 1 ReLU, 2 LeakyReLU(0.1), 3 ReLU6 (MobileNet) fused behind the affine; residual (or NULL) added last;
 * res_bcast=1 (C in {1, 2, 3} only; hipErrorInvalidValue at C % 4 == 0): residual holds one value per pixel, broadcast
 * over the channels (the stem's skip connection from the 1-channel input, spnet/models.py:337). */
long spnet_bn_ws(long M, int C);
int spnet_bn_fwd_train(const float* x, long M, int C, const float* gamma, const float* beta,
                       float* moving_mean, float* moving_var, float* save_mean, float* save_invstd,
                       float* scale_shift, int act, const float* residual, int res_bcast, float* y,
                       float eps, float momentum, float* workspace, void* stream);
int spnet_bn_fwd_infer(const float* x, long M, int C, const float* gamma, const float* beta,
                       const float* moving_mean, const float* moving_var, float* scale_shift, int act,
                       const float* residual, int res_bcast, float* y, float eps, void* stream);
int spnet_bn_bwd(const float* x, const float* dy, long M, int C, const float* gamma, const float* beta,
                 const float* save_mean, const float* save_invstd, int act, float* dx, float* dgamma,
                 float* dbeta, float* coeffs, float* workspace, void* stream);
/* Split forms for fused pipelines: statistics arrive as partial[P][2][C] from a GEMM epilogue
 * (spnet_gemm_f32_colstats) or from the fused depthwise backward.  The three finalize entries CONSUME `partial` when
 * P >= 1024: a first stage leaves 64 slice sums (hi, lo float pairs) in the buffer's own first rows, so the partial rows
 * cannot be read again afterwards (a second consumer must take its copy first). */
int spnet_bn_finalize_fwd(float* partial, int P, long M, int C, const float* gamma, const float* beta,
                          float* moving_mean, float* moving_var, float* save_mean, float* save_invstd,
                          float* scale_shift, float eps, float momentum, void* stream);
int spnet_bn_infer_coeffs(int C, const float* gamma, const float* beta, const float* moving_mean,
                          const float* moving_var, float* scale_shift, float eps, void* stream);
int spnet_bn_apply(const float* x, long M, int C, const float* scale_shift, int act, const float* residual,
                   int res_bcast, float* y, void* stream);
/* spnet_bn_finalize_fwd + spnet_bn_apply (no broadcast residual) as ONE launch while P <= 128 partial rows (P <= 512
 * while M*C <= 4 Mi; more rows: the two launches, and `partial` is consumed from P = 1024 as above) -- the closing
 * BatchNormalization + Add of a keras Xception middle block in training (spnet/models.py:357-359); results identical. */
int spnet_bn_finalize_apply(float* partial, int P, const float* x, long M, int C, const float* gamma,
                            const float* beta, float* moving_mean, float* moving_var, float* save_mean,
                            float* save_invstd, float* scale_shift, int act, const float* residual, float* y, float eps,
                            float momentum, void* stream);
/* The `_ld` forms of the three forward entries write y with a row stride of ldy floats (>= C, multiples of 4): the output
 * is a column block of a wider tensor -- a conv2d_bn branch of keras InceptionResNetV2 written straight into the buffer
 * of its Concatenate (call site spnet/models.py:357-359), so that no copy pass follows. */
int spnet_bn_finalize_apply_ld(float* partial, int P, const float* x, long M, int C, const float* gamma,
                               const float* beta, float* moving_mean, float* moving_var, float* save_mean,
                               float* save_invstd, float* scale_shift, int act, const float* residual, float* y, long ldy,
                               float eps, float momentum, void* stream);
int spnet_bn_fwd_train_ld(const float* x, long M, int C, const float* gamma, const float* beta, float* moving_mean,
                          float* moving_var, float* save_mean, float* save_invstd, float* scale_shift, int act,
                          const float* residual, int res_bcast, float* y, long ldy, float eps, float momentum,
                          float* workspace, void* stream);
int spnet_bn_fwd_infer_ld(const float* x, long M, int C, const float* gamma, const float* beta, const float* moving_mean,
                          const float* moving_var, float* scale_shift, int act, const float* residual, int res_bcast,
                          float* y, long ldy, float eps, void* stream);
int spnet_bn_bwd_from_partials(const float* x, const float* dy, long M, int C, const float* gamma,
                               const float* beta, const float* save_mean, const float* save_invstd, int P,
                               const float* partial, float* dx, float* dgamma, float* dbeta, float* coeffs,
                               void* stream);
/* spnet_bn_bwd / spnet_bn_bwd_from_partials with dx written as the bf16x3 planes of the [M][C] matrix (dx_planes: zeroed
 * allocation of 3 * spnet_bf16x3_plane_elems(M, C) bf16; C % 4 == 0): the gradient a BatchNormalization hands to the
 * pointwise convolution in front of it is read by that layer's data-gradient and weight-gradient GEMMs only
 * (spnet_gemm_bf16x3_pp, spnet_gemm_bf16x3_wgrad_batched), in this form.  Same arithmetic as the fp32 forms. */
int spnet_bn_bwd_x3(const float* x, const float* dy, long M, int C, const float* gamma, const float* beta,
                    const float* save_mean, const float* save_invstd, int act, void* dx_planes, float* dgamma,
                    float* dbeta, float* coeffs, float* workspace, void* stream);
int spnet_bn_bwd_from_partials_x3(const float* x, const float* dy, long M, int C, const float* gamma,
                                  const float* beta, const float* save_mean, const float* save_invstd, int P,
                                  const float* partial, void* dx_planes, float* dgamma, float* dbeta, float* coeffs,
                                  void* stream);

/* Reduction half of the backward only (dgamma, dbeta, blend coefficients for spnet_gemm_f32_bnblend). */
int spnet_bn_bwd_coeffs_from_partials(int P, const float* partial, long M, int C, const float* gamma,
                                      const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta,
                                      float* coef, int cld, void* stream);
int spnet_bn_bwd_coeffs(const float* x, const float* dy, long M, int C, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta, float* coef,
                        int cld, float* workspace, void* stream);

/* ---- pooling --------------------------------------------------------------------------------- */
/* MaxPooling2D(3, strides 2, 'same') + residual add (Xception blocks 2,3,4,13); idx4 packs the argmax
 * tap of 4 channels per uint32 (B*OH*OW*C/4 words) for the backward pass. */
/* x_ss / r_ss (or NULL): [scale|shift] of the BatchNorm producing x / residual, applied on load. */
int spnet_maxpool3x3s2_add_fwd(const float* x, const float* residual, float* y, uint32_t* idx4, int B,
                               int H, int W, int C, const float* x_ss, const float* r_ss, void* stream);
int spnet_maxpool3x3s2_bwd(const float* dy, const uint32_t* idx4, float* dx, int B, int H, int W, int C,
                           void* stream);
/* The same, also emitting the backward sums (sum dx, sum dx*xhat) of the BatchNorm whose un-materialised output was
 * pooled -- yp = its pre-normalisation tensor [B,H,W,C], mean / invstd as saved by its forward -- as
 * partial[rows][2][C], rows = spnet_maxpool3x3s2_bwd_rows(B,H,W,C,max_rows) <= max_rows: the gradient path of block{2,3,4,13}_pool +
 * block*_sepconv2_bn in keras.applications.Xception (call site spnet/models.py:357-359) without a reduction pass.
 * `rows` may be any count from 1 to that answer (anything else: hipErrorInvalidValue).  Pixel r = (b*H + h)*W + w
 * belongs to partial row (r / 32) % rows: a row takes 32 consecutive pixels, then strides by rows * 32. */
long spnet_maxpool3x3s2_bwd_rows(int B, int H, int W, int C, int max_rows);
int spnet_maxpool3x3s2_bwd_bnsums(const float* dy, const uint32_t* idx4, float* dx, int B, int H, int W, int C,
                                  const float* yp, const float* mean, const float* invstd, float* partial, int rows,
                                  void* stream);
/* AveragePooling2D(2) of the stem (spnet/models.py:323,337); any C. */
int spnet_avgpool2_fwd(const float* x, float* y, int B, int H, int W, int C, void* stream);
int spnet_avgpool2_bwd(const float* dy, float* dx, int B, int H, int W, int C, void* stream);

/* ---- keras InceptionResNetV2 (cf.basemodel = 'InceptionResNetV2', spnet/models.py:357-359) ------------------------ */
/* MaxPooling2D(3, strides=2, 'valid') (stem, mixed_6a, mixed_7a); idx4 as above. */
int spnet_maxpool3x3s2_valid_fwd(const float* x, float* y, uint32_t* idx4, int B, int H, int W, int C, void* stream);
int spnet_maxpool3x3s2_valid_bwd(const float* dy, const uint32_t* idx4, float* dx, int B, int H, int W, int C, void* stream);
/* AveragePooling2D(3, strides=1, 'same') (mixed_5b; TF averages over the in-image entries); backward = 1: in = dy, out = dx. */
int spnet_avgpool3x3s1_same(const float* in, float* out, int B, int H, int W, int C, int backward, void* stream);
/* Patch matrix of a KH x KW / stride s / 'same' | 'valid' convolution and its adjoint: backward = 0: out = col
 * [B*OH*OW][KH*KW*C] from in = x; backward = 1: out = dx [B][H][W][C] from in = dcol.  The convolution itself is
 * spnet_gemm_f32 on col and the flattened HWIO kernel (1x1 convs skip the patch matrix).  C % 4 == 0, stride 1 | 2;
 * a shape without output (B, H or W < 1; VALID with H < KH or W < KW, at either stride) or a NULL tensor is
 * hipErrorInvalidValue (spnet_patches_ld and spnet_conv_gemm_f32 alike). */
int spnet_patches(const float* in, float* out, int B, int H, int W, int C, int KH, int KW, int stride, int same, int backward,
                  void* stream);
/* The forward gather of an input whose pixels are ldx floats apart (a column block of a wider tensor). */
int spnet_patches_ld(const float* in, long ldx, float* out, int B, int H, int W, int C, int KH, int KW, int stride, int same,
                     void* stream);
/* The forward convolution itself on the tuned GEMM kernel (gemm.hip, AG = 1; no patch matrix written or read): the A tile of K step (tap, 32 channels) is the plain
 * K-major fetch from a shifted base with the out-of-image rows zeroed, in the pipeline slots of the matrix form -- no
 * patch matrix, no gather launch, the tile ids / autotuned table of spnet_gemm_f32.  x pixels ldx floats apart (ldx >= C:
 * a column block of a wider tensor), Wk = the HWIO kernel as [KH*KW*C][Cout], y [B*OH*OW][ldy]; C % 32 == 0, stride
 * 1 | 2, TF SAME (same != 0) or VALID; bias / colstats + stat_rows optional (as spnet_gemm_f32_colstats).  Bit-identical
 * to spnet_patches(_ld) + spnet_gemm_f32(_colstats) on the same tile (keras Conv2D k_h x k_w of Inception-ResNet-v2,
 * spnet/models.py:357-359). */
int spnet_conv_gemm_f32(const float* x, long ldx, const float* Wk, float* y, int ldy, int B, int H, int W, int C, int Cout,
                        int KH, int KW, int stride, int same, const float* bias, int tile, float* colstats,
                        int* stat_rows, void* stream);
/* Gradient producers that also leave the BatchNorm-backward sums (sum g, sum g*xhat) of the conv2d_bn layer whose output
 * y = relu(BN(yp)) they differentiate, g masked with y > 0 when relu != 0: partial[rows][2][C], rows <=
 * spnet_grad_bnsums_rows(pixels, max_rows).  spnet_patches_bwd_bnsums = spnet_patches(backward = 1) + mask + sums (the
 * consumer is a k x k convolution); spnet_copy_cols_bnsums = one branch of a Concatenate backward (strided column block
 * -> dense) + mask + sums.  The layer's BatchNorm backward then runs spnet_bn_bwd_from_partials with no activation
 * (keras InceptionResNetV2 conv2d_bn chains; call site spnet/models.py:357-359).
 * `rows` may be any count from 1 to spnet_grad_bnsums_rows(pixels, rows) (anything else: hipErrorInvalidValue).  Pixel
 * r = (b*H + h)*W + w (row r of the column block) belongs to partial row (r / 32) % rows: a row takes 32 consecutive
 * pixels, then strides by rows * 32; partial[p][0][c] = sum g, partial[p][1][c] = sum g * xhat over those pixels.
 * A shape without output (B, H or W < 1; a VALID window longer than the image, at either stride), a NULL tensor, a row
 * stride below C, or M >= 2^31 is hipErrorInvalidValue, and nothing is launched. */
long spnet_grad_bnsums_rows(long npix, int max_rows);
int spnet_patches_bwd_bnsums(const float* dcol, float* dx, int B, int H, int W, int C, int KH, int KW, int stride, int same,
                             const float* y, const float* yp, const float* mean, const float* invstd, int relu,
                             float* partial, int rows, void* stream);
int spnet_copy_cols_bnsums(const float* src, int lds, float* dst, long M, int C, const float* y, long ldy, const float* yp,
                           const float* mean, const float* invstd, int relu, float* partial, int rows, void* stream);
/* `_ld` forms: row strides for dx (lddx / ldd), yp (ldyp) and the partial rows (ldp floats per half-row) -- the layer may be one
 * member of a group of sibling 1x1 convolutions that share a concatenated pre-normalisation tensor, gradient buffer and
 * partial rows (column blocks of [.][Ct] tensors; IRv2Backbone runs such a group as one GEMM + one BatchNormalization). */
int spnet_patches_bwd_bnsums_ld(const float* dcol, float* dx, long lddx, int B, int H, int W, int C, int KH, int KW, int stride,
                                int same, const float* y, long ldy, const float* yp, long ldyp, const float* mean,
                                const float* invstd, int relu, float* partial, long ldp, int rows, void* stream);
int spnet_copy_cols_bnsums_ld(const float* src, int lds, float* dst, long ldd, long M, int C, const float* y, long ldy,
                              const float* yp, long ldyp, const float* mean, const float* invstd, int relu, float* partial,
                              long ldp, int rows, void* stream);
/* Many strided column-block copies in one launch: jobs (device memory) = njobs x {src, dst, rows, cols, lds, ldd} as six
 * 64-bit words; max_elems = the largest rows*cols (sizes the grid).  The kernels of sibling convolutions gathered into
 * their concatenated GEMM operand after every optimizer step. */
int spnet_copy_cols_batched(const void* jobs, int njobs, long max_elems, void* stream);
/* inception_resnet_block: y = x + scale*up (+ ReLU); backward: dx = g*(y>0 if relu), dup = scale*dx. */
int spnet_resadd(const float* x, const float* up, float* y, long n, float scale, int relu, void* stream);
int spnet_resadd_bwd(const float* y, const float* g, float* dx, float* dup, long n, float scale, int relu, void* stream);
/* dst[r*ldd + c] (+)= src[r*lds + c] for c < cols: Concatenate's channel blocks and gradient accumulation.  cols, lds, ldd
 * multiples of 4; lds >= cols and ldd >= cols (overlapping rows are refused). */
int spnet_copy_cols(const float* src, int lds, float* dst, int ldd, long rows, int cols, int accumulate, void* stream);

/* ---- small-channel direct 3x3 convs: stem conv2d_1..3 (models.py:321,330,335), block1_conv1 ---- */
/* op 0 fwd (a=x,b=w,out=y) | 1 bwd-data (a=dy,b=w,out=dx) | 2 bwd-weight (a=x,b=dy,out=dw).
 * (cin,cout,stride,same) in {(1,3,1,1), (3,3,1,1), (3,32,2,0)}; w is HWIO. */
int spnet_conv3x3_small(int op, int cin, int cout, int stride, int same, const float* a, const float* b,
                        float* out, int B, int H, int W, float* workspace, long ws_floats, void* stream);

/* The stem's first three layers fused (spnet/models.py:321-323, 337): conv2d_1 (1 -> 3, 3x3 'same', no bias) +
 * AveragePooling2D(2), and the skip connection's AveragePooling2D(2) of the input frame.
 * op 0: a = w [3][3][1][3]; out = p1 [B][H/2][W/2][3], out2 = px [B][H/2][W/2].
 * op 2: a = dp1 (gradient of p1); out = dw [3][3][1][3]; workspace >= 512*27 floats.  (No data gradient: x is the input.) */
int spnet_stem_head(int op, const float* x, const float* a, float* out, float* out2, int B, int H, int W,
                    float* workspace, long ws_floats, void* stream);

/* ---- loss / decode ---------------------------------------------------------------------------- */
/* custom_loss + my_loss terms + d/dy_pred (spnet/models.py:557-633).  loss_out[6] =
 * (center,size,angle,noobj,class,total); parts = B*5 floats scratch; grad may be NULL. */
int spnet_ellipse_loss(const float* y_true, const float* y_pred, float* grad, float* parts,
                       float* loss_out, int B, int ncols, int hybrid, void* stream);
/* SelectiveSigmoid (spnet/models.py:277-298) / the sigmoid columns of the 'compound' head (models.py:379-386,
 * after InterleaveColumns the sigmoid outputs sit at columns start::step).  backward == 0: y[:, start::step] =
 * sigmoid(.) in place; backward == 1: grad[:, start::step] *= y (1 - y), y being the post-sigmoid output. */
int spnet_selective_sigmoid(float* y, float* grad, int B, int ncols, int start, int step, int backward, void* stream);
/* denorm_Y + cleanup_antinode_vars angle (spnet/utils.py:186-188,56-64; evaluate_spnet.py:70-73):
 * out[B][ncols/8][7] = (cx,cy,a,b,angle_deg,noobj,rings). */
int spnet_decode(const float* y_norm, const float* means, const float* ranges, float* out, int B,
                 int ncols, int sigmoid_noobj, void* stream);

/* ---- evaluation metric (spnet/diagnostics.py:64-161: compute_iou / calc_map) ----------------------------- */
/* Raster IoU of npairs (predicted, true) ellipse rows [npairs][8] (denormalised cx,cy,a,b,cos2t,sin2t,noobj,
 * rings) on an nx x ny canvas; iou[i] = -1 where the true slot is empty (noobj > 0.99) or both rasters are; a predictor
 * with noobj >= 0.5, a <= 0 or b <= 0 has an empty raster.  hipErrorInvalidValue, nothing launched: a NULL pointer,
 * npairs < 1 or >= 2^31, nx or ny < 1 or > 32768 (a union box of nx * ny <= 2^30 pixels is counted in int). */
int spnet_ellipse_iou(const float* yp, const float* yt, long npairs, int nx, int ny, double* iou, void* stream);

/* Count metrics (spnet/diagnostics.py:13-59: calc_errors) over [N][ncols] de-normalised grids: counts[7] (int, zeroed
 * by the caller) = ring_miscounts, ring_truecounts, total_obj, false_obj_pos, false_obj_neg, true_obj_pos,
 * true_obj_neg; pix_err[N] = centre error of each row's first predictor.  The counts are ADDED to counts[].  noobj is
 * rounded half to even; a ring count differs when |difference| > 0.5.  hipErrorInvalidValue, nothing launched: a NULL
 * pointer, N < 1, ncols < 8 or ncols % 8. */
int spnet_calc_errors(const float* yp, const float* yt, long N, int ncols, int* counts, float* pix_err, void* stream);

/* ---- optimizer ---------------------------------------------------------------------------------- */
/* Keras Adam + l2 on the first l2_n elements (spnet/models.py:494, 47-71).  sq_scratch >= 2048 floats.
 * mask (or NULL): n floats, 0 = frozen element (layer.trainable=False, spnet/models.py:361-373).
 * lr_t_dev (or NULL): device float overriding lr_t, so a captured hipGraph of the step can be replayed.
 * sq_scratch and l2_loss_out may be NULL (no penalty is reported); n == 0 updates nothing and reports a penalty of 0.
 * hipErrorInvalidValue, nothing launched: p, g, m or v NULL, n < 0, n % 4. */
int spnet_adam_step(float* p, const float* g, float* m, float* v, long n, long l2_n, float lr_t,
                    float beta1, float beta2, float eps, float l2, float grad_scale, const float* mask,
                    float* sq_scratch, float* l2_loss_out, const float* lr_t_dev, void* stream);
/* The same step over a RANGE of the flat buffers (pointers to the range's first element, n % 4 == 0, l2_n = how many of
 * its leading elements are l2-regularised): the Dense head's range is updated as soon as its gradient is final, underneath
 * the backbone's backward; the rest when backward has ended.  Leaves spnet_adam_parts(n) sum-of-squares partials in
 * sq_partial; spnet_adam_l2_sum folds the partials of every range of a step into l2_loss_out[0] = l2 * sum(w^2).
 * spnet_adam_parts(n) = min(2048, ceil(n / 1024)), 0 for n < 4; workgroup b of a range sums the float4 items
 * b * 256 + t + k * 256 * parts (t < 256, k = 0, 1, ..) into sq_partial[b].  spnet_adam_part refuses (hipErrorInvalidValue,
 * nothing launched) p, g, m or v NULL, n < 4 and n % 4: the caller skips an empty range.  spnet_adam_l2_sum refuses a
 * NULL pointer, count < 1 and count > 32768 (the partials of 16 full ranges). */
long spnet_adam_parts(long n);
int spnet_adam_part(float* p, const float* g, float* m, float* v, long n, long l2_n, float lr_t, float beta1, float beta2,
                    float eps, float l2, float grad_scale, const float* mask, float* sq_partial, const float* lr_t_dev,
                    void* stream);
int spnet_adam_l2_sum(const float* sq_partial, int count, float l2, float* l2_loss_out, void* stream);

/* ---- input codec on the device (spnet/utils.py:340-342, load_X_one_proc) ------------------------------------------ */
/* uint8 grey levels -> float32 network input, dst = (src / 255 - 0.5) * 2 with numpy's float32 roundings (bit-identical
 * to the host conversion); n pixels, pointers 16-byte aligned.  Lets frames cross PCIe as bytes. */
int spnet_u8_to_input(const unsigned char* src, float* dst, long n, void* stream);
/* PIL.Image.resize((OW, OH), ANTIALIAS) of N one-channel uint8 frames [N][H][W] (spnet/utils.py:335-337), bit-identical to
 * Pillow's 8-bit Lanczos resampler: horizontal pass, then vertical over its uint8 result, both in one launch (the
 * intermediate lives in LDS).  xtab / ytab: int32 device tables [O][2 + taps] = (first input index, tap count, taps ...,
 * zero padded) of spnet_amd/resize.py lanczos_taps(), |tap| < 2^23; a pass whose size does not change is skipped as Pillow
 * skips it (its table is ignored and may be NULL).  out_u8 (or NULL): [N][OH][OW]; out_f (or NULL): the same frames as
 * network input, == spnet_u8_to_input(out_u8); at least one.  Sizes 1 .. 2048, any W / OW, no alignment asked
 * of src / out_u8 (a slice of frames is fine; out_f as a float).  hipErrorInvalidValue (nothing written) otherwise.
 * Tables that are not lanczos_taps' of the size pair give wrong or unwritten pixels, never an out-of-range access. */
int spnet_resize_u8(const unsigned char* src, int N, int H, int W, const int* xtab, int xtaps, const int* ytab, int ytaps,
                    int OH, int OW, unsigned char* out_u8, float* out_f, void* stream);
/* Batch assembly: dst[i][0..L) = src[index[i]][0..L), n rows of L floats (16 bytes per lane when L % 4 == 0 and both
 * buffers are 16-byte aligned, 4 otherwise), index int32 | int64 on the device (idx_bytes 4 | 8), clamped to [0, src_rows) -- the minibatch gather Keras' fit does on the host
 * (train_spnet.py:75,81: model.fit(X_train, Y_train, batch_size, shuffle=True)). */
int spnet_gather_rows(const float* src, long src_rows, const void* index, int idx_bytes, float* dst, int n, long L,
                      void* stream);

/* ---- augmentation (spnet/callbacks.py:272-341, spnet/augmentation.py) ---------------------------- */
/* per-frame min/max -> mm[N][2]; scratch: N*32 floats */
int spnet_minmax(const float* x, int N, long hw, float* mm, float* scratch, void* stream);
int spnet_cutout(const float* src, const int* src_index, float* dst, int N, int H, int W,
                 const int* rects, const float* vals, const int* nrect, void* stream);
int spnet_saltpepper(float* x, int N, int H, int W, const int* coords, int n_salt, int n_pepper,
                     const int* flag, const float* mm, void* stream);
/* cv2.GaussianBlur(img, (k,k), 0), k = ksize[n] in {0 = copy, 3, 5, 7} per frame (fixed small-kernel table, reflect-101
 * borders): what blur_inplace (spnet/augmentation.py:66-70) computes and then discards.  dst != src. */
int spnet_gaussian_blur(const float* src, float* dst, int N, int H, int W, const int* ksize, void* stream);
int spnet_warp_affine(const float* src, float* dst, int N, int H, int W, int C, const float* minv,
                      void* stream);
/* cv2.warpAffine as OpenCV computes it for 8-bit images (INTER_LINEAR, zero border; rotate_image / translate_image,
 * spnet/augmentation.py:193-194, 232): 1/32-pixel fixed-point coordinates, 15-bit integer bilinear weights.  src / dst
 * hold 8-bit values as fp32; xrow [N][H][2] = (X0, Y0), xcol [N][W][2] = (adelta, bdelta): the host-rounded row and
 * column terms of the INVERTED matrix, scaled by 1024 (+ round_delta 16 in X0 / Y0). */
int spnet_warp_affine_fixed(const float* src, float* dst, int N, int H, int W, int C, const int* xrow, const int* xcol,
                            void* stream);
/* flip_image -> rotate_image -> translate_image of N one-channel uint8 frames in ONE gather (augment_preproc.py:74-99;
 * spnet/augmentation.py:82-112, 184-207 and 216-239), bit-identical to the three steps run one after the other: the flip is
 * a pixel permutation, the rotation cv2.warpAffine's 8-bit fixed-point bilinear (as spnet_warp_affine_fixed computes it, its
 * row / column terms formed on the device in float64 without contraction), the translation an integer shift with zero fill.
 * src [n_src][H][W]; sel (or NULL: output n reads source n, N <= n_src): int32 source index per output, clamped to
 * [0, n_src); params: N records of 64 bytes, 8-byte aligned = { double m[6] (the INVERTED rotation matrix, row major),
 * int flip (-2 none, 0 vertical, 1 horizontal, -1 both), int xt, int yt, int pad }.  out_u8 (or NULL): [N][H][W]; out_f (or
 * NULL): the same frames as network input, == spnet_u8_to_input(out_u8); at least one.  Sizes 1 .. 2048, any W, no
 * alignment asked of src / out_u8.  hipErrorInvalidValue (nothing written) otherwise.  No parameter value causes an
 * out-of-range access: row / column terms saturate at 2^29 (bit-identity holds below that), shifts past the frame give
 * zeros, other flip codes mean none. */
int spnet_warp_chain_u8(const unsigned char* src, int n_src, const int* sel, const void* params, int N, int H, int W,
                        unsigned char* out_u8, float* out_f, void* stream);
/* Grid targets of B frames from their metadata rows (csrc/targets.hip): parse_meta_file's row processing ->
 * true_to_pred_grid -> norm_Y (spnet/utils.py:260-286, 191-244, 181-184), one wave per frame, bit-identical to
 * spnet_amd/augmentation.py _encode_targets.  rows [B][K][6] = cx, cy, a, b, angle_deg, rings in float64 (pad_metadata's
 * layout), 1 <= K <= 16; count [B] = valid rows per frame, clamped to 0..K.  Per frame: a/b swapped and 90 degrees added
 * where b > a; rows with rings <= 0 dropped; the kept rows ordered by (cx, cy), stably; ix = clip(trunc((cx - 40) / xbin),
 * 0, nx - 1), iy likewise, in float64, xbin = 430 / nx, ybin = 310 / ny (integer divisions); an ellipse takes the next free
 * slot of its cell; every other slot holds setup_means_and_ranges' blank values; the ellipse is cast to float32 and
 * (G - means) / ranges formed in float32 with one correctly rounded subtract and one correctly rounded divide.
 * Y [B][nx*ny*ns*8].  flags [B]: 0 fine; 1 a cell would take more than ns ellipses, Y holds those that fit.
 * trig [360][2] = (cos, sin) of 2 * deg2rad(k) for the whole degrees k = 0..359, computed by the host in float64 and
 * rounded to float: an angle that is integer-valued and in [0, 360) takes its entry (the same bits as the host codec), any
 * other is cos / sin (2.0 * (angle * (pi / 180.0))) in float64, then cast (within one float32 step of the host's libm).
 * fwd with warp_records (both or neither; then H, W = the frame size, >= 1): warp_metadata (spnet_amd/augmentation.py)
 * is applied to the rows first, in float64 with its roundings.  fwd [B][8] = the six entries of the FORWARD
 * rotation_matrix_2d, the rotation angle in degrees, one unused double; warp_records = the 64-byte records
 * spnet_warp_chain_u8 reads, of which flip, xt and yt are used: cy = H - cy and angle = -angle for flip 0 / -1, cx = W - cx
 * and angle = 180 - angle for flip 1 / -1, cleanup_angle's add / subtract 180 loops after each for every flip but -2; for
 * a rotation angle != 0, angle + rot with the same cleanup and the centres as rint((m00 cx + m01 cy) + m02), each product
 * and sum rounded on its own; then cx + xt, cy + yt.  A warped frame that overflows a cell is REJECTED as warp_targets
 * rejects it: its UNWARPED rows are encoded, its warp record is overwritten with the identity (m = 1,0,0,0,1,0, flip -2,
 * xt = yt = 0) and flags[b] = 1; flags[b] = 2 when the unwarped rows overflow as well (Y then holds those that fit).
 * B == 0: nothing to do, success.  hipErrorInvalidValue (nothing launched or written): K outside 1..16; nx, ny or ns < 1;
 * nx > 430 or ny > 310 (a bin of 0 pixels) or more than 2^24 slots; a NULL rows / count / trig / Y / flags; exactly one of
 * fwd and warp_records; with them H or W < 1; rows / fwd / warp_records not 8-byte, the others not 4-byte aligned.  No
 * value in rows causes an out-of-range access: NaN and huge centres clip into an edge cell, and cleanup_angle's loops end
 * after 64 turns (bit-identity holds for angles within +-11,520 degrees). */
int spnet_encode_targets(const double* rows, const int* count, int B, int K, int nx, int ny, int ns, int H, int W,
                         const float* trig, const double* fwd, void* warp_records, float* Y, int* flags, void* stream);
/* The random parameters of the on-the-fly augmentation of B samples, drawn on the device in one launch
 * (csrc/augment_params.hip), into the arrays the kernels above read.  sample [B]: int32 sample indices on the device.
 * Augmentation half (rects != NULL; 12 <= H, W <= 2048): rects [B][6][4] = (r0, r1, c0, c1), vals [B][6], nrect [B] for
 * spnet_cutout (entries past nrect are zeros); coords [B][2][n_salt + n_pepper], flag [B] for spnet_saltpepper (zeros where
 * flag is 0); ksize [B] for spnet_gaussian_blur.  mm [n_frames][2]: spnet_minmax of the pristine frames, row = the sample
 * index clamped into the table.  Warp half (warp_records != NULL; 1 <= Hw, Ww <= 2048, the full frame size): the B 64-byte
 * records of spnet_warp_chain_u8 and fwd [B][8] of spnet_encode_targets; trig [4097][2] float64 = (cos, sin) of
 * deg2rad((k - 2048) * (20 / 2048)) as the host's libm gives them.  Either half alone or both; with both a sample's warp and
 * augmentation share its key.  B == 0: nothing to do, success.  hipErrorInvalidValue (nothing launched): B < 0, a NULL
 * sample, neither half, sizes outside the ranges above, n_salt or n_pepper < 0, n_frames < 1, a NULL array of a selected
 * half, warp_records / fwd / trig not 8-byte aligned.
 * The stream, stateless and counter based -- a sample's values depend on (seed, epoch, sample index) only, not on its
 * position in the batch, the batch size, the rank or the world size; the reference's distributions, other values:
 *   mix, u(key, k) = mix(key ^ (k * 0x85ebca6b + 0xc2b2ae35)) and randint(u, lo, hi) as for spnet_fake_espi_params below
 *   (csrc/counter_rng.h); U(u) = (u >> 8) * 2^-24
 *   skey = mix(mix(mix(seed ^ 0x3c6ef372) + epoch) ^ sample)                       (uint32)
 *   key(slot) = mix(skey + slot): slot 0 = the frame's own draws, 1 + r = cutout rectangle r, 7 = warp, 8 = salt / pepper
 *   slot 0: k 0 cutout count [0, 6]; 1 salt / pepper gate = u >> 31; 2 blur when U < 0.4 and 3 U <= 0.3 (compared in
 *     double), then 4 ksize = 7 if u >> 31 else 3 (0 without blur); the band-pass mix-up's draws, made by the HOST from the
 *     same key (augmentation.draw_bandpass_keyed): 5 gate U < bpmix_prob (in double), 6 table row [0, 4 n_real - 1], 7 scale
 *     = 3 * U in float32
 *   slot 1 + r: k 0 r0 [0, H - 12]; 1 c0 [0, W - 12]; 2 dr, 3 dc [11, 74]; r1 = min(r0 + dr, H - 1), c1 = min(c0 + dc,
 *     W - 1); 4 fill = lo + U * (hi - lo) in float32, each operation rounded on its own
 *   slot 8: point p (salt points first, then pepper): k 2p row [0, H - 2], 2p + 1 column [0, W - 2]
 *   slot 7: k 0 flip = (u >> 30) - 2; 1 angle index [0, 4096]; 2 shift unless randint [0, 9] is 0; 3, 4 xt, yt =
 *     rint(40 * (2 U - 1)) in double, half to even (0 when the gate is off)
 *   matrices: index 2048 gives the identity for both; otherwise (a, b) = trig[k], fwd = rotation_matrix_2d((Ww / 2, Hw / 2),
 *     angle) and the record's m = invert_affine_cv2(fwd) (spnet_amd/augmentation.py), in double, operation by operation. */
int spnet_augment_params(unsigned seed, unsigned epoch, const int* sample, int B, int H, int W, int n_salt, int n_pepper,
                         const float* mm, int n_frames, int* rects, float* vals, int* nrect, int* coords, int* flag,
                         int* ksize, int Hw, int Ww, const double* trig, void* warp_records, double* fwd, void* stream);
/* Dropout(0.1) of the stem (spnet/models.py:340); same call with dy regenerates the mask in backward. */
int spnet_dropout(const float* x, float* y, long n, unsigned seed, float rate, const unsigned* seed_dev,
                  void* stream);   /* seed_dev (or NULL): device uint32 overriding seed (hipGraph replay) */

/* ---- synthetic input (gen_fake_espi.py:60-279 without the band-pass mix-up) -------------------------------- */
/* Rasterises N fake-ESPI frames in device memory from host-drawn parameters: waves [N][5] = amp, wavelength,
 * thickness, slope, spacing (draw_waves :60-80); nodes [N][7][8] = cx, cy, a, b, angle_deg, rings, start, valid
 * (draw_antinodes :145-206, draw_rings :101-114); nnode [N].  noise != 0 adds the clipped N(40,40) noise and the
 * 50 % pixel dropout (gen_images :255-263).  out_f (or NULL): [N][H][W] network input in [-1,1]; out_u8 (or NULL):
 * the uint8 frame. */
int spnet_fake_espi(const float* waves, const float* nodes, const int* nnode, int N, int H, int W, unsigned seed,
                    int noise, float* out_f, unsigned char* out_u8, void* stream);
/* The parameters themselves, drawn on the device (csrc/espi_params.hip): writes waves [N][5], nodes [N][7][8] (every
 * element; unused slots are zeros, valid = column 7) and nnode [N] for the global frames first_frame .. first_frame + N - 1,
 * in the layout spnet_fake_espi reads.  Same logic as the host's draw_params (draw_waves, gen_fake_espi.py:60-80;
 * draw_antinodes :145-206), its own random stream.  tries (or NULL) [N][7]: per antinode DRAWN, the try that was accepted,
 * -1 = dropped after 2000 tries, -2 = not drawn (index >= the frame's count).  trig2 [181][2] = (cos^2, sin^2) of the whole
 * degrees 0..180, computed in float64 and rounded to float.  N == 0: nothing to do, success.  hipErrorInvalidValue (nothing
 * launched): N < 0, first_frame < 0, H or W outside 64 .. 2048, count_lo < 0, count_lo > count_hi, count_hi > 7, a NULL
 * trig2 / waves / nodes / nnode.
 * The stream, stateless and counter based -- frame g's parameters depend on (seed, g) only:
 *   mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (uint32)
 *   fkey(g) = mix(mix(mix(seed ^ 0x9e3779b9) + low32(g)) ^ high32(g))
 *   key(slot, t) = mix(fkey + (slot << 12 | t)): slot 0 = the frame's draws (t = 0), slot j + 1 = antinode j, try t
 *   u(key, k) = mix(key ^ (k * 0x85ebca6b + 0xc2b2ae35)), draw index k
 *   randint(u, lo, hi) = lo + ((uint64)u * max(hi - lo + 1, 1) >> 32)              (an empty range gives lo)
 *   frame (slot 0): k 0 amp [10, 200]; 1 wavelength [100, W/2]; 2 thick [15, 40]; 3 U = (u >> 8) * 2^-24, slope =
 *     3 * (U - 0.5) in float; 4 spacing [thick + thick * int(|1.5 * slope|), H/3]; 5 count [count_lo, count_hi]
 *   antinode j, try t (0 .. 1999): k 0, 1 the axes, [15, 2W/7] and [15, 2H/7] at t = 0, [25, W/3] and [25, H/3] at t > 0 (integer
 *     divisions), a = the larger, b = the smaller; k 2 (t = 0 only) rings [1, min(b/8, 11)]; k 3 cx [a, W - a]; k 4 cy
 *     [b, H - b]; k 5 angle [1, 179] at t = 0, [1, 180] at t > 0; k 6 of t = 0: start = u >> 31
 *   box of a try: dx = sqrt(a^2 cos^2 + b^2 sin^2), dy = sqrt(a^2 sin^2 + b^2 cos^2) in float, each product and sum rounded
 *     on its own, the root correctly rounded; x0 = cx - dx, x1 = cx + dx, y0, y1 likewise.  The try passes when
 *     x0 >= 0, x1 <= W, y0 >= 0, y1 <= H and no accepted box q of the frame has NOT (x1 < q.x0 | x0 > q.x1 | y1 < q.y0 | y0 > q.y1).
 *   The first passing try is accepted; its ring count is min(rings drawn at t = 0, b_s / 4 of every try s <= t). */
int spnet_fake_espi_params(long first_frame, int N, int H, int W, unsigned seed, int count_lo, int count_hi,
                           const float* trig2, float* waves, float* nodes, int* nnode, int* tries, void* stream);
/* Strike sequences (csrc/espi_strike.hip): a movie with KNOWN identities and ring-count curves.  A sequence
 * is one set of frame-0 parameters -- waves0 [S][5], nodes0 [S][7][8], nnode0 [S] as spnet_fake_espi_params writes them,
 * row s for the GLOBAL sequence first_sequence + s -- evolved over T frames.  Writes (every element) waves [S*T][5],
 * nodes [S*T][7][8], nnode [S*T] in the layout spnet_fake_espi reads, and ident int32 [S*T][7]; frame s * T + t is time
 * step t of sequence s.  Integer and stateless: slot (s, t, j) is a function of (seed, first_sequence + s, t, j) and the
 * base row alone, one thread per slot; a frame does not depend on S or on how a range of sequences is split into calls.
 *   mix, u(key, k), randint as for spnet_fake_espi_params above (csrc/counter_rng.h)
 *   skey(g) = mix(mix(mix(seed ^ 0x51ed270b) + low32(g)) ^ high32(g)), g = first_sequence + s
 *   key(slot, t) = mix(skey + (slot << 12 | t)): slot 0 with t = j = the envelope draws of antinode j, slot j + 1 = the
 *     jitter draws of antinode j at time t
 *   base slot j is VALID iff j < clamp(nnode0[s], 0, 7) and its column 7 is not 0; the first valid slot is the STRUCK
 *     note: onset 0, rise 0.  Every other valid slot is sympathetic: k 0 onset [0, T/2]; k 1 rise [1, max(T/4, 1)].  All:
 *     k 2 hold [0, T/4]; k 3 decay [1, T]  (integer divisions)
 *   envelope e(t) in 0 .. 256, peak = onset + rise, after = peak + hold + 1: 0 for t < onset;
 *     256 (t - onset + 1) / (rise + 1) for t < peak; 256 for t < after; max(256 - 256 (t - after + 1) / (decay + 1), 0)
 *     from then on (integer divisions).  It rises, holds and falls: unimodal
 *   rings(t) = (R e(t) + 128) >> 8 with R = the base row's ring count clamped to 0 .. 255; the antinode is PRESENT at t
 *     iff rings(t) >= 1 -- one contiguous run of frames
 *   present: cx = cx0 + randint(u(key(j + 1, t), 0), -J, J), cy = cy0 + randint(u(.., 1), -J, J) (whole numbers added to
 *     whole numbers: exact floats); axes, angle and start are the base row's; column 5 = rings(t); valid = 1;
 *     ident = 1 + 7 g + j.  absent: the slot's eight floats are 0 (valid = 0: the rasteriser skips it) and ident = 0
 *   waves are the base row's; nnode = clamp(nnode0[s], 0, 7) in every frame
 * S == 0: nothing to do, success.  hipErrorInvalidValue (nothing launched): a NULL pointer, S < 0, first_sequence < 0, T
 * outside 1 .. 4096, J outside 0 .. 8, S * T > 2^31 - 1, 7 (first_sequence + S) > 2^31 - 2.
 * ADDENDUM, the sequence's SOUND (host only: spnet_amd/fake_espi.py strike_audio_host; no kernel implements it, and no
 * frame or label above depends on it).  hop = rate / fps samples per frame as an exact rational hop_num / hop_den; a
 * sequence is floor(T * hop_num / hop_den) samples of int16.  Draws 4 and up of key(0, j) are free (0 .. 3 are the envelope):
 *   pitch_j = 60 + 5 j + randint(u(key(0, j), 4), 0, 2) (MIDI: adjacent slots at least 3 semitones apart); f_j = 440 *
 *     2^((pitch_j - 69) / 12) in double; step_j = round(f_j / rate * 2^32), the note step of "Note envelopes"
 *   lag_j = 0 for the struck slot, the caller's lag (0 .. 64 frames) for a sympathetic one: the sound of a sympathetic note
 *     follows its rings by lag frames
 *   e_j(n) = the envelope above at frame floor(n * hop_den / hop_num) - lag_j (0 before the onset, so for a negative frame)
 *   sample n = ((sum over VALID slots of R_j * e_j(n) * ctab[((((uint32)(n * step_j)) >> 20) + 3072) & 4095]) >> 18) +
 *     randint(u(nkey, low32(n)), -noise, noise), nkey = u(key(0, 0), 5), noise 0 .. 1024; >> is an arithmetic shift.  Seven
 *     slots at R = 255 and e = 256 give at most 7 * 255 * 256 * 16384 >> 18 = 28,560, with the noise below 32,767: no clipping */
int spnet_fake_espi_strike(const float* waves0, const float* nodes0, const int* nnode0, long first_sequence, int S, int T,
                           unsigned seed, int J, float* waves, float* nodes, int* nnode, int* ident, void* stream);

/* ---- band-pass mix-up (spnet/augmentation.py:10-62; csrc/bandpass.hip) ------------------------------------------- */
/* Frames x [*][H][W], one channel, 16 <= H, W <= 2048; x_kind 0 = uint8, 1 = fp32 pixel units (0..255), 2 = fp32 network
 * units ([-1,1], pixel = (x/2 + 1/2) * 255, each operation rounded on its own: the bits of x_kind 1 on those pixels).
 * A window is the 16 x 16 block of the centred spectrum, frequencies k, l in [-8, 8), as [16][16] complex (re, im) fp32,
 * row k + 8, column l + 8.  ws: spnet_bandpass_ws(N, H, W) floats (-1 = the dimensions are not supported).
 *   spnet_bandpass_project  win[n] = window of x[n] after cv2.flip(x[n], flip[n]) (flip NULL or a code outside
 *                           {-1, 0, 1}: not flipped) -- the real-image table of the mix-up.
 *   spnet_bandpass_apply    frame m = x[sel[m]] (sel NULL: x[m]; sel clamped to [0, n_src)), mixed with window
 *                           table[row[m]] (row clamped to [0, n_table)) scaled by s[m]; the complex magnitude of the
 *                           inverse, min-max normalised to [0, 255] (a constant becomes 0), clipped.  Written to the same
 *                           frame index of out_f (f_kind 0 = pixel units, 1 = network units) and / or out_u8 (round half to
 *                           even, saturated).  out_f may be x (fp32 kinds) and out_u8 may be x (uint8) when sel holds no
 *                           index twice.  Deterministic: a frame's bits do not depend on the batch around it. */
long spnet_bandpass_ws(int N, int H, int W);
int spnet_bandpass_project(const void* x, int x_kind, int N, int H, int W, const int* flip, float* win, float* ws,
                           void* stream);
int spnet_bandpass_apply(const void* x, int x_kind, const int* sel, int n_src, int N, int H, int W, const float* table,
                         int n_table, const int* row, const float* s, float* out_f, int f_kind, unsigned char* out_u8,
                         float* ws, void* stream);

/* ---- keras DenseNet121 (csrc/densenet.hip, gemm.hip; call site spnet/models.py:357-359 with cf.basemodel = 'DenseNet121') */
/* Y[M,N] (row stride ldy) = relu(x[:, :K]*scale + shift) W[K,N]: BatchNorm + ReLU of the block's Concatenate buffer (pixels
 * ldx floats apart) applied while the A tile is staged.  coef = [scale | unused | shift], cld floats each, zero beyond
 * channel K-1 (spnet_dense_coeffs writes it).  colstats / stat_rows (or NULL / NULL) as spnet_gemm_f32_colstats. */
int spnet_gemm_f32_bnrelu(const float* x, int ldx, const float* coef, int cld, const float* W, int ldw, float* Y, int ldy,
                          int M, int N, int K, int tile, float* colstats, int* stat_rows, void* stream);
/* ZeroPadding2D: backward = 0 pads x [B][H][W][C] into [B][H+pt+pb][W+pl+pr][C]; backward = 1 crops such a tensor back. */
int spnet_pad_nhwc(const float* in, float* out, int B, int H, int W, int C, int pt, int pb, int pl, int pr, int backward,
                   void* stream);
/* ZeroPadding2D(3) + Conv2D(64, 7, strides 2, valid) on the 3-channel stem output (conv1/conv): op 0 fwd (a = x, b = w),
 * 1 data gradient (a = dy, b = w), 2 weight gradient (a = x, b = dy; workspace >= spnet_dense_conv7_ws floats).  H, W:
 * the input plane; output (H-1)/2+1 x (W-1)/2+1. */
long spnet_dense_conv7_ws(int B, int H, int W);
int spnet_dense_conv7(int op, const float* a, const float* b, float* out, int B, int H, int W, float* workspace,
                      long ws_floats, void* stream);
/* Column sums (sum, sum of squares) of x [M][C] (row stride ldx) as partial[spnet_dense_rows(M)][2][C] rows, the input of
 * spnet_bn_finalize_fwd: the batch statistics of a dense block's input channels.  Partial row p holds the rows (pixels)
 * 64p .. 64p+63 of x (the last one fewer when M % 64 != 0); spnet_dense_rows(M) = ceil(M / 64). */
long spnet_dense_rows(long M);
int spnet_dense_colsums_ld(const float* x, long ldx, long M, int C, float* partial, void* stream);
/* Affine of one consumer BatchNorm over channels [0, c) as coef = [scale | 0 | shift] (cld floats each, zero from c on):
 * training = 1 from the shared batch statistics (mean, invstd) + moving update of (mm, mv) towards (bmean, bvar);
 * training = 0 from (mm, mv). */
int spnet_dense_coeffs(int c, int cld, const float* gamma, const float* beta, const float* mean, const float* invstd,
                       const float* bmean, const float* bvar, float* mm, float* mv, float* coef, float eps, float momentum,
                       int training, void* stream);
/* y = act(scale*x + shift) over C channels (act 0 none, 1 ReLU), strided input and output. */
int spnet_dense_apply_ld(const float* x, long ldx, long M, int C, const float* coef, int cld, int relu, float* y, long ldy,
                         void* stream);
/* Consumer backward: g = dz * [scale*x + shift > 0] (relu) | dz; G[:, :c] += gamma*g; partial[spnet_dense_rows(M)][2][c]
 * = (sum g, sum g*x^), partial row p over the pixels 64p .. 64p+63 (dense rows of c floats).  spnet_dense_consumer_fin:
 * dbeta = sum g, dgamma = sum g*x^ over P such rows, u += gamma*dbeta, v += gamma*dgamma. */
int spnet_dense_consumer_bwd(const float* dz, long ldz, const float* x, long ldx, long M, int c, const float* coef, int cld,
                             const float* mean, const float* invstd, const float* gamma, int relu, float* G, long ldg,
                             float* partial, void* stream);
int spnet_dense_consumer_fin(const float* partial, int P, int c, const float* gamma, float* dgamma, float* dbeta, float* u,
                             float* v, void* stream);
/* Producer finalize: out[:, j - c0] = invstd*(G - u/M - x^*v/M) for c0 <= j < c1 (the summed BatchNorm backward of every
 * consumer of those channels). */
int spnet_dense_producer_fin(const float* G, long ldg, const float* u, const float* v, const float* x, long ldx,
                             const float* mean, const float* invstd, long M, int c0, int c1, float* out, long ldo,
                             void* stream);

/* ---- PNG output (csrc/png.hip): the encoder behind cv2.imwrite (gen_fake_espi.py:274-275, augment_preproc.py:99,
 *      spnet/utils.py:132) for frames that are already in device memory ------------------------------------------------- */
/* src: N uint8 frames [N][H][W][channels], channels 1 .. 4 (PNG colour types 0, 4, 2, 6 at 8 bits), no alignment asked.  The
 * FILTERED STREAM of a frame is PNG's scanline stream with filter type 0 on every row: H rows of 1 + W*channels bytes,
 * at most 2^27 bytes.  Both entries run one workgroup per frame; spnet_amd/png.py is the host side (code lengths, header
 * bits, offsets, container).  N == 0: nothing to do, success.  hipErrorInvalidValue (nothing launched) for a shape outside
 * these limits, a NULL pointer, or a word array that is not 4-byte aligned (offsets: 8-byte).
 *   spnet_png_hist  hist [N][256] = byte counts of the filtered stream (the H filter bytes are in bin 0); adler [N] = its
 *                   Adler-32 (sums modulo 65521, formed so that no 32-bit intermediate can overflow at any allowed size).
 *   spnet_png_pack  writes the complete zlib stream of frame n at out + offsets[n]: 0x78 0x01, ONE final dynamic-Huffman
 *                   deflate block (header bits, one code per byte of the filtered stream, end of block; no length or
 *                   distance code), zero bits up to a byte boundary, adler[n] most significant byte first.
 *                   codes [N][257]: canonical code of symbol s (RFC 1951 3.2.2, most significant code bit in the highest
 *                   of its bits) | length << 16, lengths 0 .. 15; the kernel reverses the bits.  header [N][64]: the block
 *                   header from BFINAL up to the last code length, bit i of the stream in bit i % 32 of word i / 32;
 *                   header_bits [N] <= 2048.  offsets [N + 1] (64-bit): frame n may write bytes offsets[n] .. offsets[n+1]
 *                   - 1 only and anything that does not fit is dropped, as is a frame whose slot is not inside
 *                   [0, out_bytes); the host sizes the slots exactly (2 + ceil((header_bits + sum hist*length + length of
 *                   256) / 8) + 4 bytes).  out: 4-byte aligned, out_bytes a multiple of 4, ZEROED by the caller: bits are
 *                   merged with 32-bit atomic OR (stream order protects it; the call does not clear it).  Bytes outside
 *                   the slots are not changed.  The bytes do not depend on the order threads run in. */
int spnet_png_hist(const unsigned char* src, int N, int H, int W, int channels, uint32_t* hist, uint32_t* adler, void* stream);
int spnet_png_pack(const unsigned char* src, int N, int H, int W, int channels, const uint32_t* codes, const uint32_t* header,
                   const int* header_bits, const long long* offsets, const uint32_t* adler, unsigned char* out, long out_bytes,
                   void* stream);

/* The LZ77 stage (csrc/png_lz.hip; opt-in, lz77=True of spnet_amd/png.py): the same frames, stream and limits, one workgroup
 * per frame, tokens (literals and (length 3 .. 258, distance 1 .. 32768) matches) by the fixed rule in that file's header --
 * a function of the stream alone.  No HBM workspace: the packer recomputes the tokens.
 *   spnet_png_lz_scan  lhist [N][286] = counts of the literal / length symbols of the frame's tokens (symbol 256, the end of
 *                      block, counted once), dhist [N][30] = counts of the distance symbols.  Both 4-byte aligned.
 *   spnet_png_lz_pack  as spnet_png_pack (same out / out_bytes / offsets / adler contract, same zlib header bytes), with both
 *                      alphabets: lcodes [N][286] and dcodes [N][30] (code | length << 16, lengths 0 .. 15), header [N][72]
 *                      (real HLIT / HDIST; header_bits [N] <= 2304).  A frame with header_bits[n] < 0 is SKIPPED: its slot
 *                      is left to spnet_png_pack, which may share words with its neighbours' (both merge with OR).  Slot
 *                      size: 2 + ceil((header_bits + sum lhist*length + sum dhist*length + the symbols' extra bits) / 8) + 4. */
int spnet_png_lz_scan(const unsigned char* src, int N, int H, int W, int channels, uint32_t* lhist, uint32_t* dhist,
                      void* stream);
int spnet_png_lz_pack(const unsigned char* src, int N, int H, int W, int channels, const uint32_t* lcodes,
                      const uint32_t* dcodes, const uint32_t* header, const int* header_bits, const long long* offsets,
                      const uint32_t* adler, unsigned char* out, long out_bytes, void* stream);

/* ---- PNG input (csrc/png_decode.hip, csrc/inflate_core.h): the decoder behind Image.open(...).convert("RGB")
 *      (spnet/utils.py:325-345) for files whose bytes are uploaded as they sit on disk ---------------------------------- */
/* One wave per file; spnet_amd/png.py is the host side (container, CRCs, classification, host fallback).  status [N]
 * (int32) holds inflate_core.h's inflate::Status per file: 0 = decoded, non-zero = that file's work ended there (1 bad zlib
 * header, 2 reserved block type, 3 LEN/NLEN mismatch, 4 over-subscribed / incomplete code, 5 invalid symbol, 6 distance
 * before the start of the output, 7 input exhausted, 8 output longer than L, 9 output shorter than L, 10 Adler-32
 * mismatch, 11 filter type above 4, 12 extent outside the blob); the other files of the launch are not affected.  N == 0:
 * nothing to do, success.  hipErrorInvalidValue (nothing launched) for a NULL pointer, a misaligned offsets / status
 * array or a size outside the limits below.
 *   spnet_png_inflate   blob: the zlib streams (concatenated IDAT payloads) of N files, file n in bytes offsets[n] ..
 *                       offsets[n+1] - 1 of the blob_bytes bytes (64-bit offsets, 8-byte aligned; a stream is at most 2^30
 *                       bytes).  Accepts all of RFC 1950 / 1951 without a preset dictionary.  L = H * (1 + W * channels)
 *                       <= 2^27 is the length every stream must inflate to; file n's filtered scanline stream is written
 *                       to out + n * out_stride (out_stride >= L).  No byte before blob + offsets[n] or at or after blob +
 *                       offsets[n+1] is read for file n; no byte outside out + n * out_stride .. + L - 1 is written; of a
 *                       file with non-zero status a prefix of its slot may have been written.  Writes every status[n].
 *   spnet_png_unfilter  inflated: the streams as written above (in_stride >= L); files whose status is non-zero are
 *                       skipped.  channels (bytes per pixel) 1 .. 4, W * channels <= 32768.  first (may be NULL): uint8
 *                       [N][H][W], channel 0 of every pixel; all (may be NULL): uint8 [N][H][W][channels]; at least one.
 *                       A filter type above 4 sets status[n] = 11 and ends that file (rows above it are written). */
int spnet_png_inflate(const unsigned char* blob, long blob_bytes, const long long* offsets, int N, long L, long out_stride,
                      unsigned char* out, int* status, void* stream);
int spnet_png_unfilter(const unsigned char* inflated, long in_stride, int N, int H, int W, int channels, unsigned char* first,
                       unsigned char* all, int* status, void* stream);

/* ---- prediction overlays (csrc/overlay.hip): the drawing of show_pred_ellipses (spnet/utils.py:67-137: cv2.ellipse,
 *      cv2.putText per frame) for frames that are already in device memory ---------------------------------------------- */
/* frames: uint8 [N][H][W] (channels 1: grey, replicated to R = G = B) or [N][H][W][3] (channels 3); out: uint8
 * [N][H][W][3], a different buffer.  H, W 1 .. 4096.  spnet_amd/overlay.py is the host side and documents the rule.
 *   frame_start int32 [N+1]   commands of frame n are cmd[frame_start[n] .. frame_start[n+1]), painted in that order
 *   cmd         int32 [n_cmd][12]   kind (0 outline, 1 mask blit), colour r | g << 8 | b << 16, box x0, y0, x1, y1 (pixels,
 *                             x1 / y1 exclusive; nothing outside box and frame is touched; an empty box paints nothing),
 *                             data, mask x, mask y, mask width, mask height, 0
 *   verts       int32 [n_verts][2]  outline: data = index of the first of its 72 vertices (x, y in 1/16 pixel, pixel (x, y)
 *                             has its centre at (16 x + 8, 16 y + 8)); closed polygon, every edge a segment of half width
 *                             24/16 pixel with round ends, in exact integer arithmetic; the pixel takes the colour.  Edges
 *                             must be shorter than 2^13 units per axis (the host gives longer ones an empty box).
 *   masks       uint8 [mask_bytes]  blit: data = byte offset of a width x height coverage mask whose top-left pixel is at
 *                             (mask x, mask y), which may lie outside the frame; per channel t = dst * (255 - m) + ink * m
 *                             + 128, out = ((t >> 8) + t) >> 8.
 * A command whose data points outside verts / masks is skipped; no byte outside the arrays as sized here is read, none
 * outside out written.  One launch (per 65,535 frames), one workgroup per 64 x 16 tile; 16-byte accesses on untouched tiles
 * when W % 16 == 0 and frames / out are 16-byte aligned (no alignment is required).  N == 0: nothing to do, success.
 * hipErrorInvalidValue (nothing launched) for a size outside these limits, a NULL pointer or a misaligned int32 array. */
int spnet_draw_overlays(const unsigned char* frames, int N, int H, int W, int channels, const int* frame_start, const int* cmd,
                        int n_cmd, const int* verts, int n_verts, const unsigned char* masks, long mask_bytes,
                        unsigned char* out, void* stream);

/* ---- JPEG output (csrc/jpeg.hip): a lossy writer for the overlays show_pred_ellipses leaves behind (spnet/utils.py:132) and
 *      the frames of the README's "Making a movie", for frames that are already in device memory ------------------------- */
/* src: N uint8 frames [N][H][W][channels], no alignment asked.  channels 1: one component (grey); channels 3: RGB, coded as
 * YCbCr 4:4:4 in interleaved MCUs of Y, Cb, Cr.  Baseline sequential DCT, 8 bit.  1 <= H, W <= 65,535 (SOF0's limit; no
 * smaller bound on W) and N * intervals <= 2^31 - 1.  spnet_amd/jpeg.py is the host side (quantisation tables, header
 * segments, offsets, EOI, the AVI container).  N == 0: nothing to do, success.  hipErrorInvalidValue (nothing launched) for a
 * shape outside these limits, channels other than 1 or 3, a NULL pointer, qtables not 2-byte, sizes not 4-byte or offsets not
 * 8-byte aligned.
 *
 * RESTART INTERVALS.  An MCU is one 8 x 8 block of every component; a frame has ceil(W/8) * ceil(H/8) of them in raster order
 * (H and W are padded to the 8-grid by replicating the last row and column).  The scan is cut into intervals of
 *     Ri = spnet_jpeg_restart_interval(W, channels) = min(ceil(W / 8), 64)
 * MCUs -- one MCU row, capped at 64 (a wave owns an interval, a lane an MCU); the last interval may be shorter, and when
 * ceil(W/8) > 64 intervals run across row ends.  spnet_jpeg_intervals(H, W, channels) = ceil(MCUs / Ri) is their number
 * (both queries: -1 outside the limits).  An interval starts with all DC predictors 0, ends with 1-bits up to a byte
 * boundary, and every 0xFF byte of it is followed by 0x00.  Interval i < intervals - 1 is followed by the marker FF D0+(i mod
 * 8); nothing follows the last one.
 *
 * ARITHMETIC, integers only (>> is an arithmetic shift, / a truncating division of non-negative numbers):
 *   colour   Y  = ( 19595 R + 38470 G +  7471 B + 32768) >> 16
 *            Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16          (8421375 = 128 * 2^16 + 2^15 - 1)
 *            Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16          each clamped to 0 .. 255; grey: the sample itself
 *   kernel   K[u][x] = rint(2^12 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u > 0) = 1/2: rows 1448 x 8; 2009 1703
 *            1138 400 -400 ..; 1892 784 -784 -1892 -1892 ..; 1703 -400 -2009 -1138 1138 ..; 1448 -1448 -1448 1448 ..; 1138
 *            -2009 400 1703 -1703 ..; 784 -1892 1892 -784 -784 ..; 400 -1138 1703 -2009 2009 ..   (sum of |row| <= 11584)
 *   rows     p[y][u] = (sum_x K[u][x] (s[y][x] - 128) + 2^8) >> 9        |sum| <= 11584 * 128 < 2^21; 3 fractional bits
 *   columns  q[v][u] = sum_y K[v][y] p[y][u]                             |p| <= 2896, |q| <= 11584 * 2896 < 2^25; 15 fractional bits
 *   quantise c = sign(q) * ((|q| + (Q << 14)) / (Q << 15))               half away from zero; Q = qtables entry v * 8 + u
 *            computed as ((|q| >> 14) + Q) / 2Q -- the same number, since the dropped 14 bits cannot carry a multiple of
 *            2Q * 2^14 -- with the division as (n * ceil(2^24 / 2Q)) >> 24, exact for every n < 2^14 and Q 1 .. 255.
 *   coding   T.81 F.1.2 with the Annex K tables K.3 - K.6: DC difference to the component's previous block in the interval,
 *            size category, (run, size) symbols, ZRL for 16 zeros, EOB unless coefficient 63 is non-zero; bits fill bytes from
 *            the most significant bit.
 * A frame's bytes are a function of its pixels and qtables alone: not of N, of the frame's place in the batch or of the order
 * threads run in.
 *   spnet_jpeg_scan  qtables uint16 [2][64]: luminance then chrominance, natural order (row v, column u), entries clamped to
 *                    1 .. 255 (channels 1 reads the first table only, but both must be there).  sizes uint32 [N][intervals]:
 *                    the exact bytes of every interval's entropy-coded data, stuffing and final padding included, markers
 *                    excluded.
 *   spnet_jpeg_pack  the same inputs, sizes as spnet_jpeg_scan wrote them (still in device memory) and offsets [N + 1]
 *                    (64-bit).  Writes frame n's whole scan -- interval 0, RST0, interval 1, ... -- at out + offsets[n]; the
 *                    host sizes the slot exactly (sum of the frame's sizes + 2 * (intervals - 1)).  Frame n may write bytes
 *                    offsets[n] .. offsets[n+1] - 1 only and anything that does not fit is dropped, as is a frame whose slot
 *                    is not inside [0, out_bytes).  Every byte has one writer (plain byte stores, no merging): out need not
 *                    be zeroed or aligned, and bytes outside the slots are not changed.  The coefficients are RECOMPUTED;
 *                    there is no workspace. */
long spnet_jpeg_restart_interval(int W, int channels);
long spnet_jpeg_intervals(int H, int W, int channels);
int spnet_jpeg_scan(const unsigned char* src, int N, int H, int W, int channels, const uint16_t* qtables, uint32_t* sizes,
                    void* stream);
int spnet_jpeg_pack(const unsigned char* src, int N, int H, int W, int channels, const uint16_t* qtables, const uint32_t* sizes,
                    const long long* offsets, unsigned char* out, long out_bytes, void* stream);

/* ---- JPEG input (csrc/jpeg_decode.hip, csrc/jpeg_decode_core.h): the decoder behind Image.open(f).convert("RGB")
 *      (spnet/utils.py:325-345) for baseline JPEG files and the frames of a Motion-JPEG movie whose entropy-coded bytes sit
 *      in device memory --------------------------------------------------------------------------------------------------- */
/* Baseline sequential DCT (SOF0), 8 bit, one scan; one component, or three (YCbCr) with luma sampled 1x1, 2x1 or 2x2 and
 * chroma 1x1.  spnet_amd/jpeg.py is the host side (marker walk, classification, table building, host fallback).  N == 0:
 * nothing to do, success.  hipErrorInvalidValue (nothing launched) for a NULL pointer, a misaligned array (int32 / uint32
 * arrays 4 bytes, quant 2, coef 16) or a size outside the limits below.
 *
 * TABLES the host builds (all int32 unless said otherwise):
 *   intervals [n_intervals][8]  first byte, end byte (positions in blob; the interval's entropy-coded data WITHOUT the RST
 *                               marker behind it), file, first MCU, MCUs, 0, 0, 0.  A file without restart markers is one
 *                               interval.  The 64 intervals of a workgroup (64 i .. 64 i + 63) must belong to files of ONE
 *                               table set -- the host pads each set's run with empty intervals (MCUs 0) -- or they get
 *                               status 6.
 *   files [n_files][16]         components (1 | 3), hs, vs (luma sampling; 1 1 | 2 1 | 2 2), MCU columns, MCU rows, table
 *                               set, first block of the file in the workspace, 0, (DC table | AC table << 4) of each
 *                               component (table 0 | 1), quantisation table of each component (index into quant), 0, 0
 *   tables uint32 [n_sets][904] a set is DC 0, AC 0, DC 1, AC 1; a table is look uint16 [256] (length << 8 | symbol of every
 *                               code of up to 8 bits, indexed by the next 8 bits; 0: longer, or none), maxcode int32 [17]
 *                               (largest code of each length 1 .. 16, -1: none), valoff int32 [17] (index of the length's
 *                               first symbol minus its first code), vals uint8 [256].  A table the file lacks is all
 *                               zeros / -1: using it is status 1.
 *   quant uint16 [n_quant][64]  natural order (row v, column u)
 *   coef int16 [total_blocks][64]  the workspace, natural order, ZEROED by the caller; a file's blocks are component after
 *                               component, each in raster order of its block grid (MCU columns * h by MCU rows * v)
 * blob_bytes < 2^31 - 1024, total_blocks < 2^25.
 *
 * ENTROPY DECODING (T.81 F.2.2), one lane per interval: bits are read most significant first; FF 00 is the data byte FF; an
 * FF followed by anything else ends the data.  MCUs in raster order, inside an MCU the hs * vs luma blocks row by row, then
 * Cb, then Cr.  Per block: a DC category s (<= 11), s bits EXTENDed (v if its top bit is set, else v - 2^s + 1) added to the
 * component's predictor (0 at the interval's start); then (run, s) symbols: 0/0 ends the block, 15/0 skips 16 coefficients,
 * else (s <= 10) k += run and coefficient k of the zigzag sequence is the next s bits EXTENDed.  status [n_files] (written
 * for every file: 0 first, then the largest code of the file's intervals) holds jpegdec::Status:
 *   1 a bit pattern that is no code   2 k past 63   3 a category above 11 (DC) / 10 (AC)   4 bits missing before the
 *   interval's MCUs are done   5 a whole byte or more left over after them   6 a table entry outside the arrays above
 * and that interval stops there.  No byte outside [first byte, end byte) is read for an interval, no coefficient outside the
 * blocks of its own MCUs written, every loop is bounded by a count that does not depend on the data; the other files of the
 * launch are not affected.
 *
 * PIXELS, integers only (>> is an arithmetic shift):
 *   dequantise  c[v][u] * quant[v][u]
 *   IDCT        libjpeg's jidctint.c ("islow"), CONST_BITS 13, PASS1_BITS 2, the same butterfly twice: with the constants
 *               FIX(0.298631336) = 2446, 0.390180644: 3196, 0.541196100: 4433, 0.765366865: 6270, 0.899976223: 7373,
 *               1.175875602: 9633, 1.501321110: 12299, 1.847759065: 15137, 1.961570560: 16069, 2.053119869: 16819,
 *               2.562915447: 20995, 3.072711026: 25172,
 *                 even: z1 = (x2 + x6) 4433; t2 = z1 - 15137 x6; t3 = z1 + 6270 x2; t0 = (x0 + x4) << 13; t1 = (x0 - x4) << 13;
 *                       t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
 *                 odd:  z1 = x7 + x1; z2 = x5 + x3; z3 = x7 + x3; z4 = x5 + x1; z5 = 9633 (z3 + z4);
 *                       z3 = z5 - 16069 z3; z4 = z5 - 3196 z4;
 *                       o0 = 2446 x7 - 7373 z1 + z3; o1 = 16819 x5 - 20995 z2 + z4; o2 = 25172 x3 - 20995 z2 + z3;
 *                       o3 = 12299 x1 - 7373 z1 + z4
 *                 out:  t10 +- o3 -> 0, 7; t11 +- o2 -> 1, 6; t12 +- o1 -> 2, 5; t13 +- o0 -> 3, 4; each (s + 2^(n-1)) >> n
 *               down every column with n = 11, then along every row with n = 18; sample = clamp(result + 128, 0, 255).
 *               Sums are formed modulo 2^32.  (libjpeg masks into a table where this clamps: the same on every stream an
 *               encoder writes.)
 *   upsampling  libjpeg's "fancy" triangle filter over the chroma component's TRUE samples (ceil(W / hs) by ceil(H / vs)),
 *               neighbours beyond an edge replaced by the edge sample.  2x1: pixel x takes i = x >> 1 and j = i - 1 (x
 *               even) or i + 1 (x odd): (3 s[i] + s[j] + 1 + (x & 1)) >> 2.  2x2: rows r = y >> 1 and rn = r - 1 (y even) or
 *               r + 1 (y odd) first, t[i] = 3 s[r][i] + s[rn][i]; then (3 t[i] + t[j] + 8 - (x & 1)) >> 4.
 *   colour      Cb' = Cb - 128, Cr' = Cr - 128; R = Y + ((91881 Cr' + 32768) >> 16), G = Y + ((-22554 Cb' - 46802 Cr' +
 *               32768) >> 16), B = Y + ((116130 Cb' + 32768) >> 16), each clamped to 0 .. 255.  One component: the sample.
 *   spnet_jpeg_pixels  H, W (1 .. 65,535): the size of EVERY file of the launch (a file whose MCU grid does not fit it gets
 *               status 6); files whose status is non-zero are skipped.  first (may be NULL): uint8 [N][H][W], channel 0 of
 *               what convert("RGB") gives (Y of a grey file, R of a colour file); all (may be NULL): uint8 [N][H][W]
 *               [channels], channels = the files' component count (another count: status 6); at least one.  No byte outside
 *               them is written, none of a skipped file's frame. */
int spnet_jpeg_entropy(const unsigned char* blob, long blob_bytes, const int* intervals, int n_intervals, const int* files,
                       int n_files, const uint32_t* tables, int n_sets, int16_t* coef, long total_blocks, int* status,
                       void* stream);
int spnet_jpeg_pixels(const int16_t* coef, long total_blocks, const int* files, int n_files, const uint16_t* quant,
                      int n_quant, int H, int W, int channels, unsigned char* first, unsigned char* all, int* status,
                      void* stream);

/* spnet_jpeg_entropy_sync (csrc/jpeg_decode_sync.hip, csrc/jpeg_sync_core.h): spnet_jpeg_entropy's decoding of the same
 * tables into the same workspace, for intervals that are too long for one lane (a file without restart markers is ONE
 * interval): ONE WORKGROUP PER INTERVAL, a lane per segment of seg_bytes bytes (a multiple of 4 in 4 .. 4096; else
 * hipErrorInvalidValue, as for the argument errors of spnet_jpeg_entropy).  The intervals need no grouping by table set
 * and no padding; an interval with MCUs 0 is skipped.  The result is spnet_jpeg_entropy's, coefficient for coefficient and
 * status for status, whatever seg_bytes is.  Recipe:
 *   segment      bytes [first + i seg_bytes, first + (i + 1) seg_bytes) of the interval; it OWNS every symbol (code and
 *                magnitude bits) whose first bit lies in it, the last segment also what starts at the interval's end
 *   state        between two symbols: position of the next bit (byte, bit; at a byte boundary the next DATA byte, never a
 *                stuffed 00), the block's index in the MCU, the zigzag position k (0: a DC symbol is next)
 *   first pass   segment 0 from the true state (bit 0, block 0, k 0), every other from a guess: its first bit -- one byte
 *                later where its first byte is the 00 stuffed behind the previous segment's FF --, block 0, k 0.  A lane
 *                decodes the symbols it owns (the reader is bounded by the interval's end, not the segment's) and notes its
 *                exit state, the blocks that FINISHED, per component the sum of the DC differences (modulo 2^32) and
 *                whether it met one of the errors 1 .. 4; an error ends the lane's decode, and its exit is then the next
 *                segment's guess (the chain is cut there, the lanes behind keep what they found)
 *   rounds       a lane takes its predecessor's latest exit as its entry and decodes again only if that differs (as a
 *                whole) from the entry it last used; until no lane decoded again.  After round r segments 0 .. r are true,
 *                so the fixed point is the serial decode; at most as many rounds as segments
 *   batches      min(256, 32,768 / seg_bytes) segments at a time; lane 0 of a batch enters in the final exit of the batch
 *                before
 *   write        an exclusive prefix sum over the lanes gives each the ordinal of its block in progress, its three DC
 *                predictors and whether the true decode failed before it (then it does nothing).  Each lane decodes its
 *                symbols once more and stores them where spnet_jpeg_entropy does; a block that straddles segments is
 *                written by several lanes at disjoint k.  No block at or beyond MCUs x blocks per MCU is decoded or
 *                written: the lane that finishes the last block applies the trailing-bytes rule (status 5) and the lanes
 *                behind it do nothing.  Data that ends early is status 4.
 * status is NOT cleared: codes are merged with atomicMax, so the call follows spnet_jpeg_entropy (which clears status even
 * with n_intervals 0) on the same status array; spnet_jpeg_pixels follows both.  Reads and writes are bounded as for
 * spnet_jpeg_entropy; every loop is bounded by a count of segments or of the interval's bits. */
int spnet_jpeg_entropy_sync(const unsigned char* blob, long blob_bytes, const int* intervals, int n_intervals,
                            const int* files, int n_files, const uint32_t* tables, int n_sets, int seg_bytes, int16_t* coef,
                            long total_blocks, int* status, void* stream);

/* ---- Ring-count masks (csrc/masks.hip): segmentation masks painted from label rows, and their pixel-level comparison.
 *      spnet_amd/masks.py is the host side and holds the same rule in numpy; DESIGN.md 5g ------------------------------- */
/* THE RULE.  A frame's mask is uint8 [H][W], background 0, painted from its first count[b] rows (count clamped to 0 .. K)
 * of rows double [B][K][6] = (cx, cy, a, b, angle_deg, rings): augmentation.pad_metadata's layout, the one
 * spnet_encode_targets reads.  Rows are painted in order and a later row overwrites an earlier one: the LAST row that
 * contains a pixel gives its value.  Per row, whole numbers:
 *   cxq, cyq, aq, bq = rint(16 v)                          (1/16 pixel, ties to even)
 *   c = rint(2^14 cos(t)), s = rint(2^14 sin(t))           t = (-angle_deg) * (pi / 180) as ONE fp64 product with the
 *                                                          fp64 constant pi / 180; cos / sin in fp64.  The minus sign is
 *                                                          the image-y-down convention of metrics.hip / espi.hip
 *   value = min(255, max(0, trunc(10 * rings)))            the product in fp64
 * Pixel (x, y) has its centre at (16 x + 8, 16 y + 8), the overlay kernel's convention.  With dx = 16 x + 8 - cxq,
 * dy = 16 y + 8 - cyq, u = dx c + dy s, v = -dx s + dy c, the pixel is inside iff
 *   (u bq)^2 + (v aq)^2 <= (aq bq 2^14)^2
 * evaluated exactly (the products fit 64 bits, the squares and their sum 128): no floating point takes part after the
 * quantisation.  A row paints NOTHING if any of its six values is not finite, if aq <= 0 or bq <= 0, or if |cx|, |cy|, a
 * or b is 32,768 or more.  A row whose value is 0 paints zeros: over an earlier row it erases, and alone it cannot be told
 * from background.
 * spnet_ring_masks  H, W 1 .. 16,384, K 1 .. 128; B == 0: nothing to do, success.  Writes every byte of out uint8
 *                   [B][H][W] (16 bytes a store where W % 16 == 0 and out is 16-byte aligned; no alignment is required).
 *                   No value in rows or count causes an access outside the three arrays.
 * spnet_mask_compare  pred, truth uint8 [N][n_pixels] (n_pixels 1 .. 2^31 - 1; 16-byte loads for a frame whose two
 *                   addresses are 16-byte aligned, none required), tol 0 .. 255.  counts int32 [N][5] is WRITTEN, not
 *                   accumulated into: bg_bg (both 0), hit (both above 0 and |p - t| <= tol), miss (both above 0 and
 *                   further apart), pred_only (only pred above 0), true_only.  Integer sums: the result does not depend on
 *                   the grid.  N == 0: success.
 * Both return hipErrorInvalidValue and launch nothing for a NULL pointer, a size or tol outside these limits, rows not
 * 8-byte aligned, count / counts not 4-byte aligned. */
int spnet_ring_masks(const double* rows, const int* count, int B, int K, int H, int W, unsigned char* out, void* stream);
int spnet_mask_compare(const unsigned char* pred, const unsigned char* truth, int N, long n_pixels, int tol, int* counts,
                       void* stream);

/* ---- Mask fitting (csrc/mask_fit.hip, csrc/mask_fit_core.h): the inverse of spnet_ring_masks as far as it has one --
 *      connected components of a ring-count mask and eight integer sums per component, from which the host forms ellipse
 *      rows (spnet_amd/masks.py rows_from_sums, float64).  masks.py holds the same rule in numpy; DESIGN.md 5h ----------- */
/* THE RULE.  A mask is uint8 [H][W], background 0.
 *   Adjacency   two pixels are adjacent iff they are 8-neighbours, both are nonzero, and their values differ by at most
 *               join_tol (0 .. 255).  join_tol 0 joins equal values only (what spnet_ring_masks paints: one value per
 *               row); 255 joins anything nonzero.
 *   Component   a connected component of that graph (well defined although the predicate is not transitive: 10, 14, 18
 *               in a chain are one component at join_tol 4).
 *   Label       1 + (y * W + x) of the component's FIRST pixel in raster order, for every pixel of the component;
 *               background 0.  int32: H * W <= 2^31 - 2, which H, W <= 16,384 guarantees.
 *   Order       the components of a frame in ascending label.
 *   Sums        eight int64 per component: n, sum x, sum y, sum x^2, sum y^2, sum x y, sum v, first -- first = label - 1,
 *               v the pixel's value, x and y its whole-number coordinates.  All fit 64 bits at 16,384 x 16,384.
 * spnet_mask_label    masks uint8 [B][H][W], H, W 1 .. 16,384, join_tol 0 .. 255.  Writes EVERY element of labels int32
 *                     [B][H][W] (which is also the working store: its contents before the call do not matter).  Three
 *                     launches for any mask: no readback, no iteration count that depends on the mask.
 * spnet_mask_moments  labels as spnet_mask_label wrote them for masks (the label form above is what it relies on: a
 *                     component's first pixel, and only that pixel, holds its own index + 1).  C 1 .. 128.  Writes
 *                     n_components int32 [B], the TRUE number of components of each frame, which may exceed C, and sums
 *                     int64 [B][C][8]: the first min(n, C) components of the frame in label order, the remaining slots
 *                     zeroed.  Both are written, not accumulated into.  The sums are integer additions: they do not
 *                     depend on the grid or on the order of arrival.
 * Both: B == 0 succeeds and launches nothing.  hipErrorInvalidValue, and nothing launched, for a NULL pointer, a size,
 * join_tol or C outside these limits, labels / n_components not 4-byte aligned, sums not 8-byte aligned.  No value in
 * masks or labels causes an access outside the arrays (labels are only ever compared, never used as an address, by
 * spnet_mask_moments). */
int spnet_mask_label(const unsigned char* masks, int B, int H, int W, int join_tol, int* labels, void* stream);
int spnet_mask_moments(const unsigned char* masks, const int* labels, int B, int H, int W, int C, int* n_components,
                       long long* sums, void* stream);

/* ---- Antinode tracks (csrc/tracks.hip, csrc/tracks_core.h, csrc/mask_rule.h): which ellipse of a later frame is the same
 *      antinode as one of an earlier frame.  spnet_amd/tracks.py is the host side and holds the same rule in numpy;
 *      DESIGN.md 5i ----------------------------------------------------------------------------------------------------- */
/* THE RULE.  Input is rows double [N][K][6] = (cx, cy, a, b, angle_deg, rings) and count int32 [N], clamped to 0 .. K:
 * the layout spnet_ring_masks reads, frames in time order.
 *   Live      detection (t, k) is live iff k < count[t] and the mask rule's quantisation accepts the row: six finite
 *             values, |cx|, |cy|, a, b below 32,768, aq > 0 and bq > 0.  rings takes no part.
 *   Pixel set S(t, k): the pixels 0 <= x < W, 0 <= y < H that the mask rule calls inside row (t, k) -- the same integers
 *             and the same 128-bit comparison as spnet_ring_masks, every row taken ALONE ("last row wins" plays no part).
 *             area[t][k] = |S(t, k)|, 0 for a dead row.
 *   Overlap   for a gap d in 1 .. G and t + d < N: inter_d[t][i][j] = |S(t, i) ^ S(t + d, j)| (intersection),
 *             union = area_i + area_j - inter.
 *   Eligible  a pair is eligible iff inter > 0 and 1024 * inter >= iou_q * union; iou_q 1 .. 1024 is the IoU threshold in
 *             1/1024.
 *   Better    candidate p beats q iff inter_p * union_q > inter_q * union_p; on equality the LOWER INDEX wins.  No floating
 *             point takes part after the quantisation; every product fits 64 bits.
 *   Linking   passes d = 1, 2, .., G in this order.  In pass d, for every frame pair (t, t + d): F = the live detections of
 *             frame t with no successor yet, P = the live detections of frame t + d with no predecessor yet; i -> j is
 *             linked iff j is the best eligible member of P for i AND i is the best eligible member of F for j.
 *             next[t][i] = (t + d) * K + j, prev[t + d][j] = t * K + i, -1 where there is no link.  Within one pass the
 *             pairs are independent: pair (t, t + d) alone writes next[t] and prev[t + d] and reads only what earlier
 *             passes wrote.  A detection has at most one successor and one predecessor: the links form chains.
 *   Tracks    track[t][k] = 1 + the flat index of its chain's head (the member with prev == -1), age[t][k] = the number
 *             of members before it in the chain; both 0 for a dead row.
 * Limits: H, W 1 .. 16,384; K 1 .. 128; d 1 .. 8; N * K <= 2^31 - 2; N == 0 and N == 1 succeed.
 * spnet_track_area     writes (not accumulates) area int32 [N][K].
 * spnet_track_overlap  the pairs (t, t + d) for t = t0 .. t0 + n_pairs - 1, which must all lie in 0 .. N-1; writes (not
 *                      accumulates) inter int32 [n_pairs][K][K].  Integer sums: the result does not depend on the grid.
 * spnet_track_link     one pass over that range with inter and area as the two calls above wrote them: next and prev int32
 *                      [N][K] (the caller fills them with -1 before the first pass) are read and updated.  A count is used
 *                      only where 0 < inter <= min(area_i, area_j), which every true count satisfies.
 * spnet_track_rank     track and age int32 [N][K] from prev by pointer jumping between two halves of ws
 *                      (spnet_track_rank_ws(N, K) bytes, 4-byte aligned; -1 for sizes outside the limits): 2 +
 *                      ceil(log2(max(N, 2))) launches, a function of N alone; no readback, no workgroup waits for another.
 *                      A prev entry is followed only where it points into an earlier frame; any other value is a head.
 * All write every element of their outputs.  hipErrorInvalidValue, and nothing launched or written, for a NULL pointer, a
 * size, d, iou_q or range outside these limits, rows not 8-byte aligned, any int32 array not 4-byte aligned.  No value in
 * rows, count, inter, area, next or prev causes an access outside the arrays. */
int spnet_track_area(const double* rows, const int* count, int N, int K, int H, int W, int* area, void* stream);
int spnet_track_overlap(const double* rows, const int* count, int N, int K, int H, int W, int t0, int n_pairs, int d,
                        int* inter, void* stream);
int spnet_track_link(const int* inter, const int* area, const double* rows, const int* count, int N, int K, int t0,
                     int n_pairs, int d, int iou_q, int* next, int* prev, void* stream);
long spnet_track_rank_ws(int N, int K);
int spnet_track_rank(const int* prev, const double* rows, const int* count, int N, int K, int* track, int* age, void* ws,
                     void* stream);

/* ---- Tracking score (csrc/track_score.hip, csrc/track_score_core.h, csrc/track_tile.h): predicted tracks against
 *      ground-truth identities.  spnet_amd/tracks.py holds the same rule in numpy; DESIGN.md 5j ------------------------- */
/* THE RULE, in the vocabulary of "Antinode tracks" above.  Truth: rows_t double [N][Kt][6], count_t int32 [N], ident int32
 * [N][Kt]; prediction: rows_p [N][Kp][6], count_p [N], track int32 [N][Kp] as spnet_track_rank wrote it; frame n of one
 * is frame n of the other.
 *   Live, pixel set, Eligible, Better: the track rule's, word for word.
 *   Identity  eff(n, i) = ident[n][i] where truth row (n, i) is live, 1 <= ident <= M and no live row i' < i of the frame
 *             holds the same ident; 0 otherwise.  So an ident of 0, below 0 or above M is no identity, and where an
 *             identity appears twice in a frame the LOWER INDEX counts and the other row has no identity.
 *   Open      a truth row is open iff eff > 0; a predicted row is open iff it is live and track > 0.
 *   Match     inter[i][j] = |S_t(n, i) ^ S_p(n, j)|.  i <-> j are matched iff j is the best eligible open predicted row for
 *             i AND i is the best eligible open truth row for j (the lower index winning a tie on either side).
 *             match[n][i] = j, -1 where there is none; frame_counts[n] = (tp, fn, fp) = (matches, open truth rows - tp,
 *             open predicted rows - tp).
 *   Identity statistics, for g = 1 .. M over the frames in which some row has eff == g, in time order:
 *             present = their number; matched = those with match >= 0; switches = the matched frames whose predicted track
 *             differs from that of g's previous matched frame (the CLEAR-MOT identity switch); fragments = the matched
 *             frames that follow an unmatched present frame after an earlier matched one; first_matched_frame, -1 for none.
 *             ident_stats int32 [M + 1][5] in this order, row 0 zeroed.
 * Limits: those of the track rule for (N, Kt) and (N, Kp), N * Kt * Kp <= 2^31 - 2 for spnet_track_match (the caller takes a
 * movie a range of frames at a time: frames are independent), M 1 .. 65,536, iou_q 1 .. 1024.
 * spnet_track_match  ws: spnet_track_match_ws(N, Kt, Kp) bytes, 4-byte aligned (-1 for sizes outside the limits): inter
 *                    and both areas.  Areas by spnet_track_area, one workgroup per (frame, 64 x 16 tile) for inter, one
 *                    per frame for the mutual-best step; integer sums, so the result does not depend on the grid.
 * spnet_track_ident  match as spnet_track_match wrote it (an entry outside 0 .. Kp-1 counts as unmatched).  ws:
 *                    spnet_track_ident_ws(N, Kt, M) bytes, 4-byte aligned.  One workgroup per frame records eff and the
 *                    first and last frame of every identity; then one lane per identity walks its own frames.
 * Both write every element of their outputs, without a readback, and no workgroup waits for another; N == 0 succeeds
 * (spnet_track_ident then writes the statistics of identities that are never present).  hipErrorInvalidValue, and nothing
 * launched or written, for a NULL pointer, a size, M or iou_q outside these limits, rows not 8-byte aligned, any int32 array
 * or ws not 4-byte aligned.  No value in rows, count, ident, track or match causes an access outside the arrays. */
long spnet_track_match_ws(int N, int Kt, int Kp);
int spnet_track_match(const double* rows_t, const int* count_t, const int* ident, int Kt, const double* rows_p,
                      const int* count_p, const int* track, int Kp, int N, int H, int W, int iou_q, int M, void* ws, int* match,
                      int* frame_counts, void* stream);
long spnet_track_ident_ws(int N, int Kt, int M);
int spnet_track_ident(const double* rows_t, const int* count_t, const int* ident, const int* match, const int* track, int N,
                      int Kt, int Kp, int M, void* ws, int* ident_stats, void* stream);

/* ---- Note envelopes (csrc/audio.hip, csrc/audio_core.h): how loud each pan note is in a strike's sound recording at the
 *      instant of every video frame -- a bank of single-frequency DFTs ("Goertzel bank"), one per note.  spnet_amd/audio.py
 *      is the host side and holds the same rule in numpy; DESIGN.md 5k -------------------------------------------------- */
/* THE RULE.  pcm int16 [S][L]: S recordings, row stride L samples, the first len[s] of row s valid (len clamped to 0 .. L).
 * Frame t = 0 .. T-1 has a window of Wn samples that starts at start(t) = offset + floor(t * hop_num / hop_den) -- hop =
 * hop_num / hop_den samples per frame, an exact rational; offset may be negative.  Note k has the phase step step[k] =
 * round(f_k / rate * 2^32), uint32.  For i = 0 .. Wn-1 and n = start(t) + i:
 *   x  = pcm[s][n] if 0 <= n < len[s], else 0
 *   p  = (uint32)(i * step[k]), wrapping;  q = p >> 20                     (a position in a table of 4096)
 *   re[s][t][k] += x * win[i] * ctab[q]
 *   im[s][t][k] += x * win[i] * ctab[(q + 3072) & 4095]
 * win int16 [Wn] (the host's Hann table, 0 .. 32,767) and ctab int16 [4096] (round(16384 cos(2 pi i / 4096))) are INPUTS:
 * the device, the host twin and the oracle read the same two tables, so no library cosine takes part in what is compared.
 * A term is at most 2^15 * 2^15 * 2^15 = 2^45 in magnitude for any int16 content and there are at most 2^13: the int64 sums
 * cannot overflow.  Integer sums: the result does not depend on the order of summation, on the grid, or on how S or T is
 * split into calls (a later range of frames is the same call with offset advanced to its first start).
 * Limits: S >= 0 (S == 0: nothing to do, success); T 1 .. 2^20; S * T * K <= 2^31 - 1; Wn 64 .. 8192; K 1 .. 64; L 1 ..
 * 2^31 - 1; hop_num, hop_den 1 .. 2^31 - 1; |offset| <= 2^40.  Writes (not accumulates) every element of re and im, int64
 * [S][T][K].  hipErrorInvalidValue, and nothing launched or written, for a NULL pointer, a size outside these limits, or an
 * array not aligned to its element.  No value in pcm, len, win, step or ctab causes an access outside the arrays. */
int spnet_note_envelopes(const int16_t* pcm, const int* len, int S, long L, int T, long offset, long hop_num, long hop_den,
                         const int16_t* win, int Wn, const uint32_t* step, int K, const int16_t* ctab, long long* re,
                         long long* im, void* stream);

#ifdef __cplusplus
}
#endif
#endif
