"""The fp32 MFMA GEMM family (csrc/gemm.hip, gemm_tile.h, gemm_plan.h) and the strided bf16x3 entries on STRIDED operands,
against exact integer products (tests/helpers/gemm_ref.py).

Every operand is a column block of a wider buffer (gaps of one float4 and of five), behind a guard row and not at the
start of its allocation.  Inputs hold NaN outside their block, outputs the sentinel 7.0.  Operands are small integers
whose absolute product stays below 2^24 (assert_exact, on the CPU, before anything is launched), so every summation order
is exact: each case demands the int64 result bit for bit, nothing written outside the block and no NaN inside it.  There
is no tolerance in this file: every assertion is an equality or an empty list of findings.

The tables (PLAIN, SPLIT, ...) are read by tests/test_gemm_ref_cpu.py as well, which confirms through spnet_gemm_plan that
every row takes the path it is there for (tile, pipelined main loop, K split)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import gemm_ref as R


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


# GEMM_TILES of csrc/gemm_plan.h, restated: id -> (BM, BN)
TILES = {1: (128, 128), 2: (128, 64), 3: (64, 64), 4: (32, 128), 5: (96, 96), 6: (96, 64), 7: (64, 128), 8: (128, 96),
         9: (32, 64), 10: (32, 32)}
AUTO = (64, 64)           # the shapes tile id 0 (the cost model's choice) is called with
K_MAJOR_KS = (4, 36, 1028)      # one short tile | one tile + a float4 tail | 33 K tiles (pipelined main loop), ragged last
OUT_MAJOR_KS = (1, 33, 1025)    # the weight-gradient form: K need not be a multiple of 4
LONG_K = 1000             # from here on operands are in {-1, 0, 1}


def shapes_of(form, tile):
    bm, bn = TILES.get(tile, AUTO)
    if form == "wgrad":       # out-major A: M % 4 == 0
        s = [(bm - 4, bn - 4), (bm + 4, bn + 4)]
        tiny = (4, 4)
    else:
        s = [(bm - 1, bn - 4), (bm + 1, bn + 4)]
        tiny = (1, 4)
    return s + ([tiny] if tile in (0, 4) else [])


def ks_of(form):
    return OUT_MAJOR_KS if form == "wgrad" else K_MAJOR_KS


# (form, tile, M, N, K): unsplit, bias on the forward form
PLAIN = [(f, t, M, N, K) for f in ("fwd", "dgrad", "wgrad") for t in range(11) for (M, N) in shapes_of(f, t) for K in ks_of(f)]
# (form, tile, split, M, N, K): the K split and its slab reduce into a strided C
SPLIT = [(f, t, s) + shapes_of(f, t)[1] + (ks_of(f)[2],) for f in ("fwd", "dgrad", "wgrad") for t in (3, 5, 6, 9) for s in (2, 3)]
ACCUMULATE = [(f, t, M, N, K) for f in ("fwd", "dgrad") for t in (0, 3, 6, 9) for (M, N) in shapes_of(f, t)[:2] for K in (36, 1028)]
COLSTATS = [(f, t, M, N, K) for f in ("fwd", "dgrad") for t in (1, 3, 5, 9, 10) for (M, N) in shapes_of(f, t)[:2] for K in (36, 1028)]
BATCHED = [(t,) + shapes_of("wgrad", t)[1] + (K,) for t in (0, 3, 5, 6) for K in (33, 1025)]
BATCHED_SPLIT = [(t, ks) + shapes_of("wgrad", t)[1] + (1025,) for t in (3, 5, 6) for ks in (2, 5)]
XF_TILES = (0, 3, 5, 8)
BNBLEND = [(t, M, N, K, i % 2) for t in XF_TILES for i, (M, N) in enumerate(shapes_of("fwd", t)[:2]) for K in K_MAJOR_KS]
BNRELU = BNBLEND
CONV_KINDS = [(3, 3, 1, 1), (3, 3, 2, 0), (1, 7, 1, 1), (7, 1, 1, 1), (3, 3, 2, 1)]       # KH, KW, stride, SAME
CONV_IMAGES = [(1, 1, 1), (2, 3, 4), (1, 5, 7)]
CONV = [(t, cout, kind, img) for t in (0, 3, 9, 10) for cout in (4, 36) for kind in CONV_KINDS for img in CONV_IMAGES]
CONV_C = 32
X3_SHAPES = [(1, 4, 4), (95, 92, 36), (97, 100, 260)]
X3_BM = 96
NONFINITE = [(t, 70, 72, 36) for t in (3, 5)]


def stored_shapes(form, M, N, K):
    """the operands as the form stores them: A [M][K] | [K][M], B [K][N] | [N][K]"""
    return ((K, M) if form == "wgrad" else (M, K)), ((N, K) if form == "dgrad" else (K, N))


def draw(form, M, N, K, seed):
    sa, sb = stored_shapes(form, M, N, K)
    v = 1 if K >= LONG_K else 2
    return R.int_operands(sa, -v, v, seed), R.int_operands(sb, -v, v, seed + 1)


class Emb:
    """a matrix as a column block of a wider device buffer (gemm_ref.embed): .ptr = the block's first element"""

    def __init__(self, mat, gap, poison=R.NAN, col0=4, rows_before=1):
        mat = np.asarray(mat, np.float32)
        self.ld, self.col0, self.rb = mat.shape[1] + gap, col0, rows_before
        buf, off = R.embed(mat, self.ld, col0, rows_before, 1, poison)
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + 4 * off
        assert self.ptr % 16 == 0 and off > 0

    def host(self):
        return self.t.cpu().numpy()

    def check(self, want):
        return R.check_output(self.host(), want, self.ld, self.col0, self.rb, R.SENTINEL)


def out_block(M, N, gap, init=None):
    return Emb(np.full((M, N), R.SENTINEL, np.float32) if init is None else init, gap, R.SENTINEL)


def gaps(i):
    """(A, B, C) gaps of case number i: one float4 and an odd number (five) of them, swapped from case to case"""
    return (4, 20, 4) if i % 2 == 0 else (20, 4, 20)


def flat(values, tail=0):
    """a dense device vector, `tail` sentinel floats behind it"""
    v = np.concatenate([np.asarray(values, np.float32).ravel(), np.full(tail, R.SENTINEL, np.float32)])
    return torch.from_numpy(v).cuda()


def nan_ws(n):
    return torch.full((max(n, 4),), R.NAN, device="cuda")


def plan_bm(L, form, M, N, K, tile, **kw):
    """BM of the tile that runs: the table's row, or for tile id 0 the host plan's choice (spnet_gemm_plan, no launch)"""
    if tile in TILES:
        return TILES[tile][0]
    am, bm_ = R.FORMS[form]
    plan = (ctypes.c_int * 10)()
    L.spnet_gemm_plan(am, bm_, M, N, K, 1, 0, 0, kw.get("colstats", 0), 0, 0, kw.get("xf", 0), 0, kw.get("conv", 0), tile,
                      ctypes.addressof(plan))
    return plan[2]


def check_stats(cs, rows, C, bm, N, total_rows):
    """the first `rows` statistics rows equal the int64 sums of their row group; the rest of the buffer is untouched"""
    want = R.col_stats(C, bm)
    if rows != want.shape[0]:
        return ["stat_rows %d, expected %d" % (rows, want.shape[0])]
    return R.check_dense(cs.cpu().numpy(), want, (total_rows - rows) * 2 * N)


# ---- 1. plain, three forms x every tile id ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(PLAIN)), ids=lambda i: "%s-t%d-%dx%dx%d" % PLAIN[i])
def test_plain(L, i):
    form, tile, M, N, K = PLAIN[i]
    A, B = draw(form, M, N, K, i)
    R.assert_exact(*R.logical(A, B, form), extra=2)
    want = R.product(A, B, form)
    bias = None
    if form == "fwd":
        bias = R.int_operands((N,), -2, 2, i + 7)
        want = R.bias_add(want, bias)
        bias = flat(bias)
    ga, gb, gc = gaps(i)
    a, b, c = Emb(A, ga), Emb(B, gb), out_block(M, N, gc)
    am, bmaj = R.FORMS[form]
    L.spnet_gemm_f32(a.ptr, am, a.ld, b.ptr, bmaj, b.ld, c.ptr, c.ld, M, N, K, 1, None, 0,
                     None if bias is None else bias.data_ptr(), tile, st())
    assert c.check(want) == []


# ---- 2. K split ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(SPLIT)), ids=lambda i: "%s-t%d-s%d-%dx%dx%d" % SPLIT[i])
def test_split_k_reduces_into_a_strided_c(L, i):
    form, tile, split, M, N, K = SPLIT[i]
    A, B = draw(form, M, N, K, 100 + i)
    R.assert_exact(*R.logical(A, B, form))
    ga, gb, gc = gaps(i)
    a, b, c = Emb(A, ga), Emb(B, gb), out_block(M, N, gc)
    ws = nan_ws(split * M * N)
    am, bmaj = R.FORMS[form]
    L.spnet_gemm_f32(a.ptr, am, a.ld, b.ptr, bmaj, b.ld, c.ptr, c.ld, M, N, K, split, ws.data_ptr(), split * M * N, None, tile, st())
    assert c.check(R.product(A, B, form)) == []
    assert not bool(torch.isnan(ws[:split * M * N]).any())        # every slab element was written


@pytest.mark.parametrize("nslab", [1, 3, 5, 17])
@pytest.mark.parametrize("gap", [4, 20])
def test_reduce_slabs_into_a_strided_output(L, nslab, gap):
    """nslab 1, 3: one lane per output float4; 5: two; 17: eight (launch_reduce_slabs); 629 float4 = several workgroups"""
    M, N = 37, 68
    slabs = R.int_operands((nslab, M, N), -8, 8, nslab)
    ws = flat(slabs)
    c = out_block(M, N, gap)
    L.spnet_reduce_slabs(ws.data_ptr(), nslab, M, N, c.ptr, c.ld, st())
    assert c.check(R.as_int(slabs).sum(0)) == []


# ---- 3. C += A B -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ACCUMULATE)), ids=lambda i: "%s-t%d-%dx%dx%d" % ACCUMULATE[i])
def test_accumulate(L, i):
    form, tile, M, N, K = ACCUMULATE[i]
    A, B = draw(form, M, N, K, 200 + i)
    C0 = R.int_operands((M, N), -8, 8, 300 + i)
    R.assert_exact(*R.logical(A, B, form), extra=2)        # |C0| <= 8 is below the bound of any of these products
    ga, gb, gc = gaps(i)
    a, b, c = Emb(A, ga), Emb(B, gb), out_block(M, N, gc, init=C0)
    am, bmaj = R.FORMS[form]
    L.spnet_gemm_f32_accumulate(a.ptr, am, a.ld, b.ptr, bmaj, b.ld, c.ptr, c.ld, M, N, K, tile, st())
    assert c.check(R.accumulate(C0, A, B, form)) == []


# ---- 4. column statistics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(COLSTATS)), ids=lambda i: "%s-t%d-%dx%dx%d" % COLSTATS[i])
def test_colstats(L, i):
    form, tile, M, N, K = COLSTATS[i]
    A, B = draw(form, M, N, K, 400 + i)
    R.assert_exact(*R.logical(A, B, form))
    want = R.product(A, B, form)
    bm = TILES[tile][0]
    R.assert_exact_stats(want, bm)
    ga, gb, gc = gaps(i)
    a, b, c = Emb(A, ga), Emb(B, gb), out_block(M, N, gc)
    total = -(-M // 32)                                        # the rows the header asks the caller to provide
    cs = flat([], total * 2 * N)
    rows = ctypes.c_int(-1)
    am, bmaj = R.FORMS[form]
    L.spnet_gemm_f32_colstats(a.ptr, am, a.ld, b.ptr, bmaj, b.ld, c.ptr, c.ld, M, N, K, tile, cs.data_ptr(),
                              ctypes.addressof(rows), st())
    assert c.check(want) == []
    assert check_stats(cs, rows.value, want, bm, N, total) == []


# ---- 5. batched ------------------------------------------------------------------------------------------------------------
def wide(mats, gap, poison):
    """the matrices side by side as column blocks of ONE wide buffer, `gap` floats between them and at both ends, a guard
    row before and after: (device tensor, ld, [col0 of each])"""
    rows, cols = mats[0].shape
    ld = gap + len(mats) * (cols + gap)
    col0s = [gap + j * (cols + gap) for j in range(len(mats))]
    buf, _ = R.embed(mats[0], ld, col0s[0], 1, 1, poison)
    for m, c0 in zip(mats[1:], col0s[1:]):
        buf[1:1 + rows, c0:c0 + cols] = m
    return torch.from_numpy(buf).cuda(), ld, col0s


def check_wide(t, wants, ld, col0s):
    buf = t.cpu().numpy()
    rows, cols = wants[0].shape
    found = []
    for j, want in enumerate(wants):
        alone = buf.copy()
        for k, c0 in enumerate(col0s):
            if k != j:
                alone[1:1 + rows, c0:c0 + cols] = R.SENTINEL        # (the other problems' blocks are checked in their turn)
        found += ["problem %d: %s" % (j, f) for f in R.check_output(alone, want, ld, col0s[j], 1, R.SENTINEL)]
    return found


def batch_operands(M, N, K, seed, nb=3):
    As = [draw("wgrad", M, N, K, seed + 10 * j)[0] for j in range(nb)]
    Bs = [draw("wgrad", M, N, K, seed + 10 * j)[1] for j in range(nb)]
    for A, B in zip(As, Bs):
        R.assert_exact(*R.logical(A, B, "wgrad"))
    return As, Bs, [R.product(A, B, "wgrad") for A, B in zip(As, Bs)]


def offsets_table(ld_a, ca, ld_b, cb, c_offs):
    """{A_b - A_0, B_b - B_0, C_b - C_0} in floats: multiples of 4, none a multiple of its row stride"""
    tab = [v for j in range(len(ca)) for v in (ca[j] - ca[0], cb[j] - cb[0], c_offs[j] - c_offs[0])]
    assert all(v % 4 == 0 for v in tab) and all(tab[3 * j] % ld_a and tab[3 * j + 1] % ld_b for j in range(1, len(ca)))
    return torch.tensor(tab, dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("i", range(len(BATCHED)), ids=lambda i: "t%d-%dx%dx%d" % BATCHED[i])
def test_batched_problems_in_column_blocks(L, i):
    tile, M, N, K = BATCHED[i]
    As, Bs, wants = batch_operands(M, N, K, 500 + i)
    ga, gb, gc = gaps(i)
    at, lda, ca = wide(As, ga, R.NAN)
    bt, ldb, cb = wide(Bs, gb, R.NAN)
    ct, ldc, cc = wide([np.full((M, N), R.SENTINEL, np.float32)] * 3, gc, R.SENTINEL)
    tab = offsets_table(lda, ca, ldb, cb, cc)
    assert ldb != N and ldc != N and all(v % ldc for v in cc[1:])
    ptr = lambda t, ld, c0: t.data_ptr() + 4 * (ld + c0)
    L.spnet_gemm_f32_batched(ptr(at, lda, ca[0]), ptr(bt, ldb, cb[0]), ptr(ct, ldc, cc[0]), tab.data_ptr(), 3, 1, lda, 1, ldb,
                             ldc, M, N, K, tile, st())
    assert check_wide(ct, wants, ldc, cc) == []


@pytest.mark.parametrize("i", range(len(BATCHED_SPLIT)), ids=lambda i: "t%d-s%d-%dx%dx%d" % BATCHED_SPLIT[i])
def test_batched_problems_with_a_k_split(L, i):
    tile, ks, M, N, K = BATCHED_SPLIT[i]
    As, Bs, wants = batch_operands(M, N, K, 600 + i)
    ga, gb, _ = gaps(i)
    at, lda, ca = wide(As, ga, R.NAN)
    bt, ldb, cb = wide(Bs, gb, R.NAN)
    # ldc == N: three dense outputs in one allocation, a guard row before, between and behind them
    ct = torch.full((3 * (M + 1) + 1, N), R.SENTINEL, device="cuda")
    c_offs = [(1 + j * (M + 1)) * N for j in range(3)]
    tab = offsets_table(lda, ca, ldb, cb, c_offs)
    ws = nan_ws(3 * ks * M * N)
    ptr = lambda t, ld, c0: t.data_ptr() + 4 * (ld + c0)
    L.spnet_gemm_f32_batched_splitk(ptr(at, lda, ca[0]), ptr(bt, ldb, cb[0]), ct.data_ptr() + 4 * c_offs[0], tab.data_ptr(), 3,
                                    1, lda, 1, ldb, N, M, N, K, tile, ks, ws.data_ptr(), 3 * ks * M * N, st())
    got = ct.cpu().numpy()
    found = []
    for j in range(3):
        r0 = 1 + j * (M + 1)
        found += ["problem %d: %s" % (j, f) for f in R.check_output(got[r0 - 1:r0 + M + 1], wants[j], N, 0, 1, R.SENTINEL)]
    assert found == []


# ---- 6. / 7. transformed A operands ----------------------------------------------------------------------------------------
def coef_rows(K, cld, rows, seed):
    """[a | b | c], cld floats each, integers in {-2..2}, zero past K"""
    co = np.zeros((3, cld), np.float32)
    co[:, :K] = R.int_operands((3, K), -2, 2, seed)
    for r in range(3):
        if r not in rows:
            co[r] = 0
    return co


@pytest.mark.parametrize("with_dy", [1, 0])
@pytest.mark.parametrize("i", range(len(BNBLEND)), ids=lambda i: "t%d-%dx%dx%d-cld%d" % BNBLEND[i])
def test_bnblend(L, i, with_dy):
    tile, M, N, K, wide_cld = BNBLEND[i]
    cld = -(-K // 32) * 32 + 32 * wide_cld
    g, B = draw("fwd", M, N, K, 700 + i)
    yp = draw("fwd", M, N, K, 750 + i)[0]
    co = coef_rows(K, cld, (0, 1, 2), 770 + i)
    dY = R.bn_blend(g, yp, co[0, :K], co[1, :K], co[2, :K])
    R.assert_exact(dY, R.as_int(B))
    ga, gb, gc = gaps(i)
    gd, ypd, b, c = Emb(g, ga), Emb(yp, ga), Emb(B, gb), out_block(M, N, gc)
    cod = flat(co)
    dy = flat(np.full(M * K, R.SENTINEL), 64) if with_dy else None
    L.spnet_gemm_f32_bnblend(gd.ptr, ypd.ptr, cod.data_ptr(), cld, gd.ld, b.ptr, b.ld, c.ptr, c.ld, M, N, K, tile,
                             dy.data_ptr() if with_dy else None, st())
    assert c.check(dY @ R.as_int(B)) == []
    if with_dy:
        assert R.check_dense(dy.cpu().numpy(), dY, 64) == []


@pytest.mark.parametrize("with_stats", [0, 1])
@pytest.mark.parametrize("i", range(len(BNRELU)), ids=lambda i: "t%d-%dx%dx%d-cld%d" % BNRELU[i])
def test_bnrelu_reads_the_first_columns_of_a_wider_buffer(L, i, with_stats):
    tile, M, N, K, wide_cld = BNRELU[i]
    cld = -(-K // 32) * 32 + 32 * wide_cld
    x, W = draw("fwd", M, N, K, 800 + i)
    co = coef_rows(K, cld, (0, 2), 870 + i)
    act = R.bn_relu(x, co[0, :K], co[2, :K])
    R.assert_exact(act, R.as_int(W))
    want = act @ R.as_int(W)
    _, gb, gc = gaps(i)
    xd = Emb(x, 4, col0=0)                                     # ldx = K + 4: the columns from K on hold NaN (channels not yet written)
    w, y = Emb(W, gb), out_block(M, N, gc)
    cod = flat(co)
    if with_stats:
        bm = plan_bm(L, "fwd", M, N, K, tile, xf=2, colstats=1)
        R.assert_exact_stats(want, bm)
        total = -(-M // 32)
        cs, rows = flat([], total * 2 * N), ctypes.c_int(-1)
        L.spnet_gemm_f32_bnrelu(xd.ptr, xd.ld, cod.data_ptr(), cld, w.ptr, w.ld, y.ptr, y.ld, M, N, K, tile, cs.data_ptr(),
                                ctypes.addressof(rows), st())
        assert check_stats(cs, rows.value, want, bm, N, total) == []
    else:
        L.spnet_gemm_f32_bnrelu(xd.ptr, xd.ld, cod.data_ptr(), cld, w.ptr, w.ld, y.ptr, y.ld, M, N, K, tile, None, None, st())
    assert y.check(want) == []


# ---- 8. the convolution as an implicit GEMM --------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CONV)), ids=lambda i: "t%d-cout%d-k%dx%ds%dsame%d-img%dx%dx%d" % ((CONV[i][0], CONV[i][1]) + CONV[i][2] + CONV[i][3]))
def test_conv_gemm(L, i):
    tile, Cout, (KH, KW, stride, same), (Bn, H, W) = CONV[i]
    C = CONV_C
    x = R.int_operands((Bn, H, W, C), -2, 2, 900 + i)
    Wk = R.int_operands((KH * KW * C, Cout), -2, 2, 950 + i)
    bias = R.int_operands((Cout,), -2, 2, 990 + i)
    OH, OW, _, _ = R.conv_geometry(H, W, KH, KW, stride, same)
    ga, _, gc = gaps(i)
    xd = Emb(x.reshape(Bn * H * W, C), 4)                      # ldx = C + 4
    wd = Emb(Wk, 0, col0=0)                                    # dense by the ABI; behind a guard row all the same
    if OH < 1 or OW < 1:                                       # a VALID window larger than the image: no output, a refusal
        y = out_block(1, Cout, 4)
        with pytest.raises(L.HipError):
            L.spnet_conv_gemm_f32(xd.ptr, xd.ld, wd.ptr, y.ptr, y.ld, Bn, H, W, C, Cout, KH, KW, stride, same, None, tile, None,
                                  None, st())
        torch.cuda.synchronize()
        assert bool((y.t == R.SENTINEL).all())
        return
    M, K = Bn * OH * OW, KH * KW * C
    col = R.patch_matrix(R.as_int(x), KH, KW, stride, same)
    R.assert_exact(col, R.as_int(Wk), extra=2)
    want = col @ R.as_int(Wk)
    # with bias
    y = out_block(M, Cout, 4)                                  # ldy = Cout + 4
    L.spnet_conv_gemm_f32(xd.ptr, xd.ld, wd.ptr, y.ptr, y.ld, Bn, H, W, C, Cout, KH, KW, stride, same, flat(bias).data_ptr(), tile,
                          None, None, st())
    assert y.check(R.bias_add(want, bias)) == []
    # with statistics
    bm = plan_bm(L, "fwd", M, Cout, K, tile, conv=1, colstats=1)
    R.assert_exact_stats(want, bm)
    y2 = out_block(M, Cout, 4)
    total = -(-M // 32)
    cs, rows = flat([], total * 2 * Cout), ctypes.c_int(-1)
    L.spnet_conv_gemm_f32(xd.ptr, xd.ld, wd.ptr, y2.ptr, y2.ld, Bn, H, W, C, Cout, KH, KW, stride, same, None, tile, cs.data_ptr(),
                          ctypes.addressof(rows), st())
    assert y2.check(want) == []
    assert check_stats(cs, rows.value, want, bm, Cout, total) == []


# ---- 9. bf16x3 -------------------------------------------------------------------------------------------------------------
def x3_planes(L, rows, K):
    """a zeroed plane set for a [rows][K] matrix"""
    return torch.zeros(3 * int(L.spnet_bf16x3_plane_elems(rows, K)), dtype=torch.int16, device="cuda")


@pytest.mark.parametrize("vmax", [256, 2])
@pytest.mark.parametrize("M,N,K", X3_SHAPES)
def test_bf16x3_strided(L, M, N, K, vmax):
    """integers up to 256 are their own high bf16 piece, so the six-product kernels are exact as well; vmax 2: small enough
    for the column statistics of a 96-row group to be exact too (asserted), so those entry points are checked there"""
    A, W = R.int_operands((M, K), -vmax, vmax, M + vmax), R.int_operands((K, N), -vmax, vmax, N + vmax)
    R.assert_exact(R.as_int(A), R.as_int(W))
    want = R.as_int(A) @ R.as_int(W)
    stats = vmax == 2
    if stats:
        R.assert_exact_stats(want, X3_BM)
    a = Emb(A, 4)                                              # lda = K + 4, NaN gap
    wd = flat(W)
    bp, ap = x3_planes(L, N, K), x3_planes(L, M, K)
    L.spnet_split_bf16x3(wd.data_ptr(), bp.data_ptr(), K, N, st())
    L.spnet_split_rows_bf16x3(a.ptr, a.ld, ap.data_ptr(), M, K, st())
    total = -(-M // X3_BM)
    for kind in ("fwd", "pp"):
        c = out_block(M, N, 4)                                 # ldc = N + 4
        cs, rows = flat([], (total + 1) * 2 * N), ctypes.c_int(-1)
        if kind == "fwd" and stats:
            L.spnet_gemm_bf16x3_fwd_colstats(a.ptr, a.ld, bp.data_ptr(), c.ptr, c.ld, M, N, K, cs.data_ptr(), ctypes.addressof(rows), st())
        elif kind == "fwd":
            L.spnet_gemm_bf16x3_fwd(a.ptr, a.ld, bp.data_ptr(), c.ptr, c.ld, M, N, K, st())
        else:
            L.spnet_gemm_bf16x3_pp(ap.data_ptr(), bp.data_ptr(), c.ptr, c.ld, M, N, K, cs.data_ptr() if stats else None,
                                   ctypes.addressof(rows) if stats else None, st())
        assert c.check(want) == [], kind
        if stats:
            assert check_stats(cs, rows.value, want, X3_BM, N, total + 1) == [], kind


# ---- 10. one non-finite operand element --------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_stats", [0, 1])
@pytest.mark.parametrize("m0", [5, 69])
@pytest.mark.parametrize("tile,M,N,K", NONFINITE)
def test_a_nan_in_a_poisons_its_row_alone(L, tile, M, N, K, m0, with_stats):
    """m0 = M - 1: rows past M are clamped to the last row when the tile is staged; what they compute must stay out of the
    stored rows and the statistics"""
    A, B = R.nonzero_operands((M, K), 2, tile), R.nonzero_operands((K, N), 2, tile + 1)
    R.assert_exact(R.as_int(A), R.as_int(B))
    clean = R.product(A, B, "fwd")
    bm = TILES[tile][0]
    R.assert_exact_stats(clean, bm)
    want = clean.astype(np.float64)
    want[m0] = R.NAN
    A[m0, 17] = R.NAN
    a, b, c = Emb(A, 4), Emb(B, 20), out_block(M, N, 4)
    if with_stats:
        total = -(-M // 32)
        cs, rows = flat([], total * 2 * N), ctypes.c_int(-1)
        L.spnet_gemm_f32_colstats(a.ptr, 0, a.ld, b.ptr, 1, b.ld, c.ptr, c.ld, M, N, K, tile, cs.data_ptr(), ctypes.addressof(rows), st())
        ws = R.col_stats(clean, bm).astype(np.float64)
        ws[m0 // bm] = R.NAN
        assert rows.value == ws.shape[0]
        assert R.check_dense(cs.cpu().numpy(), ws, (total - rows.value) * 2 * N) == []
    else:
        L.spnet_gemm_f32(a.ptr, 0, a.ld, b.ptr, 1, b.ld, c.ptr, c.ld, M, N, K, 1, None, 0, None, tile, st())
    assert c.check(want) == []


@pytest.mark.parametrize("with_stats", [0, 1])
@pytest.mark.parametrize("n0", [6, 71])
@pytest.mark.parametrize("tile,M,N,K", NONFINITE)
def test_an_inf_in_b_reaches_its_column_alone(L, tile, M, N, K, n0, with_stats):
    A, B = R.nonzero_operands((M, K), 2, tile + 2), R.nonzero_operands((K, N), 2, tile + 3)
    R.assert_exact(R.as_int(A), R.as_int(B))
    want = R.product(A, B, "fwd")
    bm = TILES[tile][0]
    R.assert_exact_stats(want, bm)
    B[17, n0] = np.inf
    a, b, c = Emb(A, 20), Emb(B, 4), out_block(M, N, 20)
    if with_stats:
        total = -(-M // 32)
        cs, rows = flat([], total * 2 * N), ctypes.c_int(-1)
        L.spnet_gemm_f32_colstats(a.ptr, 0, a.ld, b.ptr, 1, b.ld, c.ptr, c.ld, M, N, K, tile, cs.data_ptr(), ctypes.addressof(rows), st())
        ws = R.col_stats(want, bm)
        assert rows.value == ws.shape[0]
        got = cs.cpu().numpy()
        part = got[:ws.size].reshape(ws.shape)
        assert not np.isfinite(part[:, :, n0]).any()
        part[:, :, n0] = 0                                      # (a view: the column is taken out of the exact comparison)
        ws[:, :, n0] = 0
        assert R.check_dense(got, ws, (total - rows.value) * 2 * N) == []
    else:
        L.spnet_gemm_f32(a.ptr, 0, a.ld, b.ptr, 1, b.ld, c.ptr, c.ld, M, N, K, 1, None, 0, None, tile, st())
    buf = c.host()
    col = buf[c.rb:c.rb + M, c.col0 + n0]
    assert not np.isfinite(col).any()
    col[:] = 0
    want[:, n0] = 0
    assert R.check_output(buf, want, c.ld, c.col0, c.rb, R.SENTINEL) == []
