"""The Inception-ResNet-v2 glue (csrc/conv_general.hip) entry by entry against tests/helpers/glue_ref.py, behind guards.

Operands are small integers (a ramp of distinct integers for the gathers), so every sum is exact in fp32 whatever its order:
each case demands the int64 / float64 reference bit for bit -- col, dx, every partial row in the documented layout (pixel r
belongs to partial row (r / 32) % rows) -- and that nothing outside a tensor was written.  Every device tensor sits at a
16-byte-aligned offset > 0 of a larger allocation: inputs between NaN, outputs between (and filled with) the sentinel 7.0,
strided outputs with the sentinel in their gaps.  The assert_exact_* of the helper run on the CPU before anything is
launched.  There is no tolerance in this file: every assertion is an equality or an empty list of findings.

The refusal tests size every buffer for what the launch WOULD read and write if it were not refused, so that a regression
fails an assertion and touches nothing out of bounds.

The tables are read by tests/test_glue_ref_cpu.py as well, which confirms without a GPU that every row is exact, takes the
path it is there for and holds the zeros it is there for."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import gemm_ref as G
from tests.helpers import glue_ref as R
from tests.test_dwconv_gpu import Dev, out, st, tag


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


class Block:
    """a [rows][cols] matrix as the column block [:, col0:col0 + cols] of a wider device tensor [1 + rows + after][ld]
    (gemm_ref.embed): NaN around an input, the sentinel around (and, with mat None, inside) an output"""

    def __init__(self, mat, ld, col0=4, poison=R.NAN, shape=None, after=1):
        if mat is None:
            mat, poison = np.full(shape, R.SENTINEL, np.float32), R.SENTINEL
        mat = np.asarray(mat, np.float32)
        mat = mat.reshape(-1, mat.shape[-1])
        buf, off = G.embed(mat, ld, col0, 1, after, poison)
        self.ld, self.col0, self.shape = ld, col0, mat.shape
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + 4 * off
        assert self.ptr % 16 == 0 and off > 0

    def check(self, want):
        want = np.asarray(want)
        return G.check_output(self.t.cpu().numpy(), want.reshape(self.shape), self.ld, self.col0, 1)

    def untouched(self):
        return self.check(np.full(self.shape, R.SENTINEL))


def outblock(rows, cols, ld, col0=4, after=1):
    return Block(None, ld, col0, shape=(rows, cols), after=after)


# ---- tables ------------------------------------------------------------------------------------------------------------------
# (KH, KW, stride): the six unrolled tap shapes of the adjoint gather, then 1x1, 2x2 and the two stride-2 windows
TAPS = [(3, 3, 1), (1, 7, 1), (7, 1, 1), (1, 3, 1), (3, 1, 1), (5, 5, 1), (1, 1, 1), (2, 2, 1), (3, 3, 2), (5, 5, 2)]
CHANNELS = (4, 36)
PATCH_CAP = (1, 171, 171, 32, 3, 3, 1, 1)           # 171*171*9*8 = 2,105,352 float4 items > 8192*256


def patch_cases(KH, KW, s):
    """(B, H, W, C, KH, KW, stride, same): SAME on images smaller than the window and on even and odd H, W (stride 2 pads
    asymmetrically); VALID with H == KH (one output row), W == KW (one column) and both parities behind them"""
    i = TAPS.index((KH, KW, s))
    rows = []
    for same, hws in ((1, [(2, 3), (3, 2), (6, 5), (5, 8), (1, 1)]), (0, [(KH, KW + 3), (KH + 4, KW), (KH + 3, KW + 4), (KH + 2, KW + 1)])):
        for j, (H, W) in enumerate(hws):
            rows.append((1 + (i + j) % 2, H, W, CHANNELS[(i + j + same) % 2], KH, KW, s, same))
    return rows


# the adjoint gather with BatchNorm sums: every unrolled tap shape under SAME and VALID, and the generic loop
BN_TAPS = [(kh, kw, 1, same) for kh, kw in R.UNROLLED_TAPS for same in (1, 0)] + [(3, 3, 2, 0), (3, 3, 2, 1), (1, 1, 1, 1)]
BN_CHANNELS = (4, 32, 36, 68)                       # 1, 8, 9 and 17 quads: on both sides of one workgroup of 8
BN_MAX_ROWS = 512
COLS_M = (1, 31, 32, 33, 126)


def bn_shapes(KH, KW, s, same):
    """(B, H, W) of the differentiated layer's output: 1, 31, 32, 33 and 126 pixels under SAME (126 > rows*32 for rows 1
    and 2: the pixel loop strides), even and odd H at stride 2; VALID with OH == 1 (the clamped addresses of the unrolled
    loads collapse), OW == 1 and a plane with several output rows"""
    if same:
        return [(1, 1, 1), (1, 1, 31), (2, 4, 4), (1, 3, 11), (2, 7, 9)] + ([(1, 6, 5), (3, 5, 6)] if s == 2 else [])
    return [(1, KH, KW), (2, KH, KW + 4), (1, KH + 3, KW), (2, KH + 4 + s, KW + 3)]


def bn_cases(KH, KW, s, same):
    i = BN_TAPS.index((KH, KW, s, same))
    return [(B, H, W, BN_CHANNELS[(i + j) % 4]) for j, (B, H, W) in enumerate(bn_shapes(KH, KW, s, same))]


def rows_to_run(L_or_none, npix):
    """{1, a middle value, the library's maximum}"""
    full = R.grad_bnsums_rows(npix, BN_MAX_ROWS) if L_or_none is None else int(L_or_none.spnet_grad_bnsums_rows(npix, BN_MAX_ROWS))
    return sorted({1, (full + 1) // 2, full})


def seed_of(*key):
    return int(np.dot(key, [7919 ** k % 10007 for k in range(len(key))])) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def bn_case(B, H, W, C, KH, KW, s, same):
    """operands and references of one adjoint case: dcol, y (zeros of both signs), yp, mean, invstd; g before the mask"""
    OH, OW, _, _ = G.conv_geometry(H, W, KH, KW, s, same)
    seed = seed_of(B, H, W, C, KH, KW, s, same)
    d = dict(dcol=R.ints((B * OH * OW, KH * KW * C), seed), y=R.draw_y((B * H * W, C), seed + 1), yp=R.ints((B * H * W, C), seed + 2))
    d["mean"], d["invstd"] = R.draw_stats(C, seed + 3)
    R.assert_exact_patches(dcol=d["dcol"], taps=KH * KW)
    R.assert_exact_bnsums(R.patch_adjoint(np.abs(d["dcol"]), B, H, W, C, KH, KW, s, same).reshape(-1, C), d["yp"], d["mean"], d["invstd"])
    d["g"] = R.patch_adjoint(d["dcol"], B, H, W, C, KH, KW, s, same).reshape(-1, C)
    return d


@functools.lru_cache(maxsize=None)
def cols_case(M, C):
    seed = seed_of(M, C, 99)
    d = dict(src=R.ints((M, C), seed), y=R.draw_y((M, C), seed + 1), yp=R.ints((M, C), seed + 2))
    d["mean"], d["invstd"] = R.draw_stats(C, seed + 3)
    R.assert_exact_bnsums(np.abs(d["src"]), d["yp"], d["mean"], d["invstd"])
    return d


# (rows, cols, lds, ldd): one float4, a row count of 1, a total that is no multiple of the block, and one case past the grid cap
COPY_CASES = [(1, 4, 8, 12), (5, 36, 40, 44), (1, 260, 260, 264), (37, 260, 264, 268)]
COPY_CAP = (8200, 1028, 1028, 1032)                  # 8200 * 257 = 2,107,400 float4 items > 8192*256
# spnet_copy_cols_batched: (rows, cols, lds) of the jobs, side by side in one destination; max_elems = the first job's
BATCHED_JOBS = [(300, 256, 260), (3, 8, 12), (1, 4, 8)]
RESADD_N = (4, 1028)
RESADD_CAP_N = 4 * (R.EW_CAP_ITEMS + 300)


# ---- the forward gather ----------------------------------------------------------------------------------------------------
def patch_fwd_findings(L, case):
    B, H, W, C, KH, KW, s, same = case
    x = R.ramp((B, H, W, C))
    R.assert_exact_patches(x=x)
    want = R.patch_matrix(x.astype(np.int64), KH, KW, s, same)
    name = "%dx%dx%dx%d " % (B, H, W, C)
    found = []
    xd = Dev(x)
    col = out(want.size)
    L.spnet_patches(xd.ptr, col.ptr, B, H, W, C, KH, KW, s, same, 0, st())
    found += tag(col.check(want), name + "dense")
    col = out(want.size)
    L.spnet_patches_ld(xd.ptr, C, col.ptr, B, H, W, C, KH, KW, s, same, st())
    found += tag(col.check(want), name + "ld == C")
    xb = Block(x, C + 8, 4)
    col = out(want.size)
    L.spnet_patches_ld(xb.ptr, C + 8, col.ptr, B, H, W, C, KH, KW, s, same, st())
    found += tag(col.check(want), name + "ld == C + 8")
    return found


@pytest.mark.parametrize("KH,KW,s", TAPS)
def test_patches_forward(L, KH, KW, s):
    found = []
    for case in patch_cases(KH, KW, s):
        found += tag(patch_fwd_findings(L, case), "same %d" % case[-1])
    assert found == []


def test_patches_forward_past_the_grid_cap(L):
    B, H, W, C, KH, KW, s, same = PATCH_CAP
    x = R.ramp((B, H, W, C))
    R.assert_exact_patches(x=x)
    want = R.patch_matrix(x.astype(np.int64), KH, KW, s, same)
    assert want.size // 4 > R.EW_CAP_ITEMS
    xd, col = Dev(x), out(want.size)
    L.spnet_patches(xd.ptr, col.ptr, B, H, W, C, KH, KW, s, same, 0, st())
    assert col.check(want) == []


@pytest.mark.parametrize("KH,KW,s", TAPS)
def test_patches_backward_is_the_adjoint(L, KH, KW, s):
    found = []
    for B, H, W, C, _, _, _, same in patch_cases(KH, KW, s):
        OH, OW, _, _ = G.conv_geometry(H, W, KH, KW, s, same)
        dcol = R.ints((B * OH * OW, KH * KW * C), seed_of(B, H, W, C, KH, KW, s, same))
        R.assert_exact_patches(dcol=dcol, taps=KH * KW)
        want = R.patch_adjoint(dcol.astype(np.int64), B, H, W, C, KH, KW, s, same)
        dd, dx = Dev(dcol), out(want.size)
        L.spnet_patches(dd.ptr, dx.ptr, B, H, W, C, KH, KW, s, same, 1, st())
        found += tag(dx.check(want), "%dx%dx%dx%d same %d" % (B, H, W, C, same))
    assert found == []


# ---- the gradient producers with BatchNorm sums -----------------------------------------------------------------------------
def bnsums_findings(L, src, M, C, d, g, call_dense, call_ld):
    """both forms, relu 0 | 1, rows {1, middle, maximum}: dx and every partial row bit for bit, gaps untouched"""
    found = []
    yd, ypd, mud, isd = Dev(d["y"]), Dev(d["yp"]), Dev(d["mean"]), Dev(d["invstd"])
    yb, ypb = Block(d["y"], C + 12, 8), Block(d["yp"], C + 16, 4)
    for relu in (0, 1):
        dx_ref = R.relu_mask(g, d["y"], relu)
        for rows in rows_to_run(L, M):
            part_ref = R.bn_rows(dx_ref, d["yp"], d["mean"], d["invstd"], rows)
            name = "relu %d rows %d " % (relu, rows)
            dx, part = out(M * C), out(rows * 2 * C)
            call_dense(dx.ptr, yd.ptr, ypd.ptr, mud.ptr, isd.ptr, relu, part.ptr, rows)
            found += tag(dx.check(dx_ref), name + "dense dx") + tag(part.check(part_ref), name + "dense partial")
            dxb, partb = outblock(M, C, C + 8, 4), outblock(rows * 2, C, C + 20, 8)
            call_ld(dxb.ptr, C + 8, yb.ptr, C + 12, ypb.ptr, C + 16, mud.ptr, isd.ptr, relu, partb.ptr, C + 20, rows)
            found += tag(dxb.check(dx_ref), name + "ld dx") + tag(partb.check(part_ref.reshape(rows * 2, C)), name + "ld partial")
    return found


@pytest.mark.parametrize("KH,KW,s,same", BN_TAPS)
def test_patches_bwd_bnsums(L, KH, KW, s, same):
    found = []
    for B, H, W, C in bn_cases(KH, KW, s, same):
        d = bn_case(B, H, W, C, KH, KW, s, same)
        dd = Dev(d["dcol"])
        geom = (B, H, W, C, KH, KW, s, same)
        dense = lambda dx, y, yp, mu, inv, relu, part, rows: L.spnet_patches_bwd_bnsums(dd.ptr, dx, *geom, y, yp, mu, inv, relu, part, rows, st())
        ld = lambda dx, lddx, y, ldy, yp, ldyp, mu, inv, relu, part, ldp, rows: L.spnet_patches_bwd_bnsums_ld(
            dd.ptr, dx, lddx, *geom, y, ldy, yp, ldyp, mu, inv, relu, part, ldp, rows, st())
        found += tag(bnsums_findings(L, dd, B * H * W, C, d, d["g"], dense, ld), "%dx%dx%dx%d" % (B, H, W, C))
    assert found == []


@pytest.mark.parametrize("C", BN_CHANNELS)
def test_copy_cols_bnsums(L, C):
    found = []
    for M in COLS_M:
        d = cols_case(M, C)
        sb = Block(d["src"], C + 24, 8)
        dense = lambda dx, y, yp, mu, inv, relu, part, rows: L.spnet_copy_cols_bnsums(sb.ptr, C + 24, dx, M, C, y, C, yp, mu, inv, relu, part, rows, st())
        ld = lambda dx, ldd, y, ldy, yp, ldyp, mu, inv, relu, part, ldp, rows: L.spnet_copy_cols_bnsums_ld(
            sb.ptr, C + 24, dx, ldd, M, C, y, ldy, yp, ldyp, mu, inv, relu, part, ldp, rows, st())
        found += tag(bnsums_findings(L, sb, M, C, d, d["src"], dense, ld), "M %d" % M)
    assert found == []


# ---- column copies -----------------------------------------------------------------------------------------------------------
def copy_findings(L, rows, cols, lds, ldd, modes=(0, 1)):
    seed = seed_of(rows, cols, lds, ldd)
    src, dst0 = R.ints((rows, cols), seed), R.ints((rows, cols), seed + 1)
    R.assert_exact_elementwise((src, dst0))
    sd = Block(src, lds, lds - cols) if lds > cols else Dev(src)          # (lds - cols is 4 in the tables: a column offset)
    found = []
    for acc in modes:
        db = Block(dst0, ldd, 4, poison=R.SENTINEL)
        L.spnet_copy_cols(sd.ptr, lds, db.ptr, ldd, rows, cols, acc, st())
        found += tag(db.check(R.copy_cols(dst0, src, acc)), "accumulate %d" % acc)
    return found


@pytest.mark.parametrize("rows,cols,lds,ldd", COPY_CASES)
def test_copy_cols(L, rows, cols, lds, ldd):
    assert copy_findings(L, rows, cols, lds, ldd) == []


def test_copy_cols_past_the_grid_cap(L):
    rows, cols, lds, ldd = COPY_CAP
    assert rows * (cols // 4) > R.EW_CAP_ITEMS
    assert copy_findings(L, rows, cols, lds, ldd, modes=(1,)) == []


def test_copy_cols_batched(L):
    """jobs of unequal size in one launch: 300 x 256 floats (19,200 float4: past the 64 workgroups x 256 threads that
    max_elems buys), 3 x 8 and a single float4; the destinations are neighbouring column blocks of one guarded tensor"""
    srcs = [R.ints((r, c), seed_of(r, c, 5)) for r, c, _ in BATCHED_JOBS]
    blocks = [Block(s, lds, 4) for s, (_, _, lds) in zip(srcs, BATCHED_JOBS)]
    width, rows = sum(c for _, c, _ in BATCHED_JOBS), max(r for r, _, _ in BATCHED_JOBS)
    ldd = width + 8
    dst = outblock(rows, width, ldd, 4)
    jobs, off = [], 0
    for b, (r, c, lds) in zip(blocks, BATCHED_JOBS):
        jobs += [b.ptr, dst.ptr + 4 * off, r, c, lds, ldd]
        off += c
    table = torch.tensor(jobs, dtype=torch.int64, device="cuda")
    max_elems = max(r * c for r, c, _ in BATCHED_JOBS)
    assert max_elems // 4 > R.BATCHED_CAP_ITEMS
    L.spnet_copy_cols_batched(table.data_ptr(), len(BATCHED_JOBS), max_elems, st())
    assert dst.check(R.copy_cols_batched(width, rows, srcs)) == []


# ---- x + scale*up --------------------------------------------------------------------------------------------------------------
def resadd_operands(n, seed, quarter):
    """x integers in +-3; up multiples of 4 (scale 0.25: the sum is an integer, often exactly 0) or integers; a few
    x == up == -0.0"""
    x, up = R.ints((n,), seed), R.ints((n,), seed + 1) * (4 if quarter else 1)
    x[::7], up[::7] = -0.0, -0.0
    return x, up


@pytest.mark.parametrize("n", RESADD_N)
@pytest.mark.parametrize("relu", [0, 1])
def test_resadd(L, n, relu):
    found = []
    for scale, exact in ((0.25, True), (0.17, False)):
        x, up = resadd_operands(n, seed_of(n, relu), exact)
        if exact:
            R.assert_exact_elementwise((x, up), unit=0.25)
        want = R.resadd(x, up, scale, relu, exact)
        assert not exact or R.zero_share(x + 0.25 * up) >= 0.1
        xd, ud, y = Dev(x), Dev(up), out(n)
        L.spnet_resadd(xd.ptr, ud.ptr, y.ptr, n, scale, relu, st())
        found += tag(y.check(want), "scale %g" % scale)
    assert found == []


def test_resadd_past_the_grid_cap(L):
    n = RESADD_CAP_N
    x, up = resadd_operands(n, 77, True)
    R.assert_exact_elementwise((x, up), unit=0.25)
    xd, ud, y = Dev(x), Dev(up), out(n)
    L.spnet_resadd(xd.ptr, ud.ptr, y.ptr, n, 0.25, 1, st())
    assert y.check(R.resadd(x, up, 0.25, 1, exact=True)) == []


@pytest.mark.parametrize("n", RESADD_N)
@pytest.mark.parametrize("relu", [0, 1])
def test_resadd_bwd(L, n, relu):
    """dx and dup = one fp32 product, out of place and in place (dx == g)"""
    found = []
    y, g = R.draw_y((n,), seed_of(n, relu, 3)), R.ints((n,), seed_of(n, relu, 4))
    assert R.zero_share(y) >= 0.1
    for scale in (0.25, 0.17):
        dx_ref, dup_ref = R.resadd_bwd(y, g, scale, relu)
        yd, gd, dx, dup = Dev(y), Dev(g), out(n), out(n)
        L.spnet_resadd_bwd(yd.ptr, gd.ptr, dx.ptr, dup.ptr, n, scale, relu, st())
        found += tag(dx.check(dx_ref), "scale %g dx" % scale) + tag(dup.check(dup_ref), "scale %g dup" % scale)
        gio, dup = Dev(g, R.SENTINEL), out(n)
        L.spnet_resadd_bwd(yd.ptr, gio.ptr, gio.ptr, dup.ptr, n, scale, relu, st())
        found += tag(gio.check(dx_ref), "scale %g dx in place" % scale) + tag(dup.check(dup_ref), "scale %g dup in place" % scale)
    assert found == []


def test_resadd_bwd_past_the_grid_cap(L):
    n = RESADD_CAP_N
    y, g = R.draw_y((n,), 5), R.ints((n,), 6)
    dx_ref, dup_ref = R.resadd_bwd(y, g, 0.25, 1)
    yd, gd, dx, dup = Dev(y), Dev(g), out(n), out(n)
    L.spnet_resadd_bwd(yd.ptr, gd.ptr, dx.ptr, dup.ptr, n, 0.25, 1, st())
    assert dx.check(dx_ref) == [] and dup.check(dup_ref) == []


# ---- refusals ------------------------------------------------------------------------------------------------------------------
# VALID, stride 2, a window one longer than the image: floor((in - k) / 2) + 1 = 0 outputs, where truncating division gives 1
SHORT = [("H == KH - 1", 2, 5), ("W == KW - 1", 5, 2)]


def refusal_table(L, z, o, o2):
    """(name, call).  z: 16384 zeros behind every input, o / o2: 8192 sentinels each behind every output / partial row --
    more than any of these launches would read or write if it were NOT refused (the largest: the 288 x 32 kernel of
    spnet_conv_gemm_f32; the bogus output row of the short-image cases is at most 2 x 288 floats)"""
    s = st()
    t = []
    for name, H, W in SHORT:
        g = (1, H, W, 32, 3, 3, 2, 0)
        t += [("patches fwd, " + name, lambda g=g: L.spnet_patches(z.ptr, o.ptr, *g, 0, s)),
              ("patches bwd, " + name, lambda g=g: L.spnet_patches(z.ptr, o.ptr, *g, 1, s)),
              ("patches_ld, " + name, lambda g=g: L.spnet_patches_ld(z.ptr, 40, o.ptr, *g, s)),
              ("patches_bwd_bnsums, " + name, lambda g=g: L.spnet_patches_bwd_bnsums(z.ptr, o.ptr, *g, z.ptr, z.ptr, z.ptr, z.ptr, 1, o2.ptr, 1, s)),
              ("patches_bwd_bnsums_ld, " + name, lambda g=g: L.spnet_patches_bwd_bnsums_ld(z.ptr, o.ptr, 40, *g, z.ptr, 44, z.ptr, 48, z.ptr, z.ptr, 1, o2.ptr, 36, 1, s)),
              ("conv_gemm_f32, " + name, lambda H=H, W=W: L.spnet_conv_gemm_f32(z.ptr, 32, z.ptr, o.ptr, 32, 1, H, W, 32, 32, 3, 3, 2, 0, None, 0, None, None, s))]
    g = (1, 3, 11, 4, 3, 3, 1, 1)                      # 33 pixels: at most 2 partial rows
    bn = lambda g, rows=1, dcol=z.ptr, dx=o.ptr: L.spnet_patches_bwd_bnsums(dcol, dx, *g, z.ptr, z.ptr, z.ptr, z.ptr, 1, o2.ptr, rows, s)
    bnld = lambda g, rows=1, dcol=z.ptr, dx=o.ptr, ld=(8, 12, 16, 20): L.spnet_patches_bwd_bnsums_ld(
        dcol, dx, ld[0], *g, z.ptr, ld[1], z.ptr, ld[2], z.ptr, z.ptr, 1, o2.ptr, ld[3], rows, s)
    cc = lambda M=33, C=4, lds=8, rows=1, src=z.ptr, dst=o.ptr: L.spnet_copy_cols_bnsums_ld(src, lds, dst, 8, M, C, z.ptr, 12, z.ptr, 16, z.ptr, z.ptr, 1, o2.ptr, 20, rows, s)
    for rows in (0, -1, 3):
        t += [("patches_bwd_bnsums, rows %d" % rows, lambda rows=rows: bn(g, rows)),
              ("patches_bwd_bnsums_ld, rows %d" % rows, lambda rows=rows: bnld(g, rows)),
              ("copy_cols_bnsums_ld, rows %d" % rows, lambda rows=rows: cc(rows=rows)),
              ("copy_cols_bnsums, rows %d" % rows, lambda rows=rows: L.spnet_copy_cols_bnsums(z.ptr, 8, o.ptr, 33, 4, z.ptr, 4, z.ptr, z.ptr, z.ptr, 1, o2.ptr, rows, s))]
    for k, what in ((0, "B"), (1, "H"), (2, "W")):
        for v in (0, -1):
            gz = g[:k] + (v,) + g[k + 1:]
            t += [("patches fwd, %s %d" % (what, v), lambda gz=gz: L.spnet_patches(z.ptr, o.ptr, *gz, 0, s)),
                  ("patches bwd, %s %d" % (what, v), lambda gz=gz: L.spnet_patches(z.ptr, o.ptr, *gz, 1, s)),
                  ("patches_ld, %s %d" % (what, v), lambda gz=gz: L.spnet_patches_ld(z.ptr, 8, o.ptr, *gz, s)),
                  ("patches_bwd_bnsums, %s %d" % (what, v), lambda gz=gz: bn(gz)),
                  ("patches_bwd_bnsums_ld, %s %d" % (what, v), lambda gz=gz: bnld(gz))]
    # NULL tensors, on a shape of C == 0 channels: nothing would be read or written through them if the call went through
    g0 = (1, 3, 11, 0, 3, 3, 1, 1)
    t += [("patches fwd, in NULL", lambda: L.spnet_patches(None, o.ptr, *g0, 0, s)),
          ("patches fwd, out NULL", lambda: L.spnet_patches(z.ptr, None, *g0, 0, s)),
          ("patches bwd, dcol NULL", lambda: L.spnet_patches(None, o.ptr, *g0, 1, s)),
          ("patches bwd, dx NULL", lambda: L.spnet_patches(z.ptr, None, *g0, 1, s)),
          ("patches_ld, in NULL", lambda: L.spnet_patches_ld(None, 8, o.ptr, *g0, s)),
          ("patches_ld, out NULL", lambda: L.spnet_patches_ld(z.ptr, 8, None, *g0, s)),
          ("patches_bwd_bnsums_ld, dcol NULL", lambda: bnld(g0, dcol=None)),
          ("patches_bwd_bnsums_ld, dx NULL", lambda: bnld(g0, dx=None)),
          ("copy_cols_bnsums_ld, src NULL", lambda: cc(C=0, src=None)),
          ("copy_cols_bnsums_ld, dst NULL", lambda: cc(C=0, dst=None))]
    # strides and extents
    t += [("copy_cols, lds < cols", lambda: L.spnet_copy_cols(z.ptr, 4, o.ptr, 8, 5, 8, 0, s)),
          ("copy_cols, ldd < cols", lambda: L.spnet_copy_cols(z.ptr, 8, o.ptr, 4, 5, 8, 1, s)),
          ("copy_cols, cols % 4", lambda: L.spnet_copy_cols(z.ptr, 8, o.ptr, 8, 5, 6, 0, s)),
          ("copy_cols, rows 0", lambda: L.spnet_copy_cols(z.ptr, 8, o.ptr, 8, 0, 8, 0, s)),
          ("copy_cols_bnsums_ld, lds < C", lambda: cc(C=8, lds=4)),
          ("copy_cols_bnsums_ld, M 2^31", lambda: cc(M=2 ** 31)),
          ("copy_cols_bnsums_ld, M 2^32 + 4", lambda: cc(M=2 ** 32 + 4)),
          ("copy_cols_bnsums_ld, M 0", lambda: cc(M=0)),
          ("patches_bwd_bnsums_ld, lddx < C", lambda: bnld(g, ld=(0, 12, 16, 20))),
          ("patches_bwd_bnsums_ld, ldp < C", lambda: bnld(g, ld=(8, 12, 16, 0))),
          ("patches_ld, ldx < C", lambda: L.spnet_patches_ld(z.ptr, 4, o.ptr, 1, 3, 11, 8, 3, 3, 1, 1, s)),
          ("resadd, n % 4", lambda: L.spnet_resadd(z.ptr, z.ptr, o.ptr, 6, 0.25, 1, s)),
          ("resadd_bwd, n % 4", lambda: L.spnet_resadd_bwd(z.ptr, z.ptr, o.ptr, o2.ptr, 6, 0.25, 1, s)),
          ("copy_cols_batched, no jobs", lambda: L.spnet_copy_cols_batched(None, 1, 1024, s))]
    g6, g3 = (1, 3, 11, 6, 3, 3, 1, 1), (1, 3, 11, 4, 3, 3, 3, 1)
    for what, gg in (("C % 4", g6), ("stride 3", g3)):
        t += [("patches fwd, " + what, lambda gg=gg: L.spnet_patches(z.ptr, o.ptr, *gg, 0, s)),
              ("patches bwd, " + what, lambda gg=gg: L.spnet_patches(z.ptr, o.ptr, *gg, 1, s)),
              ("patches_ld, " + what, lambda gg=gg: L.spnet_patches_ld(z.ptr, 8, o.ptr, *gg, s)),
              ("patches_bwd_bnsums, " + what, lambda gg=gg: bn(gg))]
    return t


def run_refusals(L, table, outputs):
    wrong = []
    for name, call in table:
        try:
            call()
            wrong.append(name + ": no HipError")
        except L.HipError as e:
            if not str(e).endswith("hipError_t 1"):
                wrong.append(name + ": " + str(e))
        torch.cuda.synchronize()
        if any(o.check(np.full(o.n, R.SENTINEL)) != [] for o in outputs):
            wrong.append(name + ": output written")
            break
    return wrong


def test_glue_refusals_launch_nothing(L):
    z, o, o2 = Dev(np.zeros(16384, np.float32)), out(8192), out(8192)
    assert run_refusals(L, refusal_table(L, z, o, o2), (o, o2)) == []
