"""The bf16x3 GEMM family (csrc/gemm_bf16x3.hip, x3t.h) against exact integer products in which ALL SIX piece products occur.

tests/test_gemm_gpu.py checks these kernels with integers up to 256, which are their own high bf16 piece: only ah*bh is
non-zero there.  Here the operands come from gemm_ref.x3_operands: integers with non-zero middle and low pieces, laid out
so that the three products a bf16x3 kernel drops (am*bl, al*bm, al*bl) are identically zero.  The int64 product is then what
a six-term kernel must return bit for bit; a dropped, doubled or mis-paired term and a mix-up of the m and l planes change
it (tests/test_gemm_ref_cpu.py shows on the CPU in how many outputs, for every case of this file).  The fused kernels are
compared with the integer references of tests/helpers/dw_ref.py, not with other bf16x3 kernels, and the splits plane by
plane with the definition h = bf16(x), m = bf16(x - h), l = bf16(x - h - m).

Inputs hold NaN outside their block, outputs the sentinel 7.0, plane sets a sentinel word in front and behind.  Every case
is proven exact on the CPU before anything is launched, and every comparison is an equality or an empty list of findings.

The case tables and draws are read by tests/test_gemm_ref_cpu.py as well."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import dw_ref as D
from tests.helpers import gemm_ref as R
from tests.helpers.x3_layout import x3_untile
from tests.test_gemm_gpu import Emb, flat, out_block


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


INVALID = "hipError_t 1$"           # hipErrorInvalidValue, as the checked binding reports it
X3_BM = 96                          # rows of a statistics group
FB_BM = 192                         # pixel rows of a tile of the fused kernels
# one row, one ragged K step | one ragged tile, two K steps | two row tiles and two column tiles, nine K steps (the double-
# buffered main loop in its steady state), ragged last | two full column tiles, a ragged third row tile
X3_SHAPES = [(1, 4, 12), (95, 92, 36), (97, 100, 260), (200, 192, 68)]
GEMM = [(s, swap) for s in range(len(X3_SHAPES)) for swap in (0, 1)]
# seeds: chosen on the CPU, from the reference alone, so that every knock-out of tests/test_gemm_ref_cpu.py shows as widely as
# that file demands (the one-row case has four outputs, the ragged corner tile of a fused case 48 pixels x 4 channels)
GEMM_SEEDS = [1, 0, 10, 11, 20, 21, 30, 31]
WGRAD_M = (31, 96, 1000)            # one ragged step | three full steps | 32 steps, the last of 8 pixels (one row group)
WGRAD_CH = [(100, 260), (96, 96), (36, 8)]
WGRAD = [(M, c, nb) for M in WGRAD_M for c in range(len(WGRAD_CH)) for nb in (1, 3)]
WGRAD_KSPLIT = {31: (1,), 96: (1, 2), 1000: (1, 5)}       # 3 steps in slices of 2 + 1; 32 steps in slices of 7, 7, 7, 7, 4
FUSED_IMAGES = [(5, 6, 8), (3, 12, 16)]                   # 240 rows: the second tile is ragged | three tiles of one image
FUSED_CH = [(100, 96), (36, 64), (256, 260)]
DWFWD = [(im, ch, v) for im in range(2) for ch in range(3) for v in ((0, 0), (1, 1), (1, 0), (0, 1))]     # v = (affine, relu_next)
DWBWD = [(im, ch, v) for im in range(2) for ch in range(3) for v in (0, 1)]       # v 1: affine, ReLU, add, bn_x, BatchNorm sums
DWFWD_SEEDS = [300 + i for i in range(len(DWFWD))]
DWBWD_SEEDS = [400, 701] + [400 + i for i in range(2, len(DWBWD))]


# ---- the draws (numpy only: the CPU self-checks make the same ones) -----------------------------------------------------------
def gemm_case(i):
    s, swap = GEMM[i]
    M, N, K = X3_SHAPES[s]
    return R.x3_operands(M, N, K, GEMM_SEEDS[i], density=1.0 if M == 1 else 0.7, swap=bool(swap))


def stats_case(s):
    """two-piece values times small ones, few enough for the statistics of a 96-row group to be exact"""
    M, N, K = X3_SHAPES[s]
    return R.x3_operands(M, N, K, 100 + s, density=1.0 if M == 1 else 0.15, hot=1, pieces=2, pair=False, small=1,
                         facing=(1.0 if M == 1 else 0.15, 1.0))


def wgrad_case(i, b):
    """z [M][cin], dy [M][cout] of problem b: the classes run along the pixel index"""
    M, c, _ = WGRAD[i]
    cin, cout = WGRAD_CH[c]
    zt, dy = R.x3_operands(cin, cout, M, 200 + 10 * i + b, hot=4)
    return np.ascontiguousarray(zt.T), dy


class DwFwd:
    """spnet_gemm_bf16x3_pp_dwfwd, restated: the int64 GEMM, the affine and the ReLU, the depthwise 3x3 SAME of dw_ref"""

    def __init__(self, i, seed=None):
        im, ch, (self.affine, self.relu) = DWFWD[i]
        seed = DWFWD_SEEDS[i] if seed is None else seed
        self.B, self.H, self.W = FUSED_IMAGES[im]
        self.cin, self.cout = FUSED_CH[ch]
        self.M = self.B * self.H * self.W
        self.z, self.w = R.x3_operands(self.M, self.cout, self.cin, seed, density=0.3, hot=2)       # w [cin][cout]
        rs = np.random.RandomState(seed + 50)
        self.w_next = rs.randint(-1, 2, size=(3, 3, self.cout)).astype(np.float64)
        self.scale = rs.choice([-1.0, 1.0], size=self.cout)
        self.shift = rs.randint(-2, 3, size=self.cout).astype(np.float64)

    def operands(self):
        return self.z, self.w

    def finish(self, y, absolute=False):
        """the epilogue applied to a GEMM result y [M][cout]; absolute: the bound on every partial sum instead"""
        y = np.asarray(y, np.float64)
        if absolute:
            a = np.abs(y) * np.abs(self.scale) + np.abs(self.shift) if self.affine else np.abs(y)
            return D.dw_fwd(a.reshape(self.B, self.H, self.W, self.cout), np.abs(self.w_next))
        a = y * self.scale + self.shift if self.affine else y
        if self.relu:
            a = np.maximum(a, 0.0)
        return D.dw_fwd(a.reshape(self.B, self.H, self.W, self.cout), self.w_next).reshape(self.M, self.cout)

    def assert_exact(self):
        R.assert_exact(R.as_int(self.z), R.as_int(self.w))
        b = float(self.finish(np.abs(R.as_int(self.z)) @ np.abs(R.as_int(self.w)), absolute=True).max())
        assert b < R.LIMIT, "the nine-tap sum is not exact in fp32: bound %g" % b
        return b


class DwBwd:
    """spnet_gemm_bf16x3_pp_dwbwd, restated: int64 dz = dy W^T, then dw_ref's fused backward"""

    def __init__(self, i, seed=None):
        im, ch, self.full = DWBWD[i]
        seed = DWBWD_SEEDS[i] if seed is None else seed
        self.B, self.H, self.W = FUSED_IMAGES[im]
        self.cin, self.cout = FUSED_CH[ch]
        self.M = self.B * self.H * self.W
        # a 192-pixel tile sums |dz| over its pixels (weight gradient, BatchNorm sums): a few multi-piece products per
        # channel and tile are all that fits below 2^24.  So dy is multi-piece in every 96th pixel, the small dy entries
        # that face a multi-piece weight are as few, the depthwise kernel has three taps per channel and xhat is small
        self.dy, wt = R.x3_operands(self.M, self.cin, self.cout, seed, density=(0, 0.5), hot=2, small=1, a_every=96)
        self.w_pw = np.ascontiguousarray(wt.T)                # [cin][cout], as stored
        rs = np.random.RandomState(seed + 50)
        shape = (self.B, self.H, self.W, self.cin)
        ints = lambda sh, v: rs.randint(-v, v + 1, size=sh).astype(np.float64)
        self.x = ints(shape, 1)
        taps = np.argsort(rs.random_sample((9, self.cin)), 0) < 3
        self.w_dw = (taps * rs.choice([-1.0, 1.0], size=(9, self.cin))).reshape(3, 3, self.cin)
        self.add = ints(shape, 2) if self.full else None
        self.bn_x = ints(shape, 1) if self.full else None
        self.scale = rs.choice([-1.0, 1.0], size=self.cin) if self.full else None
        self.shift = ints((self.cin,), 1) if self.full else None
        self.relu_in = self.full
        self.mean = ints((self.cin,), 1)
        self.invstd = np.where(self.mean == 0, rs.choice([1.0, 2.0], size=self.cin), 1.0)       # |xhat| <= 2

    def operands(self):
        return self.dy, self.w_pw.T

    def fused(self, dz):
        dz = np.asarray(dz, np.float64).reshape(self.B, self.H, self.W, self.cin)
        return D.Fused(dz, self.x, self.w_dw, self.relu_in, self.add, self.scale, self.shift, self.mean, self.invstd, self.bn_x)

    def finish(self, dz):
        """(dx [M][cin], the nine weight sums [9][cin], the two BatchNorm sums [2][cin]) over all pixels"""
        f = self.fused(dz)
        whole = [(b, 0, self.H, 0, self.W) for b in range(self.B)]
        return f.dx.reshape(self.M, self.cin), f.dw.reshape(9, self.cin), f.bn_rows(whole).sum(0)

    def assert_exact(self):
        """every partial sum of the case, from absolute values, is below 2^24 (in units of the smallest invstd for the
        BatchNorm sums): the GEMM; the nine taps of dx plus `add`; and per 192-pixel tile -- whole images -- the weight sums
        over |xin| |dz| and the sums over |dx| and |dx| |xhat|"""
        R.assert_exact(R.as_int(self.dy), R.as_int(self.w_pw.T))
        dz = (np.abs(R.as_int(self.dy)) @ np.abs(R.as_int(self.w_pw.T))).astype(np.float64).reshape(self.B, self.H, self.W, self.cin)
        a = np.abs(self.x) * np.abs(self.scale) + np.abs(self.shift) if self.full else np.abs(self.x)
        g = D.dw_bwd_data(dz, np.abs(self.w_dw), self.H, self.W) + (np.abs(self.add) if self.full else 0.0)
        xhat = np.abs(((self.bn_x if self.full else self.x) - self.mean) * self.invstd)
        unit = min(1.0, float(self.invstd.min()))
        assert np.array_equal(np.rint(xhat / unit), xhat / unit)
        per = FB_BM // (self.H * self.W)
        bounds = [a.max(), g.max()]
        for b in range(0, self.B, per):
            t = slice(b, b + per)
            bounds += [D.dw_bwd_weight(a[t], dz[t]).max(), g[t].sum((0, 1, 2)).max() / unit, (g[t] * xhat[t]).sum((0, 1, 2)).max() / unit]
        assert max(bounds) < R.LIMIT, "the case is not exact in fp32: bounds %r" % bounds
        return max(bounds)


# ---- plane sets ---------------------------------------------------------------------------------------------------------------
GUARD_WORD, GUARD_WORDS = 0x4141, 64


class Planes:
    """a plane set for an [R][K] matrix, GUARD_WORDS sentinel words in front and behind (.ptr stays 16-byte aligned); fill
    0: as the header asks for, -1: poisoned, for the kernels that write every element"""

    def __init__(self, L, Rr, K, fill=0):
        self.R, self.K, self.n = Rr, K, 3 * int(L.spnet_bf16x3_plane_elems(Rr, K))
        assert self.n == 3 * D.plane_elems(Rr, K)
        self.t = torch.full((self.n + 2 * GUARD_WORDS,), GUARD_WORD, dtype=torch.int16, device="cuda")
        self.t[GUARD_WORDS:GUARD_WORDS + self.n] = fill
        self.ptr = self.t.data_ptr() + 2 * GUARD_WORDS
        assert self.ptr % 16 == 0

    def body(self):
        return self.t[GUARD_WORDS:GUARD_WORDS + self.n]

    def untouched(self, fill):
        return bool((self.body() == fill).all()) and self.check(None) == []

    def check(self, want, limit=6):
        """findings ([] = fine): each plane equals the piece of `want` (float32 values [R][K]) it is named after, the pad
        rows and columns are zero, the guard words intact"""
        found = []
        t = self.t.cpu().numpy()
        if (t[:GUARD_WORDS] != GUARD_WORD).any() or (t[GUARD_WORDS + self.n:] != GUARD_WORD).any():
            found.append("guard words around the planes overwritten")
        if want is None:
            return found
        pl = x3_untile(self.body(), self.R, self.K).numpy()
        pieces = R.bf16x3_pieces(want)
        for p, name in enumerate(("high", "middle", "low")):
            bad = np.argwhere(pl[p, :self.R, :self.K] != pieces[p])
            for r, k in bad[:limit]:
                found.append("%s plane differs at (%d, %d): got %r want %r (x = %r)" % (name, r, k, pl[p, r, k], pieces[p, r, k], float(want[r, k])))
            if len(bad) > limit:
                found.append("... %d elements of the %s plane differ in all" % (len(bad), name))
        pads = int((pl[:, self.R:] != 0).sum() + (pl[:, :self.R, self.K:] != 0).sum())
        if pads:
            found.append("%d pad elements are not zero" % pads)
        return found


def split_rows(L, mat, gap=4):
    """the planes of a matrix, made by spnet_split_rows_bf16x3 from a strided copy with NaN gaps"""
    a = Emb(mat, gap)
    p = Planes(L, mat.shape[0], mat.shape[1])
    L.spnet_split_rows_bf16x3(a.ptr, a.ld, p.ptr, mat.shape[0], mat.shape[1], st())
    return p


def split_fwd(L, W):
    """the planes [N][K] of a pointwise kernel W [K][N] in the forward form"""
    K, N = W.shape
    p = Planes(L, N, K)
    L.spnet_split_bf16x3(flat(W).data_ptr(), p.ptr, K, N, st())
    return p


def full_mantissa(shape, seed):
    """random float32 with all 24 significand bits in use, both signs, exponents from 2^-20 to 2^20"""
    rs = np.random.RandomState(seed)
    bits = (rs.randint(0, 2, size=shape).astype(np.uint32) << 31) | (rs.randint(107, 148, size=shape).astype(np.uint32) << 23) \
        | rs.randint(0, 1 << 23, size=shape).astype(np.uint32)
    return bits.view(np.float32)


# ---- a. the splits, plane by plane -----------------------------------------------------------------------------------------------
SPLIT_INPUTS = ["x3-%dx%dx%d-swap%d" % (X3_SHAPES[s] + (w,)) for s, w in GEMM] + ["floats"]


def split_matrices(j):
    """(A [M][K], B [K][N]) of split case j"""
    if j < len(GEMM):
        return gemm_case(j)
    return full_mantissa((37, 44), 7), full_mantissa((44, 52), 8)


@pytest.mark.parametrize("j", range(len(SPLIT_INPUTS)), ids=lambda j: SPLIT_INPUTS[j])
def test_split_planes_are_the_three_pieces(L, j):
    A, B = split_matrices(j)
    (M, K), N = A.shape, B.shape[1]
    # rows of a strided matrix, into a poisoned allocation (the split writes the pads as well)
    for gap in (4, 20):
        a, p = Emb(A, gap), Planes(L, M, K, -1)
        L.spnet_split_rows_bf16x3(a.ptr, a.ld, p.ptr, M, K, st())
        assert p.check(A) == [], gap
    # a row stride that is no multiple of 4: the scalar loads
    lda = K + 3
    buf = np.full((M + 2, lda), R.NAN, np.float32)
    buf[1:M + 1, 1:K + 1] = A
    t, p = torch.from_numpy(buf).cuda(), Planes(L, M, K, -1)
    L.spnet_split_rows_bf16x3(t.data_ptr() + 4 * (lda + 1), lda, p.ptr, M, K, st())
    assert p.check(A) == []
    # a pointwise kernel in the forward form: rows = output channels
    w, p = flat(B), Planes(L, N, K, -1)
    L.spnet_split_bf16x3(w.data_ptr(), p.ptr, K, N, st())
    assert p.check(B.T) == []
    # both operand forms in one launch
    pf, pd = Planes(L, N, K, -1), Planes(L, K, N, -1)
    jobs = torch.tensor([w.data_ptr(), pf.ptr, K, N, 1, N, w.data_ptr(), pd.ptr, N, K, N, 1], dtype=torch.int64, device="cuda")
    L.spnet_split_bf16x3_batched(jobs.data_ptr(), 2, max(pf.n, pd.n) // 3, st())
    assert pf.check(B.T) == [] and pd.check(B) == []


# ---- b. fwd, fwd_colstats, pp -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fwd", "pp"])
@pytest.mark.parametrize("i", range(len(GEMM)), ids=lambda i: "%dx%dx%d-swap%d" % (X3_SHAPES[GEMM[i][0]] + (GEMM[i][1],)))
def test_gemm_returns_the_integer_product(L, i, kind):
    A, B = gemm_case(i)
    (M, K), N = A.shape, B.shape[1]
    R.assert_exact(R.as_int(A), R.as_int(B))
    want = R.as_int(A) @ R.as_int(B)
    bp = split_fwd(L, B)
    c = out_block(M, N, 4 if i % 2 else 20)
    if kind == "fwd":
        a = Emb(A, 20 if i % 2 else 4)
        L.spnet_gemm_bf16x3_fwd(a.ptr, a.ld, bp.ptr, c.ptr, c.ld, M, N, K, st())
    else:
        ap = split_rows(L, A)
        L.spnet_gemm_bf16x3_pp(ap.ptr, bp.ptr, c.ptr, c.ld, M, N, K, None, None, st())
    assert c.check(want) == []


@pytest.mark.parametrize("kind", ["fwd", "pp"])
@pytest.mark.parametrize("s", range(len(X3_SHAPES)), ids=lambda s: "%dx%dx%d" % X3_SHAPES[s])
def test_gemm_column_statistics_are_the_integer_sums(L, s, kind):
    A, B = stats_case(s)
    (M, K), N = A.shape, B.shape[1]
    R.assert_exact(R.as_int(A), R.as_int(B))
    want = R.as_int(A) @ R.as_int(B)
    R.assert_exact_stats(want, X3_BM)
    total = -(-M // X3_BM)
    bp = split_fwd(L, B)
    c = out_block(M, N, 4)
    cs, rows = flat([], (total + 1) * 2 * N), ctypes.c_int(-1)
    if kind == "fwd":
        a = Emb(A, 4)
        L.spnet_gemm_bf16x3_fwd_colstats(a.ptr, a.ld, bp.ptr, c.ptr, c.ld, M, N, K, cs.data_ptr(), ctypes.addressof(rows), st())
    else:
        ap = split_rows(L, A)
        L.spnet_gemm_bf16x3_pp(ap.ptr, bp.ptr, c.ptr, c.ld, M, N, K, cs.data_ptr(), ctypes.addressof(rows), st())
    assert c.check(want) == []
    stats = R.col_stats(want, X3_BM)
    assert rows.value == total == stats.shape[0]
    assert R.check_dense(cs.cpu().numpy(), stats, 2 * N) == []


# ---- c. the batched weight gradient -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(WGRAD)), ids=lambda i: "M%d-%dx%d-nb%d" % ((WGRAD[i][0],) + WGRAD_CH[WGRAD[i][1]] + (WGRAD[i][2],)))
def test_wgrad_returns_the_integer_product(L, i):
    M, c, nb = WGRAD[i]
    cin, cout = WGRAD_CH[c]
    Z, G = zip(*[wgrad_case(i, b) for b in range(nb)])
    wants = []
    for z, g in zip(Z, G):
        R.assert_exact(R.as_int(z).T, R.as_int(g))
        wants.append(R.as_int(z).T @ R.as_int(g))
    zp, gp = [split_rows(L, z) for z in Z], [split_rows(L, g, 20) for g in G]
    dense = lambda: Emb(np.full((cin, cout), R.SENTINEL, np.float32), 0, R.SENTINEL, col0=0)       # ld = cout, a guard row before and behind
    for ks in WGRAD_KSPLIT[M]:
        outs = [dense() for _ in range(nb)]
        if ks == 1:
            jobs = torch.tensor([v for b in range(nb) for v in (zp[b].ptr, gp[b].ptr, outs[b].ptr)], dtype=torch.int64, device="cuda")
            L.spnet_gemm_bf16x3_wgrad_batched(jobs.data_ptr(), nb, cin, cout, M, 1, st())
        else:
            steps = -(-M // 32)
            per = -(-steps // ks)
            assert per * (ks - 1) < steps < per * ks                     # a short last slice
            slabs = [flat(np.full(ks * cin * cout, R.NAN), 64) for _ in range(nb)]
            jobs = torch.tensor([v for b in range(nb) for v in (zp[b].ptr, gp[b].ptr, slabs[b].data_ptr())], dtype=torch.int64, device="cuda")
            L.spnet_gemm_bf16x3_wgrad_batched(jobs.data_ptr(), nb, cin, cout, M, ks, st())
            for b in range(nb):
                L.spnet_reduce_slabs(slabs[b].data_ptr(), ks, cin, cout, outs[b].ptr, cout, st())
                s = slabs[b].cpu().numpy()
                assert np.isfinite(s[:-64]).all() and (s[-64:] == R.SENTINEL).all()
                assert np.array_equal(s[:-64].astype(np.float64).reshape(ks, cin, cout).sum(0), wants[b]), (ks, b)
        for b in range(nb):
            assert outs[b].check(wants[b]) == [], (ks, b)


# ---- d. forward GEMM + affine + ReLU + the next depthwise 3x3 -------------------------------------------------------------------
def fused_id(table):
    return lambda i: "%dx%dx%d-%dx%d-%s" % (FUSED_IMAGES[table[i][0]] + FUSED_CH[table[i][1]] + (table[i][2],))


@pytest.mark.parametrize("i", range(len(DWFWD)), ids=fused_id(DWFWD))
def test_dwfwd_planes_are_the_pieces_of_the_integer_result(L, i):
    c = DwFwd(i)
    c.assert_exact()
    want = c.finish(R.as_int(c.z) @ R.as_int(c.w))
    assert L.spnet_gemm_bf16x3_dwbwd_ok(c.H, c.W, c.cout) == 1
    zp, wp = split_rows(L, c.z), split_fwd(L, c.w)
    ss = flat(np.concatenate([c.scale, c.shift])) if c.affine else None
    wn = flat(c.w_next)
    out = Planes(L, c.M, c.cout)
    L.spnet_gemm_bf16x3_pp_dwfwd(zp.ptr, wp.ptr, c.B, c.H, c.W, c.cin, c.cout, ss.data_ptr() if c.affine else None, c.relu,
                                 wn.data_ptr(), out.ptr, st())
    assert out.check(want.astype(np.float32)) == []


# ---- e. data-gradient GEMM + the depthwise backward -------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(DWBWD)), ids=fused_id(DWBWD))
def test_dwbwd_returns_the_integer_gradients(L, i):
    c = DwBwd(i)
    c.assert_exact()
    dx_want, dw_want, bn_want = c.finish(R.as_int(c.dy) @ R.as_int(c.w_pw.T))
    assert L.spnet_gemm_bf16x3_dwbwd_ok(c.H, c.W, c.cin) == 1
    rows = int(L.spnet_gemm_bf16x3_dwbwd_rows(c.M))
    assert rows == -(-c.M // FB_BM)
    dyp, wp = split_rows(L, c.dy), split_rows(L, c.w_pw, 20)
    dense = lambda t: None if t is None else Emb(np.asarray(t, np.float32).reshape(c.M, c.cin), 0, col0=0)       # NaN guard rows
    vec = lambda t: None if t is None else flat(t)
    p = lambda t: None if t is None else (t.ptr if isinstance(t, Emb) else t.data_ptr())
    x, add, bnx = dense(c.x), dense(c.add), dense(c.bn_x)
    wd, sc, sh, mu, isd = vec(c.w_dw), vec(c.scale), vec(c.shift), vec(c.mean), vec(c.invstd)
    dx = Emb(np.full((c.M, c.cin), R.SENTINEL, np.float32), 0, R.SENTINEL, col0=0)
    part, bnp = flat([], rows * 9 * c.cin + 64), flat([], rows * 2 * c.cin + 64)
    L.spnet_gemm_bf16x3_pp_dwbwd(dyp.ptr, wp.ptr, c.B, c.H, c.W, c.cin, c.cout, p(x), p(wd), dx.ptr, c.relu_in, p(add),
                                 part.data_ptr(), p(sc), p(sh), p(mu), p(isd), bnp.data_ptr(), p(bnx), st())
    assert dx.check(dx_want) == []
    for name, buf, k, want in (("weight", part, 9, dw_want), ("BatchNorm", bnp, 2, bn_want)):
        got = buf.cpu().numpy()
        assert (got[-64:] == R.SENTINEL).all() and np.isfinite(got[:-64]).all(), name
        total = got[:-64].astype(np.float64).reshape(rows, k, c.cin).sum(0)
        bad = np.argwhere(total != want)
        assert len(bad) == 0, (name, len(bad), [(int(r), int(ch), total[r, ch], want[r, ch]) for r, ch in bad[:6]])


# ---- f. refusals ------------------------------------------------------------------------------------------------------------------
def test_fwd_and_pp_refusals_leave_c_untouched(L):
    M, N, K = 20, 24, 36
    A, B = R.x3_operands(M, N, K, 5)
    a, bp, ap = Emb(A, 4), split_fwd(L, B), split_rows(L, A)
    c = out_block(M, N, 4)
    cs, rows = flat([], 2 * N), ctypes.c_int(-1)
    fwd = lambda **kw: L.spnet_gemm_bf16x3_fwd(kw.get("a", a.ptr), kw.get("lda", a.ld), kw.get("b", bp.ptr), c.ptr, kw.get("ldc", c.ld), M, N,
                                               kw.get("K", K), st())
    pp = lambda **kw: L.spnet_gemm_bf16x3_pp(kw.get("a", ap.ptr), kw.get("b", bp.ptr), c.ptr, kw.get("ldc", c.ld), M, N, K, kw.get("cs"),
                                             kw.get("rows"), st())
    refused = [lambda: fwd(K=2), lambda: fwd(K=0), lambda: fwd(K=34), lambda: fwd(lda=a.ld + 2), lambda: fwd(a=a.ptr + 4),
               lambda: fwd(b=bp.ptr + 2), lambda: fwd(b=None), lambda: fwd(ldc=N - 4),
               lambda: pp(ldc=N - 4), lambda: pp(a=ap.ptr + 2), lambda: pp(b=bp.ptr + 8), lambda: pp(a=None),
               lambda: pp(cs=cs.data_ptr()),
               lambda: L.spnet_gemm_bf16x3_fwd_colstats(a.ptr, a.ld, bp.ptr, c.ptr, c.ld, M, N, K, None, ctypes.addressof(rows), st()),
               lambda: L.spnet_gemm_bf16x3_fwd_colstats(a.ptr, a.ld, bp.ptr, c.ptr, c.ld, M, N, K, cs.data_ptr(), None, st())]
    for n, call in enumerate(refused):
        with pytest.raises(L.HipError, match=INVALID):
            call()
        torch.cuda.synchronize()
        assert bool((c.t == R.SENTINEL).all()) and bool((cs == R.SENTINEL).all()) and rows.value == -1, n
    fwd()                                                      # (the operands themselves are fine)
    assert c.check(R.as_int(A) @ R.as_int(B)) == []


def test_split_refusals_leave_the_planes_untouched(L):
    A = full_mantissa((20, 36), 3)
    a, p = Emb(A, 4), Planes(L, 20, 36, -1)
    w = flat(A)
    for call in (lambda: L.spnet_split_rows_bf16x3(a.ptr, a.ld, p.ptr + 2, 20, 36, st()),
                 lambda: L.spnet_split_rows_bf16x3(a.ptr, a.ld, p.ptr, 20, 0, st()),
                 lambda: L.spnet_split_rows_bf16x3(a.ptr, a.ld, p.ptr, 0, 36, st()),
                 lambda: L.spnet_split_rows_bf16x3(None, a.ld, p.ptr, 20, 36, st()),
                 lambda: L.spnet_split_bf16x3(w.data_ptr(), p.ptr + 8, 20, 36, st()),
                 lambda: L.spnet_split_bf16x3(w.data_ptr(), None, 20, 36, st()),
                 lambda: L.spnet_split_bf16x3_batched(None, 1, 512, st())):
        with pytest.raises(L.HipError, match=INVALID):
            call()
        torch.cuda.synchronize()
        assert p.untouched(-1)


def test_wgrad_refusals_leave_the_output_untouched(L):
    M, cin, cout = 1000, 36, 8                                # 32 steps
    zt, dy = R.x3_operands(cin, cout, M, 6, hot=4)
    zp, gp = split_rows(L, np.ascontiguousarray(zt.T)), split_rows(L, dy)
    out = flat([], 40 * cin * cout)
    jobs = torch.tensor([zp.ptr, gp.ptr, out.data_ptr()], dtype=torch.int64, device="cuda")
    # more slices than steps | 9 slices of 4 steps: the last would be empty (8 * 4 = 32) | no slices | no problems | no jobs
    for nb, ks, jp in ((1, 33, jobs.data_ptr()), (1, 9, jobs.data_ptr()), (1, 0, jobs.data_ptr()), (0, 1, jobs.data_ptr()), (1, 1, None)):
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_gemm_bf16x3_wgrad_batched(jp, nb, cin, cout, M, ks, st())
        torch.cuda.synchronize()
        assert bool((out == R.SENTINEL).all()), (nb, ks)
    with pytest.raises(L.HipError, match=INVALID):              # one step only
        L.spnet_gemm_bf16x3_wgrad_batched(jobs.data_ptr(), 1, cin, cout, 31, 2, st())
    torch.cuda.synchronize()
    assert bool((out == R.SENTINEL).all())


def test_dwfwd_refusals_leave_the_planes_untouched(L):
    c = DwFwd(4)                                              # 5 x 6 x 8, 36 -> 64
    zp, wp = split_rows(L, c.z), split_fwd(L, c.w)
    wn, ss = flat(c.w_next, 8), flat(np.concatenate([c.scale, c.shift]), 8)
    out = Planes(L, c.M, c.cout)
    assert L.spnet_gemm_bf16x3_dwbwd_ok(24, 32, c.cout) == 0 and L.spnet_gemm_bf16x3_dwbwd_ok(6, 8, 62) == 0
    assert L.spnet_gemm_bf16x3_dwbwd_ok(12, 8, c.cout) == 0 and L.spnet_gemm_bf16x3_dwbwd_ok(8, 6, c.cout) == 0

    def call(**kw):
        L.spnet_gemm_bf16x3_pp_dwfwd(kw.get("z", zp.ptr), kw.get("w", wp.ptr), kw.get("B", c.B), kw.get("H", c.H), kw.get("W", c.W), c.cin,
                                     kw.get("cout", c.cout), kw.get("ss", ss.data_ptr()), 1, kw.get("wn", wn.data_ptr()),
                                     kw.get("out", out.ptr), st())
    for kw in (dict(H=12, W=8), dict(H=8, W=6), dict(cout=62), dict(B=0), dict(z=zp.ptr + 2), dict(w=wp.ptr + 8), dict(out=out.ptr + 2),
               dict(z=None), dict(wn=None), dict(wn=wn.data_ptr() + 4), dict(ss=ss.data_ptr() + 8)):
        with pytest.raises(L.HipError, match=INVALID):
            call(**kw)
        torch.cuda.synchronize()
        assert out.untouched(0), kw


def test_dwbwd_refusals_leave_the_outputs_untouched(L):
    c = DwBwd(3)                                              # 5 x 6 x 8, 36 <- 64, every optional operand
    rows = -(-c.M // FB_BM)
    dyp, wp = split_rows(L, c.dy), split_rows(L, c.w_pw)
    dev = lambda t: flat(np.asarray(t, np.float32), 8)
    x, add, bnx, wd = dev(c.x), dev(c.add), dev(c.bn_x), dev(c.w_dw)
    sc, sh, mu, isd = dev(c.scale), dev(c.shift), dev(c.mean), dev(c.invstd)
    dx, part, bnp = flat([], c.M * c.cin), flat([], rows * 9 * c.cin), flat([], rows * 2 * c.cin)

    def call(**kw):
        g = lambda k, t: kw.get(k, t.data_ptr())
        L.spnet_gemm_bf16x3_pp_dwbwd(kw.get("dy", dyp.ptr), kw.get("w", wp.ptr), kw.get("B", c.B), kw.get("H", c.H), kw.get("W", c.W),
                                     kw.get("cin", c.cin), c.cout, g("x", x), g("wd", wd), g("dx", dx), 1, g("add", add), g("part", part),
                                     sc.data_ptr(), sh.data_ptr(), g("mu", mu), g("isd", isd), bnp.data_ptr(), g("bnx", bnx), st())
    for kw in (dict(H=12, W=8), dict(H=24, W=32), dict(cin=34), dict(B=0), dict(dy=dyp.ptr + 2), dict(w=wp.ptr + 8), dict(dy=None),
               dict(x=None), dict(wd=None), dict(dx=None), dict(part=None), dict(mu=None), dict(isd=None),
               dict(x=x.data_ptr() + 4), dict(dx=dx.data_ptr() + 8), dict(add=add.data_ptr() + 4), dict(bnx=bnx.data_ptr() + 4),
               dict(wd=wd.data_ptr() + 4)):
        with pytest.raises(L.HipError, match=INVALID):
            call(**kw)
        torch.cuda.synchronize()
        assert all(bool((t == R.SENTINEL).all()) for t in (dx, part, bnp)), kw
