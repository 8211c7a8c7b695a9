"""Exact references for the GEMM family (csrc/gemm.hip, gemm_tile.h, gemm_plan.h, gemm_bf16x3.hip) on STRIDED operands.

numpy only, nothing of the code under test.  The idea: with small integer operands whose absolute product
(|A| @ |B|).max() stays below 2^24, every partial sum of every summation order is an integer that fp32 holds exactly, so
every tile, operand form, main loop, K split and fused epilogue must return the int64 product bit for bit -- no tolerance.
The same holds for the bf16x3 kernels while |a|, |b| <= 256 (such integers are their own high bf16 piece), and, for all
six of their piece products, with the multi-piece integers of x3_operands() at the end of this file.

embed() places a matrix as a column block of a wider, guarded buffer; check_output() compares the block with the int64
result and demands that nothing outside the block was written.  Inputs are poisoned with NaN outside their block: a kernel
that reads a gap element into a stored result turns it into NaN, which check_output reports as a difference."""
import numpy as np

LIMIT = 2 ** 24           # integers of magnitude below this are exact in fp32, in sums of any order
NAN = float("nan")
SENTINEL = 7.0            # finite fill of output gaps and guard rows
FORMS = {"fwd": (0, 1), "dgrad": (0, 0), "wgrad": (1, 1)}      # (a_major, b_major); 0 = K contiguous, 1 = output index contiguous


def int_operands(shape, lo, hi, seed, density=1.0):
    """integer-valued float32 in [lo, hi]; density < 1 zeroes entries at random (long-K cases stay inside the bound)"""
    rs = np.random.RandomState(seed)
    a = rs.randint(lo, hi + 1, size=shape).astype(np.int64)
    if density < 1.0:
        a = a * (rs.random_sample(shape) < density)
    return a.astype(np.float32)


def nonzero_operands(shape, hi, seed):
    """integer-valued float32 in [-hi, hi] without zeros"""
    rs = np.random.RandomState(seed)
    return (rs.randint(1, hi + 1, size=shape) * rs.choice([-1, 1], size=shape)).astype(np.float32)


def as_int(a):
    a = np.asarray(a)
    i = np.rint(a).astype(np.int64)
    if not np.array_equal(i, a):
        raise ValueError("operand is not integer-valued")
    return i


def logical(A, B, form):
    """(A as [M][K], B as [K][N]) in int64 from the arrays as the operand form stores them"""
    A, B = as_int(A), as_int(B)
    if form == "fwd":
        return A, B
    if form == "dgrad":
        return A, B.T
    if form == "wgrad":
        return A.T, B
    raise ValueError(form)


def exact_bound(A, B):
    """(|A| @ |B|).max() in int64, A [M][K], B [K][N]: no partial sum of any order exceeds it"""
    return int((np.abs(as_int(A)) @ np.abs(as_int(B))).max())


def assert_exact(A, B, extra=1):
    """a test-authoring check, run on the CPU before any launch: the case is exact in fp32 (extra: a factor for what an
    epilogue adds on top, e.g. 2 for C0 + A B with |C0| below the bound)"""
    b = exact_bound(A, B) * extra
    if not b < LIMIT:
        raise AssertionError("operands are not exact in fp32: bound %d >= 2^24" % b)
    return b


def col_stats(C, bm):
    """[ceil(M/bm)][2][N] int64: column sums and sums of squares of each group of bm rows"""
    C = np.asarray(C, np.int64)
    rows = -(-C.shape[0] // bm)
    out = np.zeros((rows, 2, C.shape[1]), np.int64)
    for t in range(rows):
        blk = C[t * bm:(t + 1) * bm]
        out[t, 0], out[t, 1] = blk.sum(0), (blk * blk).sum(0)
    return out


def assert_exact_stats(C, bm):
    """the statistics of one row group are exact whatever the order: sum |C| and sum C^2 over its bm rows below 2^24"""
    C = np.asarray(C, np.int64)
    b = max(int(col_stats(np.abs(C), bm)[:, 0].max()), int(col_stats(C, bm)[:, 1].max()))
    if not b < LIMIT:
        raise AssertionError("column statistics are not exact in fp32: bound %d >= 2^24" % b)
    return b


# ---- strided operands ------------------------------------------------------------------------------------------------
def embed(mat, ld, col0=4, rows_before=1, rows_after=1, poison=NAN):
    """(buffer [rows_before + rows + rows_after][ld] float32, offset of the matrix in floats): mat is the column block
    [:, col0:col0 + cols] behind rows_before guard rows; everything else holds `poison`.  col0 % 4 == 0 and ld % 4 == 0
    keep the operand 16-byte aligned although it does not start its allocation."""
    mat = np.asarray(mat, np.float32)
    rows, cols = mat.shape
    if col0 % 4 or ld % 4 or col0 < 0 or col0 + cols > ld:
        raise ValueError("embed: col0 %d, cols %d, ld %d" % (col0, cols, ld))
    buf = np.full((rows_before + rows + rows_after, ld), poison, np.float32)
    buf[rows_before:rows_before + rows, col0:col0 + cols] = mat
    return buf, rows_before * ld + col0


def check_output(buffer, want, ld, col0=4, rows_before=1, sentinel=SENTINEL, limit=8):
    """findings (strings; [] = fine) about an output buffer laid out by embed(): the block must equal `want` (int64 or, for
    the non-finite cases, float64 with NaN == NaN) and every other element must still hold `sentinel`."""
    buf = np.asarray(buffer, np.float32).reshape(-1, ld)
    want = np.asarray(want)
    rows, cols = want.shape
    found = []
    if rows_before + rows > buf.shape[0] or col0 + cols > ld:
        return ["block [%d][%d] does not fit the buffer %s" % (rows, cols, buf.shape)]
    blk = buf[rows_before:rows_before + rows, col0:col0 + cols].astype(np.float64)
    w = want.astype(np.float64)
    bad = ~((blk == w) | (np.isnan(blk) & np.isnan(w)))
    for r, c in np.argwhere(bad)[:limit]:
        found.append("block differs at (%d, %d): got %r want %r" % (r, c, float(blk[r, c]), float(w[r, c])))
    if bad.sum() > limit:
        found.append("... %d block elements differ in all" % int(bad.sum()))
    outside = np.ones(buf.shape, bool)
    outside[rows_before:rows_before + rows, col0:col0 + cols] = False
    hit = outside & ~(buf == np.float32(sentinel))
    for r, c in np.argwhere(hit)[:limit]:
        found.append("gap/guard overwritten at buffer (%d, %d) = block (%d, %d): %r" % (r, c, r - rows_before, c - col0, float(buf[r, c])))
    if hit.sum() > limit:
        found.append("... %d gap/guard elements overwritten in all" % int(hit.sum()))
    return found


def check_dense(got, want, sentinel_tail=0, sentinel=SENTINEL, limit=8):
    """the same for a dense array followed by sentinel_tail sentinel elements (statistics rows, dy_out)"""
    got = np.asarray(got, np.float32).ravel()
    want = np.asarray(want)
    n = want.size
    if got.size != n + sentinel_tail:
        return ["%d elements, expected %d + %d" % (got.size, n, sentinel_tail)]
    found = check_output(got[:n], want.reshape(1, n), n, 0, 0, sentinel, limit)
    hit = np.flatnonzero(got[n:] != np.float32(sentinel))
    if hit.size:
        found.append("gap/guard overwritten at %d elements behind the array, first at +%d" % (hit.size, int(hit[0])))
    return found


# ---- the operations, restated in int64 ---------------------------------------------------------------------------------
def product(A, B, form):
    a, b = logical(A, B, form)
    return a @ b


def bias_add(C, bias):
    return np.asarray(C, np.int64) + as_int(bias)[None, :]


def accumulate(C0, A, B, form):
    return as_int(C0) + product(A, B, form)


def bn_blend(g, yp, a, b, c):
    """dY[m][k] = a[k]*g + b[k]*yp + c[k]"""
    return as_int(a)[None, :] * as_int(g) + as_int(b)[None, :] * as_int(yp) + as_int(c)[None, :]


def bn_relu(x, a, c):
    """relu(a[k]*x + c[k])"""
    return np.maximum(as_int(a)[None, :] * as_int(x) + as_int(c)[None, :], 0)


def conv_geometry(H, W, KH, KW, stride, same):
    """(OH, OW, pad_top, pad_left) of TensorFlow's SAME (the smaller half of an odd padding in front) / VALID"""
    if same:
        OH, OW = -(-H // stride), -(-W // stride)
        pt = max((OH - 1) * stride + KH - H, 0) // 2
        pl = max((OW - 1) * stride + KW - W, 0) // 2
    else:
        OH, OW = (H - KH) // stride + 1, (W - KW) // stride + 1
        pt = pl = 0
    return OH, OW, pt, pl


def patch_matrix(x, KH, KW, stride, same):
    """[B*OH*OW][KH*KW*C] from x [B][H][W][C]: row (b, oh, ow), column (kh, kw, c) holds x[b][oh*s + kh - pt][ow*s + kw - pl][c],
    zero outside the image.  Keeps the dtype of x (int64 for the exact cases, float64 for the cross-check)."""
    x = np.asarray(x)
    B, H, W, C = x.shape
    OH, OW, pt, pl = conv_geometry(H, W, KH, KW, stride, same)
    col = np.zeros((B, OH, OW, KH, KW, C), x.dtype)
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(KH):
                for kw in range(KW):
                    ih, iw = oh * stride + kh - pt, ow * stride + kw - pl
                    if 0 <= ih < H and 0 <= iw < W:
                        col[:, oh, ow, kh, kw, :] = x[:, ih, iw, :]
    return col.reshape(B * OH * OW, KH * KW * C)


# ---- bf16x3: exact operands with non-zero middle and low pieces (csrc/gemm_bf16x3.hip, x3t.h) ----------------------------
# A bf16x3 kernel forms ah*bh + (ah*bm + am*bh) + (ah*bl + am*bm + al*bh) from the pieces h = bf16(x), m = bf16(x - h),
# l = bf16(x - h - m) and drops am*bl, al*bm, al*bl.  x3_operands() draws integer operands in which the dropped terms are
# identically zero while all six kept ones occur, so that the int64 product is what such a kernel must return bit for bit.
X3_TERMS = ((0, 0), (0, 1), (1, 0), (0, 2), (1, 1), (2, 0))       # (piece of A, piece of B) of the six kept products
X3_DROPPED = ((1, 2), (2, 1), (2, 2))
X3_TERM_NAMES = {(0, 0): "ah*bh", (0, 1): "ah*bm", (1, 0): "am*bh", (0, 2): "ah*bl", (1, 1): "am*bm", (2, 0): "al*bh"}


def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even) as float32, by integer arithmetic on the bit pattern; finite input only"""
    x = np.ascontiguousarray(x, np.float32)
    if not np.isfinite(x).all():
        raise ValueError("bf16_rne: non-finite input")
    u = x.view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def bf16x3_pieces(x):
    """[3] + x.shape float64: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m) of a float32 array (both differences are
    exact in fp32); asserts h + m + l == x"""
    x = np.asarray(x)
    x32 = x.astype(np.float32)
    if not np.array_equal(x32.astype(np.float64), x.astype(np.float64)):
        raise ValueError("bf16x3_pieces: the values are not float32")
    h = bf16_rne(x32)
    r = x32 - h
    m = bf16_rne(r)
    l = bf16_rne(r - m)
    p = np.stack([h, m, l]).astype(np.float64)
    assert np.array_equal(p.sum(0), x32.astype(np.float64)), "the three pieces do not sum to x"
    return p


def _hot(ks, count):
    """`count` of the indices ks, evenly spread, the first and the last among them"""
    ks = np.asarray(ks)
    if count <= 0 or ks.size == 0:
        return ks[:0]
    return ks[np.unique(np.rint(np.linspace(0, ks.size - 1, min(count, ks.size))).astype(int))]


def _multi(rs, shape, pieces):
    """integers with exactly `pieces` non-zero bf16 pieces: 3: +-((128 + j) * 2^11 +- (128 + i) * 4 +- 1), about 2^18 (the
    smallest magnitude at which an INTEGER has a low piece that no rounding tie decides); 2: +-((128 + j) * 4 +- 1), about 2^9"""
    sgn = lambda: rs.choice([-1, 1], size=shape)
    if pieces == 3:
        v = sgn() * ((128 + rs.randint(1, 17, size=shape)) * 2048 + sgn() * (128 + rs.randint(0, 128, size=shape)) * 4 + sgn())
    else:
        v = sgn() * ((128 + rs.randint(1, 17, size=shape)) * 4 + sgn())
    return v.astype(np.int64)


def x3_operands(M, N, K, seed, density=0.7, hot=3, pieces=3, pair=True, swap=False, small=2, facing=1.0, a_every=0):
    """(A [M][K], B [K][N]) integer-valued float32.  The contraction index k falls into three classes by k % 3:
         0: A is a `pieces`-piece integer in some places, B a small one      -> ah*bh, am*bh, al*bh
         1: the mirror image                                                 -> ah*bh, ah*bm, ah*bl
         2: A and B are both two-piece integers in some places (pair)        -> ah*bh, ah*bm, am*bh, am*bm
    and everything else is a small integer |v| <= small (its own high piece).  No k pairs (m, l), (l, m) or (l, l): the
    three products a bf16x3 kernel drops are identically zero.  The multi-piece entries sit at `hot` values of k per class
    only -- evenly spread over the class, its first and its last k among them, so that the first and the last K step, and
    every slice of a K split, hold some -- and there in a share `density` of the rows of A / columns of B: a fixed small
    count per row and per column, whatever K, which is what keeps (|A| @ |B|).max() below 2^24 at a long K.
    swap: classes 0 and 1 change roles (B multi-piece where A was).  pieces=2, pair=False: two-piece values times small
    ones only, small enough for exact column statistics.  density and facing may be pairs (for A, for B); facing < 1
    zeroes that share of the SMALL entries that face the other operand's multi-piece ones (a row of B at a hot k of A and
    the reverse): sums over many rows of the product -- column statistics, the sums behind a fused epilogue -- then stay
    below 2^24 as well.  a_every = P > 0 replaces the random choice of A's rows by a regular one, for the operands of a
    kernel that sums over row tiles: rows P apart (another offset for every hot k), so that every tile of P or more rows,
    a ragged last one included, holds its share; B is drawn as before."""
    pair_of = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    (da, db), (fa, fb) = pair_of(density), pair_of(facing)
    rs = np.random.RandomState(seed)
    A = rs.randint(-small, small + 1, size=(M, K)).astype(np.int64)
    B = rs.randint(-small, small + 1, size=(K, N)).astype(np.int64)
    k = np.arange(K)
    ca, cb = (1, 0) if swap else (0, 1)
    rows_a = lambda share, off: (np.arange(M) - off) % a_every == 0 if a_every > 0 else rs.random_sample(M) < share
    for j, kk in enumerate(_hot(k[k % 3 == ca], hot)):
        A[:, kk] = np.where(rows_a(da, 16 * j), _multi(rs, M, pieces), A[:, kk])
        B[kk, :] *= rs.random_sample(N) < fb
    for j, kk in enumerate(_hot(k[k % 3 == cb], hot)):
        B[kk, :] = np.where(rs.random_sample(N) < db, _multi(rs, N, pieces), B[kk, :])
        A[:, kk] *= rows_a(fa, 16 * j + 5)
    if pair:
        for j, kk in enumerate(_hot(k[k % 3 == 2], hot)):
            A[:, kk] = np.where(rows_a(da, 16 * j + 10), _multi(rs, M, 2), A[:, kk])
            B[kk, :] = np.where(rs.random_sample(N) < db, _multi(rs, N, 2), B[kk, :])
    return A.astype(np.float32), B.astype(np.float32)


def x3_term(pa, pb, i, j):
    """the contribution of the product (piece i of A) x (piece j of B), int64 [M][N]"""
    return as_int(pa[i]) @ as_int(pb[j])


def x3_model(pa, pb, scale=None):
    """what a six-term kernel returns from the pieces pa [3][M][K], pb [3][K][N]; scale: {(i, j): factor} (0 knocks a term
    out, 2 doubles it)"""
    out = 0
    for t in X3_TERMS:
        out = out + x3_term(pa, pb, *t) * (1 if scale is None else scale.get(t, 1))
    return out
