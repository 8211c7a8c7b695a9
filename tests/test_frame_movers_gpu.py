"""The float frame kernels the augmentation path launches per batch (csrc/augment.hip): spnet_gather_rows,
spnet_gaussian_blur, spnet_warp_affine and spnet_warp_affine_fixed, exactly and behind guards.

gather_rows is a copy: bits in, bits out.  The blur's taps are multiples of 2^-6 (7/64 is the finest) and its pixels here
integers in [-1024, 1024]: row sums are multiples of 2^-6 below 2^10, the result a multiple of 2^-12 below 2^10 -- 22 bits,
every partial sum exact whatever the compiler contracts.  The float warp gets integer pixels and matrices whose entries
are multiples of 1/8: coordinates, weights (multiples of 1/8), products and sums are all exact.  The fixed-point warp is
integer arithmetic.  So every comparison is an equality against a float64 / integer reference; there is no tolerance in
this file.  Outputs are NaN inside, between sentinel bands that must come back untouched (dw_ref.place); float inputs sit
between NaN."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import warp_ref as WR
from tests.helpers import dw_ref as D
from tests.helpers.glue_ref import EW_CAP_ITEMS
from tests.test_dwconv_gpu import Dev, work

FRONT, TAIL, S = D.FRONT, D.TAIL, np.float32(D.SENTINEL)


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel()


def refused(L, table, o):
    """names of the calls that were not refused with hipErrorInvalidValue, or after which the output buffer o was written"""
    wrong = []
    for name, call in table:
        try:
            call()
            wrong.append(name + ": no HipError")
        except L.HipError as e:
            if not str(e).endswith("hipError_t 1"):
                wrong.append(name + ": " + str(e))
        torch.cuda.synchronize()
        if o.check(np.full(o.n, S)) != []:
            wrong.append(name + ": output written")
            break
    return wrong


# ---- spnet_gather_rows -------------------------------------------------------------------------------------------------------
class Rows:
    """rows x Lr floats as a contiguous torch view `skew` floats behind a 16-byte-aligned offset > 0 of a larger device
    buffer: skew 0 = aligned, 1 = 4-byte aligned only.  Source: data between NaN; destination: NaN between the sentinel."""

    def __init__(self, rows, Lr, skew, data=None):
        self.n, self.front = rows * Lr, FRONT + skew
        buf = np.full(self.front + self.n + TAIL, np.nan if data is not None else S, np.float32)
        buf[self.front:self.front + self.n] = np.nan if data is None else np.asarray(data, np.float32).ravel()
        self.buf = torch.from_numpy(buf).cuda()
        self.t = self.buf[self.front:self.front + self.n].view(rows, Lr)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 4 * skew


def float_bits(rs, shape):
    """finite floats of every exponent, negative zero and denormals among them: a copy must move bits, not values"""
    u = rs.randint(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    u[(u & 0x7F800000) == 0x7F800000] &= 0xBFFFFFFF                     # no Inf / NaN: the guards are NaN
    return u.view(np.float32)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def gather_case(L, Lr, idx_dtype, src_skew, dst_skew, n=9, src_rows=5, seed=0):
    rs = np.random.RandomState(1000 * Lr + 10 * src_skew + dst_skew + seed)
    data = float_bits(rs, (src_rows, Lr))
    idx = rs.randint(0, src_rows, size=n)
    idx[:3] = [-1, src_rows, src_rows - 1]                              # clamped to 0 and to the last row; the last row itself
    src, dst = Rows(src_rows, Lr, src_skew, data), Rows(n, Lr, dst_skew)
    L.gather_rows(src.t, torch.tensor(idx, dtype=idx_dtype, device="cuda"), dst.t)
    want = data[np.clip(idx, 0, src_rows - 1)]
    host = dst.buf.cpu().numpy()
    found = D.check_guards(host, dst.n, front=dst.front)
    if not same_bits(host[dst.front:dst.front + dst.n], want):
        found.append("rows differ")
    return found


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("Lr", [1, 7, 120, 124])
def test_gather_rows_every_length(L, Lr, idx_dtype):
    """L = 120 and 124 take the 16-byte kernel (30 and 31 vectors per row), 1 and 7 the 4-byte one"""
    assert gather_case(L, Lr, idx_dtype, 0, 0) == []


@pytest.mark.parametrize("idx_dtype", [torch.int32, torch.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("src_skew,dst_skew", [(1, 1), (1, 0), (0, 1)])
def test_gather_rows_of_a_vector_length_at_4_byte_alignment(L, src_skew, dst_skew, idx_dtype):
    """L = 120 is vectorisable, a pointer one float off a 16-byte boundary is not: the 4-byte kernel must take the call"""
    assert gather_case(L, 120, idx_dtype, src_skew, dst_skew) == []


def test_gather_rows_past_the_grid_cap(L):
    """spnet_ew_grid caps the grid at 8192 workgroups of 256: 2,097,152 items per lap.  n * L = 2^21 + 1 = 699051 * 3 is the
    smallest product that makes the 4-byte kernel's grid-stride loop run a second lap"""
    n, Lr = 699051, 3
    assert n * Lr == EW_CAP_ITEMS + 1 and Lr % 4
    assert gather_case(L, Lr, torch.int32, 0, 0, n=n, src_rows=11) == []


def test_gather_rows_of_nothing_and_rejections(L):
    src = Dev(np.arange(64, dtype=np.float32))
    o = Dev(np.full(64, S, np.float32), S)
    idx = torch.zeros(4, dtype=torch.int64, device="cuda")
    s = st()
    L.spnet_gather_rows(src.ptr, 4, idx.data_ptr(), 8, o.ptr, 0, 16, s)             # n = 0: returns 0, writes nothing
    L.spnet_gather_rows(src.ptr, 4, idx.data_ptr(), 4, o.ptr, 0, 16, s)
    torch.cuda.synchronize()
    assert o.check(np.full(o.n, S)) == []
    g = lambda src=src.ptr, rows=4, index=idx.data_ptr(), ib=8, dst=o.ptr, n=2, Lr=16: L.spnet_gather_rows(src, rows, index, ib, dst, n, Lr, s)
    table = [("L = 0", lambda: g(Lr=0)), ("L = -4", lambda: g(Lr=-4)), ("src_rows = 0", lambda: g(rows=0)), ("idx_bytes = 2", lambda: g(ib=2)),
             ("idx_bytes = 0", lambda: g(ib=0)), ("src NULL", lambda: g(src=None)), ("index NULL", lambda: g(index=None)),
             ("dst NULL", lambda: g(dst=None)), ("n = -1", lambda: g(n=-1)), ("src at 2 bytes", lambda: g(src=src.ptr + 2)),
             ("dst at 2 bytes", lambda: g(dst=o.ptr + 2))]
    assert refused(L, table, o) == []


# ---- spnet_gaussian_blur -----------------------------------------------------------------------------------------------------
TAPS = {0: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
        7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}


def reflect101(i, n):
    """index i of a line of n pixels continued as ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..."""
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def blur_ref(x, ksize):
    """cv2.GaussianBlur(img, (k, k), 0) for k <= 7, separable, BORDER_REFLECT_101, in float64; x [N][H][W]"""
    x = np.asarray(x, np.float64)
    N, H, W = x.shape
    out = x.copy()
    for n in range(N):
        k = TAPS[int(ksize[n])]
        r = len(k) // 2
        cols = [[reflect101(j + d, W) for j in range(W)] for d in range(-r, r + 1)]
        rows = [[reflect101(i + d, H) for i in range(H)] for d in range(-r, r + 1)]
        h = sum(k[t] * x[n][:, cols[t]] for t in range(len(k)))
        out[n] = sum(k[t] * h[rows[t], :] for t in range(len(k)))
    return out


@pytest.mark.parametrize("H,W", [(4, 4), (4, 9), (9, 4), (5, 256), (5, 257), (6, 300)])
def test_gaussian_blur_is_exact(L, H, W):
    """4 = the smallest extent the entry point takes (k = 7 reflects three pixels deep at both ends of a 4-pixel line);
    256 | 257 | 300: one whole x-block, one pixel and 44 pixels into a second one"""
    ks = np.array([0, 3, 5, 7, 7, 0, 3], np.int32)
    N = len(ks)
    x = D.ints((N, H, W), -1024, 1024, 31 * H + W)
    x[4, 0, 0], x[4, -1, -1], x[4, 0, -1], x[4, -1, 0] = 1024, -1024, 1023, -1023          # the extremes, in the corners
    want = blur_ref(x, ks)
    assert np.array_equal(np.rint(want * 4096), want * 4096) and np.abs(want).max() * 4096 < D.LIMIT
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    xd, out = Dev(x), work(N * H * W)
    kd = torch.from_numpy(ks).cuda()
    L.spnet_gaussian_blur(xd.ptr, out.ptr, N, H, W, kd.data_ptr(), st())
    assert out.check(want) == []
    got = out.head(N * H * W).reshape(N, H, W)
    for n in np.flatnonzero(ks == 0):
        assert same_bits(got[n], x[n])                                 # k = 0: the frame passes through, bit for bit
    for n in np.flatnonzero(ks):
        assert not np.array_equal(got[n], x[n])


def test_gaussian_blur_rejections(L):
    H, W, N = 6, 8, 2
    src = Dev(np.zeros(N * H * W, np.float32))
    o = Dev(np.full(N * H * W, S, np.float32), S)
    ks = torch.tensor([3, 7], dtype=torch.int32, device="cuda")
    s = st()
    b = lambda src=src.ptr, dst=o.ptr, N=N, H=H, W=W, k=ks.data_ptr(): L.spnet_gaussian_blur(src, dst, N, H, W, k, s)
    table = [("H = 3", lambda: b(H=3)), ("W = 3", lambda: b(W=3)), ("N = 0", lambda: b(N=0)), ("N = -1", lambda: b(N=-1)),
             ("src == dst", lambda: b(src=o.ptr)), ("src NULL", lambda: b(src=None)), ("dst NULL", lambda: b(dst=None)),
             ("ksize NULL", lambda: b(k=None))]
    assert refused(L, table, o) == []


# ---- spnet_warp_affine -------------------------------------------------------------------------------------------------------
def warp_ref(x, minv):
    """dst(x, y) = bilinear sample of src at (a x + b y + c, d x + e y + f), zero outside, float64; x [N][H][W][C]"""
    x = np.asarray(x, np.float64)
    N, H, W, C = x.shape
    out = np.zeros_like(x)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for n in range(N):
        a, b, c, d, e, f = np.asarray(minv[n], np.float64)
        sx, sy = a * xs + b * ys + c, d * xs + e * ys + f
        x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        wx, wy = (sx - x0)[..., None], (sy - y0)[..., None]

        def at(yy, xx):
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = np.zeros((H, W, C))
            v[ok] = x[n][yy[ok], xx[ok]]
            return v
        top = at(y0, x0) + wx * (at(y0, x0 + 1) - at(y0, x0))
        bot = at(y0 + 1, x0) + wx * (at(y0 + 1, x0 + 1) - at(y0 + 1, x0))
        out[n] = top + wy * (bot - top)
    return out


def warp_case(L, H, W, C, mats, seed):
    """findings of one launch over len(mats) images, one matrix each; proves the case exact first"""
    m = np.asarray(mats, np.float64)
    N = len(m)
    assert np.array_equal(np.rint(m * 8), m * 8) and np.abs(m[:, [0, 1, 3, 4]]).max() <= 4 and np.abs(m).max() <= 1024
    x = D.ints((N, H, W, C), -255, 255, seed)
    want = warp_ref(x, m)
    # coordinates are multiples of 1/8 below 2^13 (16 bits), results multiples of 1/64 below 2^9
    assert np.array_equal(np.rint(want * 64), want * 64) and np.abs(want).max() < 512
    xd, md, out = Dev(x), Dev(m), work(N * H * W * C)
    L.spnet_warp_affine(xd.ptr, out.ptr, N, H, W, C, md.ptr, st())
    return out.check(want), want


@pytest.mark.parametrize("C", [1, 3])
def test_warp_affine_fractional_shifts_three_matrices_per_launch(L, C):
    """half a pixel in x, in y and in both, in either direction: sx = x - 0.5 puts x0 = -1 under destination column 0 (only
    the right neighbour is inside), sx = x + 0.5 puts x0 = W - 1 under the last column (only the left one is); the same
    for the rows"""
    H, W = 7, 10
    sets = [[[1, 0, 0.5, 0, 1, 0], [1, 0, 0, 0, 1, 0.5], [1, 0, 0.5, 0, 1, 0.5]],
            [[1, 0, -0.5, 0, 1, 0], [1, 0, 0, 0, 1, -0.5], [1, 0, -0.5, 0, 1, -0.5]],
            [[1, 0, 0.375, 0, 1, -0.125], [1, 0.125, -0.625, -0.25, 1, 0.875], [-1, 0, W - 1.5, 0, -1, H - 0.5]]]
    for k, mats in enumerate(sets):
        found, _ = warp_case(L, H, W, C, mats, 40 + 3 * k + C)
        assert found == [], k
    # the border pairs: with sx = x - 0.5 column 0 is half its source pixel, with sx = x + 0.5 the last column is
    x = D.ints((3, H, W, C), -255, 255, 40 + C)
    w0 = warp_ref(x, sets[0])
    w1 = warp_ref(x[:1], sets[1][:1])
    assert np.array_equal(w0[0][:, -1], 0.5 * x[0][:, -1]) and np.array_equal(w1[0][:, 0], 0.5 * x[0][:, 0])
    assert np.array_equal(w0[1][-1], 0.5 * x[1][-1])


def test_warp_affine_everything_outside_is_zero(L):
    H, W = 5, 6
    mats = [[1, 0, W + 5, 0, 1, 0], [1, 0, 0, 0, 1, -(H + 5)], [1, 0, W, 0, 1, 0], [1, 0, -1, 0, 1, 0]]
    found, want = warp_case(L, H, W, 3, mats, 50)
    assert found == []
    assert not want[:3].any() and want[3].any()                      # x0 = W: nothing inside; a shift by one pixel: W - 1 columns stay


def test_warp_affine_past_its_grid_cap(L):
    """256 workgroups of 256 at most: 260 x 256 = 66,560 pixels per image make the grid-stride loop lap"""
    H, W = 260, 256
    assert H * W > 256 * 256
    found, _ = warp_case(L, H, W, 1, [[1, 0.125, -3.5, -0.125, 1, 2.25], [1, 0, 0.5, 0, 1, 0.5]], 60)
    assert found == []


# ---- spnet_warp_affine_fixed -------------------------------------------------------------------------------------------------
def fixed_tables(mats, H, W):
    """xrow [N][H][2] = (X0, Y0), xcol [N][W][2] = (adelta, bdelta) from the oracle's own host rounding"""
    xrow, xcol = [], []
    for M in mats:
        X0, Y0, ad, bd = WR.cv2_fixed_point_terms(M, H, W)
        xrow.append(np.stack([X0, Y0], 1))
        xcol.append(np.stack([ad, bd], 1))
    return np.stack(xrow).astype(np.int32), np.stack(xcol).astype(np.int32)


@pytest.mark.parametrize("C", [1, 3])
def test_warp_affine_fixed_three_tables_per_launch(L, C):
    H, W = 24, 40
    mats = [WR.rotation_matrix((W / 2, H / 2), ang) for ang in (3.0, -7.5, 11.0)]
    N = len(mats)
    img = np.random.RandomState(70 + C).randint(0, 256, size=(N, H, W, C)).astype(np.uint8)
    want = np.stack([WR.warp_affine_cv2(img[n], mats[n]) for n in range(N)])
    for n in range(N):                                             # the tables differ: image n under table m is another image
        assert not np.array_equal(want[n], WR.warp_affine_cv2(img[n], mats[(n + 1) % N]))
    xrow, xcol = fixed_tables(mats, H, W)
    xd, out = Dev(img.astype(np.float32)), work(N * H * W * C)
    xr, xc = torch.from_numpy(xrow).cuda(), torch.from_numpy(xcol).cuda()
    L.spnet_warp_affine_fixed(xd.ptr, out.ptr, N, H, W, C, xr.data_ptr(), xc.data_ptr(), st())
    assert out.check(want.astype(np.int64)) == []


def test_warp_affine_fixed_rejections(L):
    H, W = 6, 8
    src = Dev(np.zeros(H * W, np.float32))
    o = Dev(np.full(H * W, S, np.float32), S)
    xrow, xcol = fixed_tables([WR.rotation_matrix((4, 3), 5.0)], H, W)
    xr, xc = torch.from_numpy(xrow).cuda(), torch.from_numpy(xcol).cuda()
    s = st()
    f = lambda src=src.ptr, dst=o.ptr, N=1, r=xr.data_ptr(), c=xc.data_ptr(): L.spnet_warp_affine_fixed(src, dst, N, H, W, 1, r, c, s)
    table = [("N = 0", lambda: f(N=0)), ("N = -1", lambda: f(N=-1)), ("src NULL", lambda: f(src=None)), ("dst NULL", lambda: f(dst=None)),
             ("src == dst", lambda: f(src=o.ptr)), ("xrow NULL", lambda: f(r=None)), ("xcol NULL", lambda: f(c=None))]
    assert refused(L, table, o) == []
