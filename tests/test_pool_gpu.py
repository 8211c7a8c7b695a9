"""The pooling layers (csrc/pool.hip) against tests/helpers/dw_ref.py, behind guards, on data full of ties.

Max pools: integers in [-2, 2] with ties planted (dw_ref.draw_pool), a tensor that is constant per channel (every window
a full tie) and the integers again with both BatchNorm affines and the residual on.  "First maximum in row-major window
order over the in-image taps" decides the packed tap ids, and through them the gradient: y, the idx4 words, dx and the
fused BatchNorm sums are demanded bit for bit, with every tensor inside a guarded allocation.  The partial rows of
spnet_maxpool3x3s2_bwd_bnsums are checked ROW BY ROW: pixel r = (b*H + h)*W + w belongs to row (r / 32) % rows.
The 2x2 average pool runs on multiples of 4 (exact).  The only tolerance of the depthwise / pooling test files is the
derived ulp bound of the 3x3 average pool (see test_avgpool3x3s1_same)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import dw_ref as R
from tests.test_dwconv_gpu import Dev, out, st, tag


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


SAME_HW = [(h, w) for h in range(1, 6) for w in range(1, 6)] + [(7, 6)]
SAME_C, SAME_B = (4, 36), (1, 2)
VALID_HW = [(h, w) for h in range(3, 8) for w in range(3, 8)]
VALID_CB = [(4, 1), (36, 2)]
# more than 128 pixels, so that spnet_maxpool3x3s2_bwd_rows answers 3, 6 and (one step of 32 pixels only) 1
BNSUMS_SHAPES = [(2, 13, 11, 36), (3, 16, 15, 4), (1, 5, 4, 36)]
BNSUMS_MAX_ROWS = (1, 3, 128)
AVG2_N, AVG2_C = (1, 2, 3, 5, 8), (1, 3, 4)
AVG3_N, AVG3_C = (1, 2, 3, 5), (4, 36)
IDX_SENTINEL = 0x07070707


def pool_seed(B, H, W, C):
    return 5000 + ((B * 8 + H) * 8 + W) * 64 + C


def pool_data(kind, B, H, W, C, same=True):
    """(x, x_ss, residual, r_ss) of the three data sets ("affine": the same integers, ties planted where the affine on load puts the maximum)"""
    seed = pool_seed(B, H, W, C)
    (OH, _), (OW, _) = (R.same_geom(H, 2), R.same_geom(W, 2)) if same else (R.valid_geom(H), R.valid_geom(W))
    if kind == "const":
        return np.broadcast_to(R.ints((C,), -2, 2, seed + 1), (B, H, W, C)).copy(), None, None, None
    if kind == "ints":
        return R.draw_pool(B, H, W, C, seed, same), None, None, None
    x_ss = R.draw_ss(C, seed + 2)
    return R.draw_pool(B, H, W, C, seed, same, np.sign(x_ss[:C])), x_ss, R.ints((B, OH, OW, C), -2, 2, seed + 3), R.draw_ss(C, seed + 4)


class Words:
    """a guarded uint32 output (the idx4 words)"""

    def __init__(self, n):
        self.n = n
        self.t = torch.from_numpy(np.full(R.FRONT + n + R.TAIL, IDX_SENTINEL, np.int32)).cuda()
        self.ptr = self.t.data_ptr() + 4 * R.FRONT

    def check(self, want):
        got = self.t.cpu().numpy().view(np.uint32)
        found = []
        bad = np.flatnonzero(got[R.FRONT:R.FRONT + self.n] != want)
        if bad.size:
            found.append("%d idx4 words differ, first at %d: got %#x want %#x" % (bad.size, bad[0], got[R.FRONT + bad[0]], want[bad[0]]))
        if (got[:R.FRONT] != IDX_SENTINEL).any() or (got[R.FRONT + self.n:] != IDX_SENTINEL).any():
            found.append("guard words overwritten")
        return found


def maxpool_findings(L, kind, B, H, W, C, same=True):
    x, x_ss, res, r_ss = pool_data(kind, B, H, W, C, same)
    (OH, _), (OW, _) = (R.same_geom(H, 2), R.same_geom(W, 2)) if same else (R.valid_geom(H), R.valid_geom(W))
    dy = R.ints((B, OH, OW, C), -2, 2, pool_seed(B, H, W, C) + 5)
    R.assert_exact_pool(x, dy, res, x_ss, r_ss)
    y_ref, taps = R.maxpool_fwd(x, same, res, x_ss, r_ss)
    dx_ref = R.maxpool_bwd(dy, taps, H, W, same)
    xd, dyd = Dev(x), Dev(dy)
    ssd, resd, rsd = (None if t is None else Dev(t) for t in (x_ss, res, r_ss))
    p = lambda t: None if t is None else t.ptr
    name = "%s B%d C%d " % (kind, B, C)
    found = []
    y, idx, dx = out(y_ref.size), Words(y_ref.size // 4), out(x.size)
    if same:
        L.spnet_maxpool3x3s2_add_fwd(xd.ptr, p(resd), y.ptr, idx.ptr, B, H, W, C, p(ssd), p(rsd), st())
        L.spnet_maxpool3x3s2_bwd(dyd.ptr, idx.ptr, dx.ptr, B, H, W, C, st())
        y2 = out(y_ref.size)                                  # idx4 == NULL: y alone
        L.spnet_maxpool3x3s2_add_fwd(xd.ptr, p(resd), y2.ptr, None, B, H, W, C, p(ssd), p(rsd), st())
        found += tag(y2.check(y_ref), name + "y without idx4")
    else:
        L.spnet_maxpool3x3s2_valid_fwd(xd.ptr, y.ptr, idx.ptr, B, H, W, C, st())
        L.spnet_maxpool3x3s2_valid_bwd(dyd.ptr, idx.ptr, dx.ptr, B, H, W, C, st())
    found += tag(y.check(y_ref), name + "y") + tag(idx.check(R.pack_taps(taps)), name + "idx4") + tag(dx.check(dx_ref), name + "dx")
    return found


@pytest.mark.parametrize("H,W", SAME_HW)
def test_maxpool_same(L, H, W):
    """kind "ints" runs with residual == NULL, kind "affine" with the residual and both affines"""
    found = []
    for C in SAME_C:
        for B in SAME_B:
            for kind in ("ints", "const", "affine"):
                found += maxpool_findings(L, kind, B, H, W, C)
    assert found == []


@pytest.mark.parametrize("H,W", VALID_HW)
def test_maxpool_valid(L, H, W):
    found = []
    for C, B in VALID_CB:
        for kind in ("ints", "const"):
            found += maxpool_findings(L, kind, B, H, W, C, same=False)
    assert found == []


@pytest.mark.parametrize("B,H,W,C", BNSUMS_SHAPES)
def test_maxpool_bwd_bnsums(L, B, H, W, C):
    seed = pool_seed(B, H, W, C)
    x = R.draw_pool(B, H, W, C, seed)
    (OH, _), (OW, _) = R.same_geom(H, 2), R.same_geom(W, 2)
    dy, yp, mean = R.ints((B, OH, OW, C), -2, 2, seed + 5), R.ints((B, H, W, C), -2, 2, seed + 6), R.ints((C,), -2, 2, seed + 7)
    invstd = np.random.RandomState(seed + 8).choice([0.5, 1.0, 2.0], size=C)
    R.assert_exact_pool(x, dy, yp=yp, mean=mean, invstd=invstd)
    _, taps = R.maxpool_fwd(x)
    dx_ref = R.maxpool_bwd(dy, taps, H, W)
    dyd, ypd, mud, isd = Dev(dy), Dev(yp), Dev(mean), Dev(invstd)
    idx = torch.from_numpy(R.pack_taps(taps).view(np.int32)).cuda()
    full = int(L.spnet_maxpool3x3s2_bwd_rows(B, H, W, C, 128))
    rows_to_run = sorted({int(L.spnet_maxpool3x3s2_bwd_rows(B, H, W, C, m)) for m in BNSUMS_MAX_ROWS} | ({full - 1} if full > 1 else set()))
    assert all(int(L.spnet_maxpool3x3s2_bwd_rows(B, H, W, C, m)) == R.pool_bwd_rows(B, H, W, m) <= m for m in BNSUMS_MAX_ROWS)
    found = []
    for rows in rows_to_run:
        dx, part = out(x.size), out(rows * 2 * C)
        L.spnet_maxpool3x3s2_bwd_bnsums(dyd.ptr, idx.data_ptr(), dx.ptr, B, H, W, C, ypd.ptr, mud.ptr, isd.ptr, part.ptr, rows, st())
        found += tag(dx.check(dx_ref), "rows %d dx" % rows)
        found += tag(part.check(R.maxpool_bn_rows(dx_ref, yp, mean, invstd, rows)), "rows %d partial" % rows)
    assert found == []
    dx, part = out(x.size), out((full + 1) * 2 * C)
    for rows in (0, -1, full + 1):
        with pytest.raises(L.HipError, match="hipError_t 1$"):
            L.spnet_maxpool3x3s2_bwd_bnsums(dyd.ptr, idx.data_ptr(), dx.ptr, B, H, W, C, ypd.ptr, mud.ptr, isd.ptr, part.ptr, rows, st())
    torch.cuda.synchronize()
    assert dx.check(np.full(dx.n, R.SENTINEL)) == [] and part.check(np.full(part.n, R.SENTINEL)) == []


def test_pool_refusals_launch_nothing(L):
    z, o = Dev(np.zeros(256, np.float32)), out(256)
    s = st()
    table = [("valid_fwd, H 2", lambda: L.spnet_maxpool3x3s2_valid_fwd(z.ptr, o.ptr, o.ptr, 1, 2, 3, 4, s)),
             ("valid_fwd, W 2", lambda: L.spnet_maxpool3x3s2_valid_fwd(z.ptr, o.ptr, o.ptr, 1, 3, 2, 4, s)),
             ("valid_bwd, H 2", lambda: L.spnet_maxpool3x3s2_valid_bwd(z.ptr, z.ptr, o.ptr, 1, 2, 3, 4, s)),
             ("valid_bwd, W 2", lambda: L.spnet_maxpool3x3s2_valid_bwd(z.ptr, z.ptr, o.ptr, 1, 3, 2, 4, s)),
             ("add_fwd, C % 4", lambda: L.spnet_maxpool3x3s2_add_fwd(z.ptr, None, o.ptr, o.ptr, 1, 3, 3, 6, None, None, s)),
             ("bwd, C % 4", lambda: L.spnet_maxpool3x3s2_bwd(z.ptr, z.ptr, o.ptr, 1, 3, 3, 6, s)),
             ("bwd_bnsums, C % 4", lambda: L.spnet_maxpool3x3s2_bwd_bnsums(z.ptr, z.ptr, o.ptr, 1, 3, 3, 6, z.ptr, z.ptr, z.ptr, o.ptr, 1, s)),
             ("bwd_bnsums, no yp", lambda: L.spnet_maxpool3x3s2_bwd_bnsums(z.ptr, z.ptr, o.ptr, 1, 3, 3, 4, None, z.ptr, z.ptr, o.ptr, 1, s)),
             ("valid_fwd, C % 4", lambda: L.spnet_maxpool3x3s2_valid_fwd(z.ptr, o.ptr, o.ptr, 1, 3, 3, 6, s)),
             ("avgpool3x3s1, C % 4", lambda: L.spnet_avgpool3x3s1_same(z.ptr, o.ptr, 1, 3, 3, 6, 0, s))]
    wrong = []
    for name, call in table:
        try:
            call()
            wrong.append(name + ": no HipError")
        except L.HipError as e:
            if not str(e).endswith("hipError_t 1"):
                wrong.append(name + ": " + str(e))
        torch.cuda.synchronize()
        if o.check(np.full(o.n, R.SENTINEL)) != []:
            wrong.append(name + ": output written")
            break
    assert wrong == []


@pytest.mark.parametrize("H", AVG2_N)
@pytest.mark.parametrize("W", AVG2_N)
def test_avgpool2(L, H, W):
    """inputs are multiples of 4: sums of four and the product with 0.25 are exact; the dropped odd row / column gets a
    zero gradient (and H or W of 1 gives an empty output: nothing may be written)"""
    found = []
    for C in AVG2_C:
        for B in (1, 2):
            x = 4 * R.ints((B, H, W, C), -2, 2, 7000 + H * 100 + W * 10 + C)
            dy = 4 * R.ints((B, H // 2, W // 2, C), -2, 2, 7500 + H * 100 + W * 10 + C)
            xd, dyd = Dev(x), Dev(dy)
            y, dx = out(dy.size), out(x.size)
            L.spnet_avgpool2_fwd(xd.ptr, y.ptr, B, H, W, C, st())
            L.spnet_avgpool2_bwd(dyd.ptr, dx.ptr, B, H, W, C, st())
            want_dx = R.avgpool2_bwd(dy, H, W)
            assert not want_dx[:, 2 * (H // 2):].any() and not want_dx[:, :, 2 * (W // 2):].any()
            found += tag(y.check(R.avgpool2_fwd(x)), "B%d C%d y" % (B, C)) + tag(dx.check(want_dx), "B%d C%d dx" % (B, C))
    assert found == []


U = 2.0 ** -24            # unit roundoff of fp32


def within(dev, want, bound):
    """findings: the placed array within `bound` (elementwise) of the float64 reference, guards intact"""
    got = dev.host()
    found = R.check_guards(got, dev.n)
    err = np.abs(got[R.FRONT:R.FRONT + dev.n].astype(np.float64) - want.ravel())
    bad = np.flatnonzero(~(err <= bound.ravel()))
    if bad.size:
        found.append("%d elements beyond the bound, first at %d: error %g, bound %g" % (bad.size, bad[0], err[bad[0]], bound.ravel()[bad[0]]))
    return found


@pytest.mark.parametrize("H", AVG3_N)
@pytest.mark.parametrize("W", AVG3_N)
def test_avgpool3x3s1_same(L, H, W):
    """Integer inputs: the window sum s (at most nine integers, fmaf with the factor 1) is exact.  With u = 2^-24:

    forward   y = fl(s * fl(1/n)): the reciprocal carries a relative error of at most u, the product another u, so
              |y - s/n| <= |s/n| * (2u + u^2).  (n in {1, 2, 4}: exact; the bound still holds.)
    backward  dx = a chain of at most nine fmaf(dy_j, fl(1/n_j), acc): each factor is off by at most u relative, which puts
              at most u * A into the sum, A = sum |dy_j| / n_j; each of the nine fmaf rounds a partial sum of magnitude at
              most A (1 + u) once, at most u of it.  |dx - exact| <= (1 + 9 (1 + u)) u A <= 10 u A (1 + u).

    The float64 reference itself is accurate to 2^-53 relative, far below either bound."""
    found = []
    for C in AVG3_C:
        for B in (1, 2):
            x = R.ints((B, H, W, C), -2, 2, 8000 + H * 100 + W * 10 + C)
            dy = R.ints((B, H, W, C), -2, 2, 8500 + H * 100 + W * 10 + C)
            xd, dyd = Dev(x), Dev(dy)
            y, dx = out(x.size), out(x.size)
            L.spnet_avgpool3x3s1_same(xd.ptr, y.ptr, B, H, W, C, 0, st())
            L.spnet_avgpool3x3s1_same(dyd.ptr, dx.ptr, B, H, W, C, 1, st())
            want, _ = R.avgpool3_fwd(x)
            found += tag(within(y, want, np.abs(want) * (2 * U + U * U)), "B%d C%d y" % (B, C))
            A = R.avgpool3_bwd(np.abs(dy))
            found += tag(within(dx, R.avgpool3_bwd(dy), 10 * U * A * (1 + U)), "B%d C%d dx" % (B, C))
    assert found == []
