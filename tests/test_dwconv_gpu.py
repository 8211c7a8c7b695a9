"""The depthwise 3x3 family (csrc/dwconv.hip) against exact integer sums (tests/helpers/dw_ref.py), behind guards.

Operands are small integers (dw_ref.draw_dw; the affine makes a == 0 a frequent value), so every fmaf and every summation
order is exact: each case demands the float64 reference bit for bit -- y, dx, dw, every partial row of the documented
layouts -- and that nothing outside a tensor was written.  Every device tensor sits at a 16-byte-aligned offset > 0 of a
larger allocation: inputs between NaN, outputs between (and filled with) the sentinel 7.0, workspaces sized exactly by
the library's *_ws() / *_rows() answers, NaN inside and the sentinel behind.  assert_exact_dw runs on the CPU before
anything is launched.  There is no tolerance in this file: every assertion is an equality or an empty list of findings.

The tables are read by tests/test_dw_ref_cpu.py as well, which confirms through the library's host-only functions that
every row takes the path it is there for, that its operands are exact and that its data holds the ties it is there for."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import dw_ref as R
from tests.helpers import gemm_ref as G


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


# (B, H, W, C).  cfg 1: 6x8 pixel tiles x 64 channels (H <= 6 and W <= 8); cfg 0: 12x16 x 32 channels
CFG1 = [(1, 1, 1, 4), (3, 6, 8, 64), (2, 5, 7, 36), (1, 6, 1, 68), (1, 1, 8, 4),
        (2, 3, 4, 516)]                 # 9 channel chunks: the XCD remap is on, the last chunk is ragged
CFG0 = [(1, 7, 1, 4), (1, 1, 9, 36),
        (2, 12, 16, 32),                # exactly one tile
        (3, 13, 17, 36),                # 2x2 tiles with one-pixel ragged edges and a one-quad ragged chunk
        (1, 11, 15, 64), (1, 25, 33, 4),
        (2, 13, 17, 260)]               # 9 chunks: the remap is on, with a ragged chunk
STRIDE1 = CFG1 + CFG0
# streaming only: planes shorter than the 4-row / 3-row load rings, W in {7, 9}, and 3 strips x 2 chunks x 3 images = 18
# waves per segment, so that the wave count is no multiple of 4 for rows_per_seg 2, 3, 5, H and the library's choice
STREAM_EXTRA = [(1, 2, 7, 4), (1, 3, 9, 36), (1, 4, 8, 32), (3, 5, 17, 36)]
STREAM = STRIDE1 + STREAM_EXTRA
ALL = STREAM
BNFIN_SHAPES = [(2, 5, 7, 36), (3, 13, 17, 36), (2, 13, 17, 260)]
BNFIN_ROWS = [1, 15, 16, 17, 128]       # the prologue sums 16 interleaved groups of partial rows
STRIDED_HW = [(1, 1), (2, 2), (3, 3), (4, 5), (9, 8)]         # pad-before 0 and 1 at stride 2
STRIDED_C, STRIDED_B = (4, 36, 260), (1, 3)
# dws_rows = min(256, ceil(B*OH*OW / (8 * 256/chan_lanes))): chan_lanes(1) = 8 gives 32 pixel rows per workgroup, so the
# cap of 256 is reached from 255*256 + 1 output pixels on; at C = 4 that is the smallest such tensor (wider planes reach
# it with fewer pixels but more floats).  264 x 256 pixels ask for 264 rows: capped, and the pixel loop wraps.
ROW_CAP = (1, 264, 256, 4, 1)           # B, H, W, C, stride


def sid(shape):
    return "x".join(str(v) for v in shape)


def seed_of(shape):
    return ALL.index(shape)


@functools.lru_cache(maxsize=None)
def case(shape):
    return R.draw_dw(*shape, seed_of(shape))


def rps_values(shape, backward):
    """rows_per_seg arguments {0, 1, 2, 3, 5, H, H+3} with distinct geometry once clamped"""
    B, H, W, C = shape
    seen, out = set(), []
    for rps in (0, 1, 2, 3, 5, H, H + 3):
        g = R.stream_geom(B, H, W, C, rps, backward)
        if g[3] not in seen:
            seen.add(g[3])
            out.append(rps)
    return out


# (name, relu_in, add, affine, bn_partial, bn_x): the option sets the engine uses
OPTIONS = [("plain-relu0", 0, 0, 0, 0, 0), ("plain-relu1", 1, 0, 0, 0, 0), ("add-relu0", 0, 1, 0, 0, 0), ("add-relu1", 1, 1, 0, 0, 0),
           ("affine+bn-relu0", 0, 0, 1, 1, 0), ("affine+bn-relu1", 1, 0, 1, 1, 0),
           ("add+affine+bn-relu0", 0, 1, 1, 1, 0), ("add+affine+bn-relu1", 1, 1, 1, 1, 0),
           ("bnx+bn-relu1", 1, 0, 0, 1, 1), ("add+bnx+bn-relu1", 1, 1, 0, 1, 1)]


def option_args(d, opt):
    _, relu_in, add, affine, bn, bnx = opt
    return dict(relu_in=relu_in, add=d["add"] if add else None, scale=d["scale"] if affine else None,
                shift=d["shift"] if affine else None, mean=d["mean"] if bn else None, invstd=d["invstd"] if bn else None,
                bn_x=d["bn_x"] if bnx else None)


@functools.lru_cache(maxsize=None)
def fused(shape, k):
    d = case(shape)
    kw = option_args(d, OPTIONS[k])
    R.assert_exact_dw(d["dy"], d["x"], d["w"], **{n: v for n, v in kw.items() if n != "relu_in"})
    return R.Fused(d["dy"], d["x"], d["w"], **kw)


# ---- guarded device tensors --------------------------------------------------------------------------------------------------
class Dev:
    """a dense array at a 16-byte-aligned offset > 0 of a larger device allocation (dw_ref.place): .ptr = its first element"""

    def __init__(self, arr, poison=R.NAN, inside=None):
        buf, off = R.place(arr, poison, inside=inside)
        self.n = int(np.asarray(arr).size)
        self.t = torch.from_numpy(buf).cuda()
        self.ptr = self.t.data_ptr() + 4 * off
        assert self.ptr % 16 == 0 and off > 0

    def host(self):
        return self.t.cpu().numpy()

    def check(self, want):
        return R.check_placed(self.host(), want)

    def guards(self):
        return R.check_guards(self.host(), self.n)

    def head(self, n):
        return self.host()[R.FRONT:R.FRONT + n]


def out(n):
    """an output: the sentinel inside and around"""
    return Dev(np.full(int(n), R.SENTINEL, np.float32), R.SENTINEL)


def work(n):
    """a workspace of exactly n floats: NaN inside, the sentinel before and behind"""
    return Dev(np.empty(int(n), np.float32), R.SENTINEL, inside=R.NAN)


PLANE_SENTINEL = 0x40E0                  # bf16 7.0
PLANE_FRONT, PLANE_TAIL = 8, 64          # words: 16 bytes in front


class Planes:
    """a zeroed allocation of exactly 3 * spnet_bf16x3_plane_elems bf16 inside a sentinel-filled bf16 buffer"""

    def __init__(self, L, rows, K):
        self.ps = int(L.spnet_bf16x3_plane_elems(rows, K))
        assert self.ps == R.plane_elems(rows, K)
        buf = np.full(PLANE_FRONT + 3 * self.ps + PLANE_TAIL, PLANE_SENTINEL, np.uint16)
        buf[PLANE_FRONT:PLANE_FRONT + 3 * self.ps] = 0
        self.t = torch.from_numpy(buf.view(np.int16)).cuda()
        self.ptr = self.t.data_ptr() + 2 * PLANE_FRONT
        assert self.ptr % 16 == 0

    def host(self):
        return self.t.cpu().numpy().view(np.uint16)

    def check(self, want):
        return R.check_planes(self.host(), want, PLANE_FRONT, PLANE_TAIL, PLANE_SENTINEL)


def P(d):
    return None if d is None else d.ptr


class Form:
    """the tiled form (rps None) or the streaming form with a rows_per_seg argument, behind one call shape"""

    def __init__(self, L, rps):
        self.L, self.rps = L, rps

    def rows(self, B, H, W, C):
        return int(self.L.spnet_dwconv3x3_tiled_rows(B, H, W, C) if self.rps is None else self.L.spnet_dwconv3x3_stream_rows(B, H, W, C, self.rps))

    def ws(self, B, H, W, C):
        return int(self.L.spnet_dwconv3x3_tiled_bwd_ws(B, H, W, C) if self.rps is None else self.L.spnet_dwconv3x3_stream_bwd_ws(B, H, W, C, self.rps))

    def regions(self, B, H, W):
        return R.tiled_regions(B, H, W) if self.rps is None else R.stream_regions(B, H, W, self.rps)

    def fwd(self, x, w, y, shape, relu_in, sc, sh):
        if self.rps is None:
            return self.L.spnet_dwconv3x3_tiled_fwd(x, w, y, *shape, relu_in, sc, sh, st())
        return self.L.spnet_dwconv3x3_stream_fwd(x, w, y, *shape, relu_in, sc, sh, self.rps, st())

    def fwd_x3(self, x, w, planes, shape, relu_in, sc, sh):
        if self.rps is None:
            return self.L.spnet_dwconv3x3_tiled_fwd_x3(x, w, planes, *shape, relu_in, sc, sh, st())
        return self.L.spnet_dwconv3x3_stream_fwd_x3(x, w, planes, *shape, relu_in, sc, sh, self.rps, st())

    def bwd(self, dy, x, w, dx, dw, shape, relu_in, add, ws, sc, sh, mu, inv, bnp, bnx):
        if self.rps is None:
            return self.L.spnet_dwconv3x3_tiled_bwd(dy, x, w, dx, dw, *shape, relu_in, add, ws, sc, sh, mu, inv, bnp, bnx, st())
        return self.L.spnet_dwconv3x3_stream_bwd(dy, x, w, dx, dw, *shape, relu_in, add, ws, sc, sh, mu, inv, bnp, bnx, self.rps, st())


def tag(found, name):
    return ["%s: %s" % (name, f) for f in found]


# ---- forward -----------------------------------------------------------------------------------------------------------------
def forward_findings(L, shape, rps):
    B, H, W, C = shape
    d = case(shape)
    F = Form(L, rps)
    x, w, sc, sh = Dev(d["x"]), Dev(d["w"]), Dev(d["scale"]), Dev(d["shift"])
    found = []
    for relu_in in (0, 1):
        for affine in (0, 1):
            k = relu_in + (4 if affine else 0)              # the option set with this relu_in / affine: the same y
            want = fused(shape, k).y
            assert np.abs(want).max() < 256                 # (its own high bf16 piece)
            y = out(B * H * W * C)
            F.fwd(x.ptr, w.ptr, y.ptr, shape, relu_in, sc.ptr if affine else None, sh.ptr if affine else None)
            found += tag(y.check(want), "y relu %d affine %d" % (relu_in, affine))
            pl = Planes(L, B * H * W, C)
            F.fwd_x3(x.ptr, w.ptr, pl.ptr, shape, relu_in, sc.ptr if affine else None, sh.ptr if affine else None)
            found += tag(pl.check(want.reshape(B * H * W, C)), "planes relu %d affine %d" % (relu_in, affine))
    return found


@pytest.mark.parametrize("shape", STRIDE1, ids=sid)
def test_tiled_forward_and_planes(L, shape):
    assert forward_findings(L, shape, None) == []


@pytest.mark.parametrize("shape", STREAM, ids=sid)
def test_stream_forward_and_planes(L, shape):
    for rps in rps_values(shape, False):
        assert forward_findings(L, shape, rps) == [], "rows_per_seg %d" % rps


# ---- fused backward ----------------------------------------------------------------------------------------------------------
def reduce_job(L, src_ptr, rows, Lw, dst):
    jobs = torch.tensor([src_ptr, dst.ptr, rows, Lw], dtype=torch.int64, device="cuda")
    L.spnet_reduce_rows_batched(jobs.data_ptr(), 1, Lw, st())
    torch.cuda.synchronize()


def backward_findings(L, shape, rps):
    B, H, W, C = shape
    d = case(shape)
    F = Form(L, rps)
    rows, nws, regions = F.rows(B, H, W, C), F.ws(B, H, W, C), F.regions(B, H, W)
    assert rows == len(regions) and nws >= rows * 9 * C
    dev = {k: Dev(d[k]) for k in ("x", "dy", "add", "bn_x", "w", "scale", "shift", "mean", "invstd")}
    found = []
    for k, opt in enumerate(OPTIONS):
        name, relu_in, add, affine, bn, bnx = opt
        ref = fused(shape, k)
        want_rows = ref.weight_rows(regions)
        args = lambda dx, dw, ws, bnp: (dev["dy"].ptr, dev["x"].ptr, dev["w"].ptr, dx.ptr, P(dw), shape, relu_in,
                                        dev["add"].ptr if add else None, ws.ptr, dev["scale"].ptr if affine else None,
                                        dev["shift"].ptr if affine else None, dev["mean"].ptr if bn else None,
                                        dev["invstd"].ptr if bn else None, P(bnp), dev["bn_x"].ptr if bnx else None)
        # 1. with dw: the library folds the partial rows itself
        dx, dw, ws = out(B * H * W * C), out(9 * C), work(nws)
        bnp = out(rows * 2 * C) if bn else None
        F.bwd(*args(dx, dw, ws, bnp))
        found += tag(dx.check(ref.dx), name + " dx") + tag(dw.check(ref.dw), name + " dw") + tag(ws.guards(), name + " workspace")
        if bn:
            found += tag(bnp.check(ref.bn_rows(regions)), name + " bn_partial")
        # 2. dw == NULL: the partial rows stay in the workspace, row by row as documented, for spnet_reduce_rows_batched
        dx, dw, ws = out(B * H * W * C), out(9 * C), work(nws)
        bnp = out(rows * 2 * C) if bn else None
        F.bwd(*args(dx, None, ws, bnp))
        found += tag(dx.check(ref.dx), name + " dx (dw NULL)") + tag(ws.guards(), name + " workspace (dw NULL)")
        found += tag(G.check_dense(ws.head(rows * 9 * C), want_rows), name + " partial rows")
        if bn:
            found += tag(bnp.check(ref.bn_rows(regions)), name + " bn_partial (dw NULL)")
        reduce_job(L, ws.ptr, rows, 9 * C, dw)
        found += tag(dw.check(ref.dw), name + " dw folded by reduce_rows_batched")
    return found


@pytest.mark.parametrize("shape", STRIDE1, ids=sid)
def test_tiled_backward(L, shape):
    assert backward_findings(L, shape, None) == []


STREAM_BWD = [(s, rps) for s in STREAM for rps in rps_values(s, True)]


@pytest.mark.parametrize("shape,rps", STREAM_BWD, ids=lambda v: sid(v) if isinstance(v, tuple) else "rps%d" % v)
def test_stream_backward(L, shape, rps):
    assert backward_findings(L, shape, rps) == []


# ---- the producer BatchNorm's finalize folded into the tiled forward ---------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


@pytest.mark.parametrize("rows", BNFIN_ROWS)
@pytest.mark.parametrize("shape", BNFIN_SHAPES, ids=sid)
def test_tiled_forward_bnfin_is_finalize_then_forward(L, shape, rows):
    """The derived coefficients are no integers: the contract is bit-identity with spnet_bn_finalize_fwd followed by
    spnet_dwconv3x3_tiled_fwd(in_scale, in_shift) -- y, the planes, save_mean, save_invstd, scale_shift[2C] and both moving
    statistics -- with every buffer guarded."""
    B, H, W, C = shape
    d = case(shape)
    rs = np.random.RandomState(rows + C)
    M = B * H * W + 3
    part = rs.randn(rows, 2, C).astype(np.float32) * 3
    part[:, 1] = np.abs(part[:, 1]) * 40 + 10
    gamma, beta = (rs.rand(C) + 0.5).astype(np.float32), (rs.randn(C) * 0.3).astype(np.float32)
    mm0, mv0 = rs.randn(C).astype(np.float32), (rs.rand(C) + 0.5).astype(np.float32)
    x, w, g, b = Dev(d["x"]), Dev(d["w"]), Dev(gamma), Dev(beta)
    eps, mom = 1e-3, 0.99
    for relu_in in (0, 1):
        # the two-launch path
        p0 = Dev(part)
        mm, mv, sm, si, ss = Dev(mm0, R.SENTINEL), Dev(mv0, R.SENTINEL), out(C), out(C), out(2 * C)
        L.spnet_bn_finalize_fwd(p0.ptr, rows, M, C, g.ptr, b.ptr, mm.ptr, mv.ptr, sm.ptr, si.ptr, ss.ptr, eps, mom, st())
        y0, pl0 = out(B * H * W * C), Planes(L, B * H * W, C)
        L.spnet_dwconv3x3_tiled_fwd(x.ptr, w.ptr, y0.ptr, *shape, relu_in, ss.ptr, ss.ptr + 4 * C, st())
        L.spnet_dwconv3x3_tiled_fwd_x3(x.ptr, w.ptr, pl0.ptr, *shape, relu_in, ss.ptr, ss.ptr + 4 * C, st())
        ref = [t.host() for t in (y0, mm, mv, sm, si, ss)]
        assert not np.isnan(ref[0][R.FRONT:R.FRONT + y0.n]).any() and y0.guards() == [] and ss.guards() == [] and mm.guards() == []
        for x3 in (0, 1):
            p1 = Dev(part)
            mm1, mv1, sm1, si1, ss1 = Dev(mm0, R.SENTINEL), Dev(mv0, R.SENTINEL), out(C), out(C), out(2 * C)
            tail = (relu_in, p1.ptr, rows, M, g.ptr, b.ptr, mm1.ptr, mv1.ptr, sm1.ptr, si1.ptr, ss1.ptr, eps, mom, st())
            if x3:
                pl1 = Planes(L, B * H * W, C)
                L.spnet_dwconv3x3_tiled_fwd_bnfin_x3(x.ptr, w.ptr, pl1.ptr, *shape, *tail)
                assert np.array_equal(pl1.host(), pl0.host())                      # planes and their sentinel words
                got = [ref[0]] + [t.host() for t in (mm1, mv1, sm1, si1, ss1)]
            else:
                y1 = out(B * H * W * C)
                L.spnet_dwconv3x3_tiled_fwd_bnfin(x.ptr, w.ptr, y1.ptr, *shape, *tail)
                got = [t.host() for t in (y1, mm1, mv1, sm1, si1, ss1)]
            for name, a, r in zip(("y", "moving_mean", "moving_var", "save_mean", "save_invstd", "scale_shift"), got, ref):
                assert np.array_equal(bits(a), bits(r)), (name, x3, relu_in)           # values AND guards, bit for bit
            assert np.array_equal(bits(p1.host()), bits(p0.host()))                    # the partial rows are only read
    pl = pl0.host()
    assert (pl[:PLANE_FRONT] == PLANE_SENTINEL).all() and (pl[-PLANE_TAIL:] == PLANE_SENTINEL).all()


# ---- strided gather kernels --------------------------------------------------------------------------------------------------
def strided_seed(B, H, W, C, stride):
    return 1000 + 100 * stride + 10 * H + B + C


def strided_draw(B, H, W, C, stride, seed, v=2):
    """(x, dy, w) of a strided case, proved exact"""
    (OH, _), (OW, _) = R.same_geom(H, stride), R.same_geom(W, stride)
    x, dy, w = R.ints((B, H, W, C), -v, v, seed), R.ints((B, OH, OW, C), -v, v, seed + 1), R.ints((3, 3, C), -v, v, seed + 2)
    R.assert_exact_dw(dy, x, w, stride=stride)
    return x, dy, w


ROW_CAP_SEED = 77


def strided_findings(L, B, H, W, C, stride, seed, v=2, ops=(0, 1, 2)):
    (OH, _), (OW, _) = R.same_geom(H, stride), R.same_geom(W, stride)
    x, dy, w = strided_draw(B, H, W, C, stride, seed, v)
    xd, dyd, wd = Dev(x), Dev(dy), Dev(w)
    found = []
    name = "B%d C%d " % (B, C)
    if 0 in ops:
        y = out(B * OH * OW * C)
        L.spnet_dwconv3x3_strided(0, xd.ptr, wd.ptr, y.ptr, B, H, W, C, stride, None, st())
        found += tag(y.check(R.dw_fwd(x, w, stride)), name + "op 0")
    if 1 in ops:
        dx = out(B * H * W * C)
        L.spnet_dwconv3x3_strided(1, dyd.ptr, wd.ptr, dx.ptr, B, H, W, C, stride, None, st())
        found += tag(dx.check(R.dw_bwd_data(dy, w, H, W, stride)), name + "op 1")
    if 2 in ops:
        nws = int(L.spnet_dwconv3x3_strided_ws(B, H, W, C, stride))
        assert nws == R.strided_rows(B, OH, OW, C) * 9 * C
        dw, ws = out(9 * C), work(nws)
        L.spnet_dwconv3x3_strided(2, xd.ptr, dyd.ptr, dw.ptr, B, H, W, C, stride, ws.ptr, st())
        found += tag(dw.check(R.dw_bwd_weight(x, dy, stride)), name + "op 2") + tag(ws.guards(), name + "op 2 workspace")
        found += tag(["NaN left in the partial rows"] if np.isnan(ws.head(nws)).any() else [], name + "op 2")
    return found


@pytest.mark.parametrize("H,W", STRIDED_HW)
@pytest.mark.parametrize("stride", [1, 2])
def test_strided(L, stride, H, W):
    found = []
    for C in STRIDED_C:
        for B in STRIDED_B:
            found += strided_findings(L, B, H, W, C, stride, strided_seed(B, H, W, C, stride))
    assert found == []


def test_strided_weight_gradient_at_its_row_cap(L):
    """operands from {-1, 0, 1}: the sums run over 67,584 pixels"""
    B, H, W, C, stride = ROW_CAP
    assert R.strided_rows(B, H, W, C) == 256 and -(-(B * H * W) // 256) > 256
    assert strided_findings(L, B, H, W, C, stride, ROW_CAP_SEED, v=1) == []


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(L):
    """every argument set below is rejected before anything is launched (hipErrorInvalidValue), valid buffers all the same:
    the sentinel-filled buffer that stands for every output stays untouched"""
    B, H, W, C = 2, 5, 7, 8
    n = B * H * W * C
    z = Dev(np.zeros(4 * n, np.float32))
    o = out(max(8 * n, 3 * R.plane_elems(B * H * W, C)))
    s = st()
    X, Wt, O = z.ptr, z.ptr, o.ptr
    tf = lambda B=B, H=H, W=W, C=C: L.spnet_dwconv3x3_tiled_fwd(X, Wt, O, B, H, W, C, 1, None, None, s)
    tfx = lambda B=B, H=H, W=W, C=C, pl=O: L.spnet_dwconv3x3_tiled_fwd_x3(X, Wt, pl, B, H, W, C, 1, None, None, s)
    sf = lambda B=B, H=H, W=W, C=C: L.spnet_dwconv3x3_stream_fwd(X, Wt, O, B, H, W, C, 1, None, None, 0, s)
    sfx = lambda B=B, H=H, W=W, C=C, pl=O: L.spnet_dwconv3x3_stream_fwd_x3(X, Wt, pl, B, H, W, C, 1, None, None, 0, s)
    fin = lambda x3=0, B=B, H=H, W=W, C=C, rows=4, M=70, pl=O: (L.spnet_dwconv3x3_tiled_fwd_bnfin_x3 if x3 else L.spnet_dwconv3x3_tiled_fwd_bnfin)(
        X, Wt, pl, B, H, W, C, 1, X, rows, M, X, X, O, O, O, O, O, 1e-3, 0.99, s)
    tb = lambda B=B, H=H, W=W, C=C, mu=None, inv=None, bnp=None, bnx=None: L.spnet_dwconv3x3_tiled_bwd(
        X, X, Wt, O, O, B, H, W, C, 1, None, O, None, None, mu, inv, bnp, bnx, s)
    sb = lambda B=B, H=H, W=W, C=C, ws=O, mu=None, inv=None, bnp=None, bnx=None: L.spnet_dwconv3x3_stream_bwd(
        X, X, Wt, O, O, B, H, W, C, 1, None, ws, None, None, mu, inv, bnp, bnx, 0, s)
    sd = lambda op, C=C, stride=1, ws=O: L.spnet_dwconv3x3_strided(op, X, X, O, B, H, W, C, stride, ws, s)
    table = [("tiled_fwd, C % 4", lambda: tf(C=6)), ("tiled_fwd_x3, C % 4", lambda: tfx(C=6)), ("stream_fwd, C % 4", lambda: sf(C=6)),
             ("stream_fwd_x3, C % 4", lambda: sfx(C=6)), ("bnfin, C % 4", lambda: fin(C=6)), ("bnfin_x3, C % 4", lambda: fin(1, C=6)),
             ("tiled_bwd, C % 4", lambda: tb(C=6)), ("stream_bwd, C % 4", lambda: sb(C=6)),
             ("strided op 0, C % 4", lambda: sd(0, C=6)), ("strided op 1, C % 4", lambda: sd(1, C=6)), ("strided op 2, C % 4", lambda: sd(2, C=6)),
             ("strided, stride 3", lambda: sd(0, stride=3)), ("strided, op 3", lambda: sd(3)), ("strided, op -1", lambda: sd(-1)),
             ("strided op 2, no workspace", lambda: sd(2, ws=None)), ("stream_bwd, no workspace", lambda: sb(ws=None)),
             ("tiled_bwd, bn_partial without mean", lambda: tb(inv=X, bnp=O)), ("tiled_bwd, bn_partial without invstd", lambda: tb(mu=X, bnp=O)),
             ("stream_bwd, bn_partial without mean", lambda: sb(inv=X, bnp=O)), ("stream_bwd, bn_partial without invstd", lambda: sb(mu=X, bnp=O)),
             ("tiled_bwd, bn_x without bn_partial", lambda: tb(mu=X, inv=X, bnx=X)), ("stream_bwd, bn_x without bn_partial", lambda: sb(mu=X, inv=X, bnx=X)),
             ("tiled_fwd_x3, no planes", lambda: tfx(pl=None)), ("stream_fwd_x3, no planes", lambda: sfx(pl=None)), ("bnfin_x3, no planes", lambda: fin(1, pl=None)),
             ("tiled_fwd_x3, planes at 8 bytes", lambda: tfx(pl=O + 8)), ("stream_fwd_x3, planes at 8 bytes", lambda: sfx(pl=O + 8)),
             ("bnfin_x3, planes at 8 bytes", lambda: fin(1, pl=O + 8)),
             ("bnfin, rows 0", lambda: fin(rows=0)), ("bnfin, rows 129", lambda: fin(rows=129)), ("bnfin, M 0", lambda: fin(M=0)),
             ("bnfin_x3, rows 0", lambda: fin(1, rows=0)), ("bnfin_x3, rows 129", lambda: fin(1, rows=129)), ("bnfin_x3, M 0", lambda: fin(1, M=0)),
             ("stream_fwd, H*W*C*4 = 2^31", lambda: sf(B=1, H=8192, W=8192, C=8)), ("stream_fwd_x3, H*W*C*4 = 2^31", lambda: sfx(B=1, H=8192, W=8192, C=8)),
             ("stream_bwd, H*W*C*4 = 2^31", lambda: sb(B=1, H=8192, W=8192, C=8))]
    for dim in ("B", "H", "W"):
        for fname, f in (("tiled_fwd", tf), ("tiled_fwd_x3", tfx), ("bnfin", fin), ("bnfin_x3", lambda **kw: fin(1, **kw)), ("tiled_bwd", tb),
                         ("stream_fwd", sf), ("stream_fwd_x3", sfx), ("stream_bwd", sb)):
            for v in (0, -1):
                table.append(("%s, %s = %d" % (fname, dim, v), lambda f=f, dim=dim, v=v: f(**{dim: v})))
    wrong = []
    for name, call in table:
        try:
            call()
            wrong.append(name + ": no HipError")
        except L.HipError as e:
            if not str(e).endswith("hipError_t 1"):             # hipErrorInvalidValue
                wrong.append(name + ": " + str(e))
        torch.cuda.synchronize()
        if o.check(np.full(o.n, R.SENTINEL)) != []:
            wrong.append(name + ": output written")
            break
    assert wrong == []
