"""spnet_calc_errors and spnet_ellipse_iou (csrc/metrics.hip) against tests/helpers/metrics_ref.py: integer counts, the
centre error and the IoU double bit for bit, every output behind guards and pre-filled.  The only tolerance is the derived
boundary-safety margin of the IoU table, which lives in the helper and is applied on the CPU (tests/test_metrics_ref_cpu.py);
every assertion here is an equality or an empty list of findings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import metrics_ref as R
from tests.helpers.dw_ref import SENTINEL
from tests.test_dwconv_gpu import Dev, out, st
from tests.test_irv2_glue_gpu import run_refusals
from tests.test_tracks_gpu import GUARD, PATTERN, Guarded


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


# ---- calc_errors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,ncols", R.ERROR_CASES)
def test_calc_errors(L, N, ncols):
    yp, yt = R.errors_case(N, ncols)
    want_counts, want_pix = R.calc_errors(yp, yt)
    dp, dt = Dev(yp), Dev(yt)
    counts = Guarded(7)
    counts.buf[GUARD:GUARD + 7] = torch.tensor(R.COUNTS0, dtype=torch.int32, device="cuda")
    pix = out(N)
    L.spnet_calc_errors(dp.ptr, dt.ptr, N, ncols, counts.ptr, pix.ptr, st())
    torch.cuda.synchronize()
    assert counts.host((7,)).tolist() == want_counts
    assert pix.guards() == []
    assert np.array_equal(pix.head(N).view(np.int32), want_pix.astype(np.float32).view(np.int32))


# ---- ellipse_iou -----------------------------------------------------------------------------------------------------------
class GuardedDoubles:
    """n doubles between GUARD canary doubles, pre-filled with a NaN"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float(PATTERN), dtype=torch.float64, device="cuda")
        self.buf[GUARD:GUARD + n] = float("nan")
        self.ptr = self.buf.data_ptr() + 8 * GUARD

    def host(self):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == float(PATTERN)).all() and (h[GUARD + self.n:] == float(PATTERN)).all(), "a canary was overwritten"
        return h[GUARD:GUARD + self.n].copy()


def iou_findings(L, key, npairs):
    nx, ny, names, yp, yt, want = R.iou_table()[key]
    dp, dt, iou = Dev(yp[:npairs]), Dev(yt[:npairs]), GuardedDoubles(npairs)
    L.spnet_ellipse_iou(dp.ptr, dt.ptr, npairs, nx, ny, iou.ptr, st())
    torch.cuda.synchronize()
    got = iou.host()
    bad = np.flatnonzero(got.view(np.int64) != want[:npairs].view(np.int64))
    return ["%s: %r, expected %r" % (names[k], got[k], want[k]) for k in bad]


@pytest.mark.parametrize("npairs", (1, 72, 1000))
def test_ellipse_iou_on_the_full_canvas(L, npairs):
    assert iou_findings(L, "big", npairs) == []


def test_ellipse_iou_at_the_borders_of_a_small_canvas(L):
    assert iou_findings(L, "small", len(R.iou_table()["small"][2])) == []


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_metrics_refusals_launch_nothing(L):
    """the grids behind yp / yt hold 3 x 576 floats and the IoU rows 72 x 8, more than any of these calls would read if it were
    not refused; pix_err has 8192 floats, counts 7 ints, iou 72 doubles"""
    yp, yt = R.errors_case(3, 576)
    dp, dt, pix = Dev(yp), Dev(yt), out(8192)
    counts = Guarded(7)
    s = st()
    err = lambda p=dp.ptr, t=dt.ptr, N=3, ncols=576, c=counts.ptr, x=pix.ptr: L.spnet_calc_errors(p, t, N, ncols, c, x, s)
    table = [("calc_errors, yp NULL", lambda: err(p=None)), ("calc_errors, yt NULL", lambda: err(t=None)),
             ("calc_errors, counts NULL", lambda: err(c=None)), ("calc_errors, pix_err NULL", lambda: err(x=None)),
             ("calc_errors, N 0", lambda: err(N=0)), ("calc_errors, N -1", lambda: err(N=-1)),
             ("calc_errors, ncols 0", lambda: err(ncols=0)), ("calc_errors, ncols 4", lambda: err(ncols=4)),
             ("calc_errors, ncols 12", lambda: err(ncols=12)), ("calc_errors, ncols -8", lambda: err(ncols=-8))]
    nx, ny, names, bp, bt, want = R.iou_table()["small"]
    n = len(names)
    ep, et, iou = Dev(bp), Dev(bt), GuardedDoubles(n)
    run = lambda p=ep.ptr, t=et.ptr, k=n, x=nx, y=ny, o=iou.ptr: L.spnet_ellipse_iou(p, t, k, x, y, o, s)
    table += [("ellipse_iou, yp NULL", lambda: run(p=None)), ("ellipse_iou, yt NULL", lambda: run(t=None)),
              ("ellipse_iou, iou NULL", lambda: run(o=None)), ("ellipse_iou, npairs 0", lambda: run(k=0)),
              ("ellipse_iou, npairs -1", lambda: run(k=-1)), ("ellipse_iou, nx 0", lambda: run(x=0)), ("ellipse_iou, ny 0", lambda: run(y=0)),
              ("ellipse_iou, nx -64", lambda: run(x=-64)), ("ellipse_iou, nx above the cap", lambda: run(x=R.MAX_EXTENT + 1)),
              ("ellipse_iou, ny above the cap", lambda: run(y=R.MAX_EXTENT + 1))]
    assert run_refusals(L, table, (pix,)) == []
    assert (counts.host((7,)) == PATTERN).all() and np.isnan(iou.host()).all()
    # valid calls afterwards still give the right answers; the largest canvas is not refused
    assert iou_findings(L, "small", n) == []
    run(x=R.MAX_EXTENT, y=R.MAX_EXTENT)
    torch.cuda.synchronize()
    assert np.isfinite(iou.host()).all()
    counts.buf[GUARD:GUARD + 7] = 0
    err()
    torch.cuda.synchronize()
    assert counts.host((7,)).tolist() == R.calc_errors(yp, yt, counts0=(0,) * 7)[0]
