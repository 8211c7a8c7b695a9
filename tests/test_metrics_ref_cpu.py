"""The case tables of tests/test_metrics_gpu.py, proved on the CPU (tests/helpers/metrics_ref.py): the calc_errors table is
exact in integers and holds every rounding and ring case; the IoU table is boundary-safe by the derived margin and holds
every named case; each planted defect changes the expected output of at least one case.  No GPU."""
import numpy as np
import pytest

from tests.helpers import metrics_ref as R

SMALL_ERRORS = [c for c in R.ERROR_CASES if c[0] * c[1] < 1 << 20]


def test_rounding_is_half_to_even_in_integers():
    want = [0, 0, 0, 1, 1, 2, 2, 0, -1]
    assert [R.rint_fraction(v) for v in R.NOOBJ] == want
    assert R.errors_rint(np.array(R.NOOBJ, np.float32)).tolist() == want
    assert R.errors_rint(np.array(R.NOOBJ, np.float32), half_up=True).tolist() == [0, 0, 1, 1, 1, 2, 3, 0, -1]
    assert np.signbit(np.float32(R.NOOBJ[0])) and float(np.float32(R.NOOBJ[3])) == 0.5 + 2.0 ** -24 > 0.5
    with pytest.raises(AssertionError):
        R.errors_rint(np.array([np.nan], np.float32))
    d = [abs(np.float32(t) - np.float32(p)) for t, p in R.RINGS]
    assert [float(v) for v in d] == [0.0, 0.5, 0.5, 0.5 + 2.0 ** -24, 0.5 + 2.0 ** -24, 2.0]


def test_the_errors_table_holds_every_combination():
    seen_no, seen_ring = set(), set()
    for N, ncols in SMALL_ERRORS:
        yp, yt = R.errors_case(N, ncols)
        P, T = yp.reshape(-1, 8), yt.reshape(-1, 8)
        seen_no |= set(zip(T[:, 6].tolist(), P[:, 6].tolist()))
        both = (R.errors_rint(T[:, 6]) == 0) & (R.errors_rint(P[:, 6]) == 0)
        seen_ring |= set(zip(T[both, 7].tolist(), P[both, 7].tolist()))
        if ncols > 8:                                   # large centre differences everywhere but in predictor 0
            other = np.ones(P.shape[0], bool)
            other[::ncols // 8] = False
            assert (np.abs(P[other, :2] - T[other, :2]).min(axis=1) > 1000).all()
        counts, pix = R.calc_errors(yp, yt)
        assert pix.shape == (N,) and set(pix.tolist()) <= {5.0, 13.0, 0.0, 17.0, 10.0, 25.0, 29.0, 9.0}
        got = [c - c0 for c, c0 in zip(counts, R.COUNTS0)]
        assert got[2] == got[4] + got[5] and got[5] == got[0] + got[1] and got[2] + got[3] + got[6] == N * ncols // 8
    assert len(seen_no) == 81 and len(seen_ring) == len(R.RINGS)
    assert R.ERROR_CASES[-1][0] * R.ERROR_CASES[-1][1] // 8 > R.EW_CAP_ITEMS and all(c > 0 for c in R.COUNTS0)


def test_the_errors_oracle_agrees_with_python_integers():
    yp, yt = R.errors_case(3, 576)
    c = [0] * 7
    for p, t in zip(yp.reshape(-1, 8), yt.reshape(-1, 8)):
        there, predicted = R.rint_fraction(t[6]) == 0, R.rint_fraction(p[6]) == 0
        if there:
            c[2] += 1
            if predicted:
                c[5] += 1
                c[0 if abs(R.Fraction(float(t[7])) - R.Fraction(float(p[7]))) > R.Fraction(1, 2) else 1] += 1
            else:
                c[4] += 1
        else:
            c[3 if predicted else 6] += 1
    assert R.calc_errors(yp, yt, counts0=(0,) * 7)[0] == c


@pytest.mark.parametrize("defect", R.DEFECTS_ERRORS)
def test_the_errors_table_notices_the_planted_defect(defect):
    hits = []
    for case in SMALL_ERRORS:
        yp, yt = R.errors_case(*case)
        a, b = R.calc_errors(yp, yt), R.calc_errors(yp, yt, defect=defect)
        if a[0] != b[0] or not np.array_equal(a[1], b[1]):
            hits.append(case)
    assert hits, defect
    print(defect, "->", hits)


# ---- IoU ---------------------------------------------------------------------------------------------------------------------
def test_the_iou_table_is_boundary_safe_and_holds_every_case():
    t = R.iou_table()
    margin, ties = 0.0, 0
    for key in ("big", "small"):
        nx, ny, names, yp, yt, want = t[key]
        for rp, rt in zip(yp, yt):
            safe, n, m = R.pair_safe(rp, rt, nx, ny)
            assert safe
            margin, ties = max(margin, m), ties + n
    print("TRIG_ULPS %d: largest margin %.3g, %d exact ties, %d candidates rejected" % (R.TRIG_ULPS, margin, ties, t["rejected"]))
    assert margin < 1e-4 and ties >= 2
    nx, ny, names, yp, yt, want = t["big"]
    assert len(names) == 1000 and yp.shape == (1000, 8)
    w = dict(zip(names, want))
    box = {}
    for name, rp, rt in zip(names[:20], yp, yt):
        ep, et = R.Ellipse(rp, nx, ny), R.Ellipse(rt, nx, ny)
        if ep.active and et.active:
            x0, x1, y0, y1 = R.union_box(ep, et)
            box[name] = (x1 - x0) * (y1 - y0)
    assert box["box below 256 pixels"] < 256 and box["box no multiple of 256"] % 256 and box["opposite corners"] > 100000
    assert 0 < w["box below 256 pixels"] < 1 and 0 < w["box no multiple of 256"] < 1 and 0 < w["circle"] < 1
    assert w["opposite corners"] == 0.0 and w["prediction empty, IoU 0"] == 0.0 and w["truth outside the canvas, IoU 0"] == 0.0
    assert w["both empty, -1"] == -1.0 and w["true noobj just above 0.99"] == -1.0 and w["true noobj 0.99"] == 0.0
    assert w["predicted noobj just below 0.5"] > 0 and w["predicted noobj 0.5"] == 0.0
    assert w["a == 0"] == 0.0 and w["a < 0"] == 0.0 and w["b == 0 in the truth"] == 0.0 and 0 < w["aligned, with exact ties"] < 1
    k = names.index("one pixel")
    assert R.Ellipse(yp[k], nx, ny).raster().sum() == 1 and 0 < w["one pixel"] < 1
    assert (want[20:] > 0).sum() > 500 and (want[20:] == -1).sum() > 50
    nx, ny, names, yp, yt, want = t["small"]
    assert ((want > 0) & (want < 1)).all()                                  # every border case overlaps for real
    for rp, name in zip(yp, names[:5]):                                     # the box is cut by the border it is named for
        e = R.Ellipse(rp, nx, ny)
        cut = {"left border": e.cx - e.a < 0, "right border": e.cx + e.a > nx, "top border": e.cy - e.b < 0,
               "bottom border": e.cy + e.b > ny, "corner": e.x1 == nx and e.y1 == ny}[name]
        assert cut, name


def test_the_oracle_raster_is_the_host_metric():
    """the project's own host raster (diagnostics.create_ellipse_image) counts the same pixels on these safe pairs"""
    from spnet_amd import diagnostics as D
    nx, ny, names, yp, yt, want = R.iou_table()["small"]
    for rp, rt, w in zip(yp, yt, want):
        a, b = D.create_ellipse_image(rp, nx, ny) > 0, D.create_ellipse_image(rt, nx, ny) > 0
        assert w == (a & b).sum() / (a | b).sum()


@pytest.mark.parametrize("defect", R.DEFECTS_IOU)
def test_the_iou_table_notices_the_planted_defect(defect):
    t = R.iou_table()
    hits = []
    for key in ("big", "small"):
        nx, ny, names, yp, yt, want = t[key]
        for name, rp, rt, w in zip(names[:40], yp, yt, want):
            if R.iou_value(R.iou_counts(rp, rt, nx, ny, defect)) != w:
                hits.append(name)
    assert hits, defect
    print(defect, "->", hits[:6])
