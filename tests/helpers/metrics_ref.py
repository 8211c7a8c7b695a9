"""TEST INFRASTRUCTURE -- the evaluation metrics of csrc/metrics.hip restated: spnet_calc_errors in integers,
spnet_ellipse_iou as a float64 raster on a table of pairs that no admissible libm can count differently.

calc_errors
    Every noobj value of the table is a multiple of 2^-25, so round-half-to-even is done on the scaled INTEGER (errors_rint);
    the ring difference is the fp32 subtraction the kernel makes, on operands whose difference is exact; the centre error
    comes from Pythagorean triples, so dx^2 + dy^2 is a perfect square and the fp32 root is exact (math.isqrt).  The counts
    are ADDED to what counts[] held.  NaN in noobj is outside the contract: (int)rintf(NaN) is not defined, and the host
    loop of diagnostics.calc_errors raises on it.

ellipse_iou
    The kernel takes th = -(atan2f(sin2t, cos2t) / 2), cosf(th), sinf(th) in fp32 and everything else in fp64.  iou_counts
    does the same with numpy's fp32 functions.  A device libm may differ from numpy's: TRIG_ULPS = 4 is the bound assumed
    here on each of atan2f, cosf and sinf, in units in the last place of the result (the HIP device library documents
    1 - 2 ulp for them, numpy's are within 1).  That gives, per ellipse,

        d_th = TRIG_ULPS * ulp32(|atan2|) / 2,      d_c = d_th + TRIG_ULPS * 2^-24 * 2       (|cos'|, |sin'| <= 1, ulp32(x <= 1) <= 2^-23)

    and per pixel, with u = dx cs + dy sn, w = -dx sn + dy cs, p = u / a, q = w / b,

        d_u = d_w = (|dx| + |dy|) (d_c + 4 * 2^-53),     d_p = d_u / a,     d_q = d_w / b,
        margin = 2 |p| d_p + 2 |q| d_q + d_p^2 + d_q^2 + 2^-48 (1 + p^2 + q^2)

    The last term covers every fp64 rounding of the chain and the one rounding that a contracted p*p + q*q saves.  A pair is
    boundary-safe when no pixel of either ellipse's box has |p^2 + q^2 - 1| <= margin.  Over the table the largest margin of
    a pixel near an outline (0.5 < p^2 + q^2 < 1.5) is 2.4e-5 (tests/test_metrics_ref_cpu.py prints it).  One exception, which is what lets the table tell `<` from `<=`: for
    sin2t == +0 and cos2t > 0 the trig values are atan2f = 0, cosf = 1, sinf = -0 on every conforming libm (C Annex F), so
    d_c = 0, and a pixel with (|p|, |q|) exactly (1, 0) or (0, 1) has p^2 + q^2 == 1 exactly: such tie pixels are allowed.

    Candidates are drawn from a fixed seed and the unsafe ones dropped (iou_table).  DEFECTS_* name one-line variants."""
import functools
import math
from fractions import Fraction

import numpy as np

# ---- calc_errors -----------------------------------------------------------------------------------------------------------
ULP_HALF = 2.0 ** -24                                   # the fp32 spacing above 0.5
NOOBJ = (-0.0, 0.49, 0.5, 0.5 + ULP_HALF, 1.0, 1.5, 2.5, -0.5, -0.5 - ULP_HALF)
RINGS = ((3.0, 3.0), (3.0, 3.5), (3.5, 3.0), (0.0, 0.5 + ULP_HALF), (0.5 + ULP_HALF, 0.0), (2.0, 4.0))   # (truth, prediction)
TRIPLES = ((3, 4), (5, 12), (0, 0), (8, 15), (-6, 8), (7, -24), (-20, -21), (0, 9))
COUNTS0 = (11, 22, 33, 44, 55, 66, 77)
EW_CAP_ITEMS = 8192 * 256
ERROR_CASES = [(N, ncols) for ncols in (8, 16, 576) for N in (1, 3, 257)] + [(EW_CAP_ITEMS + 300, 8)]
DEFECTS_ERRORS = ("round half up", ">= 0.5 for the ring test", "pix_err from the last predictor", "counts overwritten",
                  "true positives and false negatives swapped")
SCALE = 1 << 25


def errors_case(N, ncols):
    """(yp, yt) float32 [N][ncols]: predictor i of the flattened grid takes the noobj pair (i % 9, i // 9 % 9) and the ring pair
    i // 81 % 6, shifted by a start that differs from case to case; predictor 0 of row j holds the triple j % 8, the others a
    centre difference of more than 1000"""
    npred = ncols // 8
    i = np.arange(N * npred) + 7 * N + ncols
    no = np.array(NOOBJ, np.float32)
    rg = np.array(RINGS, np.float32)
    yt, yp = np.zeros((N * npred, 8), np.float32), np.zeros((N * npred, 8), np.float32)
    yt[:, 6], yp[:, 6] = no[i % 9], no[i // 9 % 9]
    yt[:, 7], yp[:, 7] = rg[i // 81 % 6, 0], rg[i // 81 % 6, 1]
    k = np.arange(N * npred)
    yt[:, 0], yt[:, 1] = 100 + k % 13, 50 + k % 11
    yp[:, 0], yp[:, 1] = yt[:, 0] + 1001 + k % 5, yt[:, 1] - 2000
    tr = np.array(TRIPLES, np.float32)[np.arange(N) % len(TRIPLES)]
    yp[::npred, 0], yp[::npred, 1] = yt[::npred, 0] + tr[:, 0], yt[::npred, 1] + tr[:, 1]
    return yp.reshape(N, ncols), yt.reshape(N, ncols)


def errors_rint(x, half_up=False):
    """round half to even of fp32 values that are multiples of 2^-25, in int64"""
    s = np.asarray(x, np.float64) * SCALE
    assert np.isfinite(s).all(), "NaN and infinite noobj values are outside the contract"
    n = s.astype(np.int64)
    assert np.array_equal(n.astype(np.float64), s), "a noobj value is no multiple of 2^-25"
    q, r = n // SCALE, n % SCALE
    up = (r > SCALE // 2) | ((r == SCALE // 2) & (True if half_up else (q % 2 == 1)))
    return q + up


def calc_errors(yp, yt, counts0=COUNTS0, defect=None):
    """(counts [7] Python ints, pix_err [N] ints as float64)"""
    assert defect is None or defect in DEFECTS_ERRORS
    N, ncols = yp.shape
    npred = ncols // 8
    P, T = yp.reshape(-1, 8), yt.reshape(-1, 8)
    half_up = defect == "round half up"
    there, predicted = errors_rint(T[:, 6], half_up) == 0, errors_rint(P[:, 6], half_up) == 0
    diff = np.abs(T[:, 7] - P[:, 7])                                       # the kernel's fp32 subtraction
    assert np.array_equal(diff.astype(np.float64), np.abs(T[:, 7].astype(np.float64) - P[:, 7].astype(np.float64)))
    miss = diff >= np.float32(0.5) if defect == ">= 0.5 for the ring test" else diff > np.float32(0.5)
    c = [int((there & predicted & miss).sum()), int((there & predicted & ~miss).sum()), int(there.sum()),
         int((~there & predicted).sum()), int((there & ~predicted).sum()), int((there & predicted).sum()),
         int((~there & ~predicted).sum())]
    if defect == "true positives and false negatives swapped":
        c[4], c[5] = c[5], c[4]
    if defect != "counts overwritten":
        c = [a + b for a, b in zip(c, counts0)]
    first = slice(npred - 1, None, npred) if defect == "pix_err from the last predictor" else slice(0, None, npred)
    d = P[first, :2].astype(np.float64) - T[first, :2].astype(np.float64)
    assert np.array_equal(d, np.round(d))
    s = (d[:, 0] ** 2 + d[:, 1] ** 2).astype(np.int64)
    root = np.array([math.isqrt(int(v)) for v in np.unique(s)])
    pix = root[np.searchsorted(np.unique(s), s)].astype(np.float64)
    if defect is None:
        assert np.array_equal(pix * pix, s.astype(np.float64)), "a centre difference is no Pythagorean triple"
    return c, pix


def rint_fraction(x):
    """the same rounding in Python's own integers: round() of a Fraction is half-to-even"""
    return round(Fraction(float(np.float32(x))))


# ---- ellipse_iou -----------------------------------------------------------------------------------------------------------
TRIG_ULPS = 4
MAX_EXTENT = 32768
DEFECTS_IOU = ("< instead of <=", "box without the +1", "union box from one ellipse only", "angle sign flipped", "half angle dropped")


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


class Ellipse:
    """one predictor row on an nx x ny canvas, as make_ellipse() sees it"""

    def __init__(self, row, nx, ny, defect=None):
        v = np.asarray(row, np.float32)
        a, b, noobj = v[2], v[3], v[6]
        self.active = bool(noobj < np.float32(0.5) and a > 0 and b > 0)
        self.cx, self.cy, self.a, self.b = (float(t) for t in v[:4])
        ang = np.arctan2(v[5], v[4])
        half = ang if defect == "half angle dropped" else ang / np.float32(2.0)
        th = half if defect == "angle sign flipped" else -half
        self.cs, self.sn = float(np.cos(np.float32(th))), float(np.sin(np.float32(th)))
        self.exact_trig = bool(v[5] == 0 and not np.signbit(v[5]) and v[4] > 0)
        d_th = 0.0 if self.exact_trig else TRIG_ULPS * ulp32(float(ang)) / 2
        self.d_c = 0.0 if self.exact_trig else d_th + TRIG_ULPS * 2.0 ** -23
        plus = 0.0 if defect == "box without the +1" else 1.0
        r = float(max(a, b)) + plus
        self.x0, self.x1 = int(max(0.0, math.floor(self.cx - r))), int(min(float(nx), math.ceil(self.cx + r) + plus))
        self.y0, self.y1 = int(max(0.0, math.floor(self.cy - r))), int(min(float(ny), math.ceil(self.cy + r) + plus))
        if self.x1 <= self.x0 or self.y1 <= self.y0:
            self.active = False
        self.nx, self.ny = nx, ny

    def field(self):
        """(p, q, dx, dy) float64 over the ellipse's own box"""
        xs, ys = np.meshgrid(np.arange(self.x0, self.x1, dtype=np.float64), np.arange(self.y0, self.y1, dtype=np.float64))
        dx, dy = xs - self.cx, ys - self.cy
        u, w = dx * self.cs + dy * self.sn, -dx * self.sn + dy * self.cs
        return u / self.a, w / self.b, dx, dy

    def raster(self, strict=False):
        img = np.zeros((self.ny, self.nx), bool)
        if self.active:
            p, q, _, _ = self.field()
            f = p * p + q * q
            img[self.y0:self.y1, self.x0:self.x1] = f < 1.0 if strict else f <= 1.0
        return img

    def unsafe_pixels(self):
        """(pixels within the margin that are no exact ties, exact ties, largest margin among the pixels with 0.5 < f < 1.5)"""
        if not self.active:
            return 0, 0, 0.0
        p, q, dx, dy = self.field()
        d_u = (np.abs(dx) + np.abs(dy)) * (self.d_c + 4 * 2.0 ** -53)
        d_p, d_q = d_u / self.a, d_u / self.b
        f = p * p + q * q
        margin = 2 * np.abs(p) * d_p + 2 * np.abs(q) * d_q + d_p ** 2 + d_q ** 2 + 2.0 ** -48 * (1 + f)
        near = np.abs(f - 1.0) <= margin
        tie = near & self.exact_trig & (((np.abs(p) == 1) & (q == 0)) | ((p == 0) & (np.abs(q) == 1)))
        ring = np.abs(f - 1.0) < 0.5
        return int((near & ~tie).sum()), int(tie.sum()), float(margin[ring].max()) if ring.any() else 0.0


def union_box(ep, et, defect=None):
    if ep.active and et.active and defect != "union box from one ellipse only":
        return min(ep.x0, et.x0), max(ep.x1, et.x1), min(ep.y0, et.y0), max(ep.y1, et.y1)
    e = ep if ep.active else et
    return e.x0, e.x1, e.y0, e.y1


def iou_counts(rp, rt, nx, ny, defect=None):
    """(ti, tu) of one pair, or None where the true slot is empty (noobj > 0.99)"""
    assert defect is None or defect in DEFECTS_IOU
    if np.float32(rt[6]) > np.float32(0.99):
        return None
    ep, et = Ellipse(rp, nx, ny, defect), Ellipse(rt, nx, ny, defect)
    if not (ep.active or et.active):
        return 0, 0
    strict = defect == "< instead of <="
    a, b = ep.raster(strict), et.raster(strict)
    x0, x1, y0, y1 = union_box(ep, et, defect)
    box = np.zeros((ny, nx), bool)
    box[y0:y1, x0:x1] = True
    return int((a & b & box).sum()), int(((a | b) & box).sum())


def iou_value(counts):
    if counts is None or counts == (0, 0):
        return -1.0
    return counts[0] / counts[1]                          # the kernel's (double)ti / (double)tu


def pair_safe(rp, rt, nx, ny):
    """(safe, exact ties, largest margin)"""
    bad = ties = 0
    margin = 0.0
    for e in (Ellipse(rp, nx, ny), Ellipse(rt, nx, ny)):
        n, t, m = e.unsafe_pixels()
        bad, ties, margin = bad + n, ties + t, max(margin, m)
    return bad == 0, ties, margin


def row(cx, cy, a, b, ang_deg, noobj=0.0):
    t = 2 * math.radians(ang_deg)
    return [cx, cy, a, b, math.cos(t), math.sin(t), noobj, 1.0]


def aligned(cx, cy, a, b, noobj=0.0):
    """sin2t = +0, cos2t = 1: the trig values are exact on every libm"""
    return [cx, cy, a, b, 1.0, 0.0, noobj, 1.0]


def _near(rs, r, shift=3.0, grow=0.1):
    p = list(r)
    p[0] += rs.randn() * shift
    p[1] += rs.randn() * shift
    p[2] *= 1 + rs.randn() * grow
    return p


def _slots512(rs):
    """(name, draw) for the 512 x 384 canvas: draw() gives a candidate (prediction, truth)"""
    u = rs.uniform
    small = lambda: row(u(20, 480), u(20, 360), u(2, 4.5), u(2, 4.5), u(0, 180))
    mid = lambda: row(u(30, 480), u(30, 350), u(15, 60), u(10, 40), u(0, 180))

    def with_noobj(r, v):
        return r[:6] + [v, 1.0]
    below_half = float(np.nextafter(np.float32(0.5), np.float32(0)))
    above_099 = float(np.nextafter(np.float32(0.99), np.float32(1)))
    t = [("box below 256 pixels", lambda: (lambda r: (_near(rs, r, 1.0), r))(small())),
         ("box no multiple of 256", lambda: (lambda r: (_near(rs, r), r))(mid())),
         ("opposite corners", lambda: (row(u(20, 40), u(20, 40), u(15, 30), u(10, 20), u(0, 180)), row(u(470, 490), u(345, 365), u(15, 30), u(10, 20), u(0, 180)))),
         ("circle", lambda: (lambda c, r: (row(c[0], c[1], r, r, u(0, 180)), row(c[0] + 1.5, c[1] - 2.25, r + 0.5, r + 0.5, 0.0)))((u(100, 400), u(100, 300)), u(8, 30))),
         ("one pixel", lambda: (row(100.1, 70.2, 0.4, 0.4, 0.0), row(u(98, 102), u(68, 72), u(3, 6), u(2, 5), u(0, 180)))),
         # integer centres and axes: the four axis ends are exact ties; 9 k^2 + 49 j^2 = 441 and k^2 + 4 j^2 = 64 have no other
         # integer solutions, so no other pixel centre lies on either outline
         ("aligned, with exact ties", lambda: (aligned(30.0, 20.0, 7.0, 3.0), aligned(32.0, 21.0, 8.0, 4.0))),
         ("prediction empty, IoU 0", lambda: (with_noobj(mid(), 0.6), mid())),
         ("truth outside the canvas, IoU 0", lambda: (mid(), row(u(100, 400), -200.5, u(15, 40), u(10, 30), u(0, 180)))),
         ("both empty, -1", lambda: (with_noobj(mid(), 0.7), row(900.5, u(30, 350), u(15, 40), u(10, 30), u(0, 180)))),
         ("true noobj 0.99", lambda: (mid(), with_noobj(mid(), 0.99))),
         ("true noobj just above 0.99", lambda: (mid(), with_noobj(mid(), above_099))),
         ("predicted noobj just below 0.5", lambda: (lambda r: (with_noobj(_near(rs, r), below_half), r))(mid())),
         ("predicted noobj 0.5", lambda: (lambda r: (with_noobj(_near(rs, r), 0.5), r))(mid())),
         ("a == 0", lambda: (lambda r: (r[:2] + [0.0] + r[3:], r))(mid())),
         ("a < 0", lambda: (lambda r: (r[:2] + [-3.0] + r[3:], r))(mid())),
         ("b == 0 in the truth", lambda: (lambda r: (r, r[:3] + [0.0] + r[4:]))(mid()))]
    return t


def _slots64(rs):
    u = rs.uniform
    pair = lambda cx, cy: (lambda r: (_near(rs, r, 1.5), r))(row(cx, cy, u(8, 14), u(5, 8), u(0, 180)))
    return [("left border", lambda: pair(u(2, 6), u(20, 28))), ("right border", lambda: pair(u(58, 63), u(20, 28))),
            ("top border", lambda: pair(u(25, 40), u(0, 4))), ("bottom border", lambda: pair(u(25, 40), u(44, 48))),
            ("corner", lambda: pair(u(59, 65), u(44, 49))), ("centres outside", lambda: pair(u(-5, -1), u(-4, 0))),
            ("wider than the canvas", lambda: (row(u(28, 36), u(20, 28), u(70, 95), u(50, 75), u(0, 180)), row(u(28, 36), u(20, 28), u(60, 85), u(12, 18), u(0, 180))))]


def _fill(slots, nx, ny, tries=400):
    names, pairs, rejected = [], [], 0
    for name, draw in slots:
        for _ in range(tries):
            rp, rt = draw()
            if pair_safe(rp, rt, nx, ny)[0]:
                names.append(name)
                pairs.append((rp, rt))
                break
            rejected += 1
        else:
            raise AssertionError("no boundary-safe pair for %r in %d draws" % (name, tries))
    return names, pairs, rejected


@functools.lru_cache(maxsize=1)
def iou_table():
    """dict canvas -> (nx, ny, names, yp float32 [n][8], yt, want float64 [n]); 'big' holds 1000 pairs (the named slots, then
    seeded random pairs), 'small' the border cases of a 64 x 48 canvas; 'rejected': how many candidates were dropped"""
    rs = np.random.RandomState(2024)
    out = {}
    names, pairs, rejected = _fill(_slots512(rs), 512, 384)
    u = rs.uniform
    rand = lambda: (lambda r: (_near(rs, r), r))(row(u(10, 500), u(10, 374), u(4, 50), u(3, 35), u(0, 180), 1.0 if u() < 0.2 else 0.0))
    n2, p2, r2 = _fill([("random %d" % k, rand) for k in range(1000 - len(pairs))], 512, 384)
    out["big"] = (512, 384, names + n2, pairs + p2)
    n3, p3, r3 = _fill(_slots64(rs), 64, 48)
    out["small"] = (64, 48, n3, p3)
    res = {"rejected": rejected + r2 + r3}
    for key, (nx, ny, nm, pr) in out.items():
        yp, yt = (np.array([p[k] for p in pr], np.float32) for k in (0, 1))
        want = np.array([iou_value(iou_counts(a, b, nx, ny)) for a, b in zip(yp, yt)], np.float64)
        for a in (yp, yt, want):
            a.setflags(write=False)
        res[key] = (nx, ny, nm, yp, yt, want)
    return res
