"""TEST INFRASTRUCTURE -- the ring-count mask rule (include/spnet_hip.h "Ring-count masks") restated with
Python integers, independently of spnet_amd/masks.py: math.cos / math.sin, round() (ties to even) and arbitrary-precision
ints (numpy object arrays hold Python ints; nothing here can overflow or round).

Small frames (up to WHOLE_FRAME pixels) test every pixel against every row.  Larger ones test a window of
max(a, b) * 1.01 + 4 pixels around the centre, far more generous than the kernel's culling box, so that a pixel the kernel
culled wrongly would still show.

assert_trig_safe is a condition on the INPUTS of a test, not a tolerance: device and host fp64 cos / sin may differ in the
last place, which changes c = rint(2^14 cos) only if 2^14 cos lies that close to a half-integer.  The guard fails for any
angle within 1e-6 of one (an ulp is 4e-12 here), so for the angles that pass, c and s are the same on every libm.
"""
import math

import numpy as np

WHOLE_FRAME = 1 << 16
LIMIT = 32768.0


def trig_pair(angle_deg):
    t = (-float(angle_deg)) * (math.pi / 180.0)
    return 16384.0 * math.cos(t), 16384.0 * math.sin(t)


def assert_trig_safe(angles, margin=1e-6):
    for ang in np.asarray(angles, np.float64).reshape(-1).tolist():
        if not math.isfinite(ang):
            continue                                            # such a row paints nothing: its trig is never used
        for v in trig_pair(ang):
            frac = abs(v - math.floor(v) - 0.5)
            assert frac > margin, "angle %r: 2^14 cos or sin = %r is within %g of a half-integer" % (ang, v, margin)


def value_of(rings):
    """The mask value of a finite ring count."""
    t = 10.0 * float(rings)
    if t >= 255.0:
        return 255
    if t <= 0.0:
        return 0
    return int(t)                                               # truncates


def quantise(row):
    cx, cy, a, b, ang, rings = (float(v) for v in row)
    if not all(math.isfinite(v) for v in (cx, cy, a, b, ang, rings)):
        return None
    if abs(cx) >= LIMIT or abs(cy) >= LIMIT or a >= LIMIT or b >= LIMIT:
        return None
    aq, bq = round(16.0 * a), round(16.0 * b)
    if aq <= 0 or bq <= 0:
        return None
    tc, ts = trig_pair(ang)
    return round(16.0 * cx), round(16.0 * cy), aq, bq, round(tc), round(ts), value_of(rings)


def paint(mask, row):
    q = quantise(row)
    if q is None:
        return
    cxq, cyq, aq, bq, c, s, value = q
    H, W = mask.shape
    x0, y0, x1, y1 = 0, 0, W, H
    if H * W > WHOLE_FRAME:
        r = int(max(float(row[2]), float(row[3])) * 1.01) + 4
        x0, x1 = max(0, int(math.floor(row[0])) - r), min(W, int(math.floor(row[0])) + r + 1)
        y0, y1 = max(0, int(math.floor(row[1])) - r), min(H, int(math.floor(row[1])) + r + 1)
    if x1 <= x0 or y1 <= y0:
        return
    dx = np.array([16 * x + 8 - cxq for x in range(x0, x1)], dtype=object)[None, :]
    dy = np.array([16 * y + 8 - cyq for y in range(y0, y1)], dtype=object)[:, None]
    u = dx * c + dy * s
    v = dy * c - dx * s
    lhs = (u * bq) ** 2 + (v * aq) ** 2
    inside = (lhs <= (aq * bq * 16384) ** 2).astype(bool)
    mask[y0:y1, x0:x1][inside] = value


def ring_masks(rows, count, H, W):
    """rows [B][K][6] (anything float() takes), count [B] -> uint8 [B,H,W]."""
    rows = np.asarray(rows, np.float64)
    B, K = rows.shape[:2]
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for k in range(min(max(int(count[b]), 0), K)):
            paint(out[b], rows[b, k])
    return out


def masks_of_labels(labels, H, W):
    """A list of label lists [[(cx, cy, a, b, angle, rings), ...], ...] -> uint8 [B,H,W]."""
    out = np.zeros((len(labels), H, W), np.uint8)
    for b, rows in enumerate(labels):
        for row in rows:
            paint(out[b], row)
    return out


def compare_counts(pred, truth, tol):
    """int64 [N,5]: bg_bg, hit, miss, pred_only, true_only per frame of two uint8 arrays [N, n]."""
    p, t = np.asarray(pred).astype(np.int64), np.asarray(truth).astype(np.int64)
    both, close = (p > 0) & (t > 0), np.abs(p - t) <= tol
    return np.stack([((p == 0) & (t == 0)).sum(1), (both & close).sum(1), (both & ~close).sum(1),
                     ((p > 0) & (t == 0)).sum(1), ((p == 0) & (t > 0)).sum(1)], 1)


# ----------------------------------------------------------------------------- the shared case table (G1 / C1)
Q = 20.0 / 2048.0                 # the augmentation's angle quantum
NAN, INF = float("nan"), float("inf")
TABLE_H, TABLE_W, TABLE_K = 40, 56, 4


def case_table():
    """[(name, rows (up to K), count or None = len(rows))] at 40 x 56, K = 4."""
    t = [("centred", [(28, 20, 12, 7, 30, 3)], None),
         ("crosses left", [(2, 20, 9, 5, 20, 2)], None),
         ("crosses right", [(54, 18, 9, 5, 160, 2)], None),
         ("crosses top", [(30, 1, 6, 10, 10, 4)], None),
         ("crosses bottom", [(25, 39, 6, 10, 100, 4)], None),
         ("crosses all four", [(28, 20, 30, 22, 0, 1)], None),
         ("wholly outside", [(120, 90, 10, 5, 30, 5)], None),
         ("centre outside, rim inside", [(-6, 20, 12, 6, 0, 6), (60, 44, 9, 9, 0, 7)], None),
         ("circle", [(28, 20, 9, 9, 33, 2.5)], None),
         ("a < b", [(28, 20, 5, 13, 20, 7.34)], None),
         ("half-pixel centre", [(20.5, 15.5, 8, 4, 45, 1)], None),
         ("sixteenth-pixel centre", [(20.0625, 15.9375, 8, 4, 135, 1)], None),
         ("one pixel", [(10.5, 7.5, 0.5, 0.5, 0, 11)], None),
         ("painter order", [(22, 18, 12, 8, 10, 1), (30, 20, 10, 6, 170, 2), (26, 22, 5, 9, 90, 3)], None),
         ("a zero erases", [(28, 20, 14, 9, 15, 4), (28, 20, 6, 4, 15, 0.05)], None),
         ("count 0", [(28, 20, 12, 7, 30, 3)], 0),
         ("count above K", [(28, 20, 12, 7, 30, 3), (10, 10, 5, 5, 0, 1), (40, 30, 5, 3, 1, 2), (45, 8, 6, 3, 179, 9)], 9),
         ("count below 0", [(28, 20, 12, 7, 30, 3)], -2),
         ("rows that paint nothing", [(NAN, 20, 12, 7, 30, 3), (28, 20, 0, 7, 30, 3), (28, 20, 12, -3, 30, 3),
                                      (1e12, 20, 12, 7, 30, 3)], None),
         ("more that paint nothing", [(28, INF, 12, 7, 30, 3), (28, 20, 12, 7, NAN, 3), (28, 20, 12, 7, 30, NAN),
                                      (28, 20, -INF, 7, 30, 3)], None),
         ("nothing, then something", [(28, 20, 40000, 7, 30, 3), (28, 20, 12, 7, 30, INF), (28, 20, 0.03, 7, 30, 3),
                                      (28, 20, 4, 7, 30, 3)], None)]
    for ang in (0, 1, 45, 90, 135, 179, 7 * Q, -3 * Q, 180 + 11 * Q):
        t.append(("angle %r" % (ang,), [(27, 19, 15, 6, ang, 2)], None))
    return t


def table_arrays():
    """The table as (names, rows float64 [B,K,6], count int32 [B])."""
    t = case_table()
    rows, count = np.zeros((len(t), TABLE_K, 6), np.float64), np.zeros(len(t), np.int32)
    for i, (_, r, c) in enumerate(t):
        rows[i, :len(r)] = np.asarray(r, np.float64)
        count[i] = len(r) if c is None else c
    return [n for n, _, _ in t], rows, count
