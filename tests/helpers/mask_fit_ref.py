"""TEST INFRASTRUCTURE -- the mask-fitting rule (include/spnet_hip.h "Mask fitting") restated as a plain flood
fill with Python integers, independently of spnet_amd/masks.py (no run lengths, no union-find, no scipy), and the case
tables that tests/test_mask_fit_cpu.py and tests/test_mask_fit_gpu.py share.

Adjacent: 8-neighbours, both nonzero, |v - w| <= join_tol.  Label: 1 + (y W + x) of the component's first pixel in raster
order (the fill starts from exactly that pixel, because the frame is scanned in raster order).  Sums: (n, sum x, sum y,
sum x^2, sum y^2, sum xy, sum v, first) as Python ints.

The border cases sit on the borders of the kernels' 64 x 16 tile: x = 63 | 64 and y = 15 | 16 on a 33 x 130 frame."""
import functools

import numpy as np

NEIGHBOURS = ((-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1))
TILE_W, TILE_H = 64, 16


def fill_frame(mask, join_tol):
    """(labels int32 [H,W], [sums of every component, in label order]) of one frame."""
    H, W = mask.shape
    m = mask.astype(np.int64).tolist()
    labels = [[0] * W for _ in range(H)]
    comps = []
    for y0 in range(H):
        for x0 in range(W):
            if m[y0][x0] == 0 or labels[y0][x0]:
                continue
            first = y0 * W + x0
            labels[y0][x0] = first + 1
            stack = [(x0, y0)]
            n = sx = sy = sxx = syy = sxy = sv = 0
            while stack:
                x, y = stack.pop()
                v = m[y][x]
                n += 1; sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y; sv += v
                for dx, dy in NEIGHBOURS:
                    xx, yy = x + dx, y + dy
                    if 0 <= xx < W and 0 <= yy < H and m[yy][xx] != 0 and not labels[yy][xx] and abs(m[yy][xx] - v) <= join_tol:
                        labels[yy][xx] = first + 1
                        stack.append((xx, yy))
            comps.append((n, sx, sy, sxx, syy, sxy, sv, first))
    return np.asarray(labels, np.int32).reshape(H, W), comps


def fill(masks, join_tol):
    """(labels int32 [B,H,W], per frame the list of its components' sums)."""
    got = [fill_frame(f, join_tol) for f in masks]
    return np.stack([g[0] for g in got]), [g[1] for g in got]


def packed(comps, C):
    """(n_components int32 [B], sums int64 [B,C,8]) as spnet_mask_moments writes them: the true count, the first C."""
    n = np.asarray([len(c) for c in comps], np.int32)
    sums = np.zeros((len(comps), C, 8), np.int64)
    for b, c in enumerate(comps):
        for k, s in enumerate(c[:C]):
            sums[b, k] = s                                   # Python ints: an overflow would raise
    return n, sums


# ----------------------------------------------------------------------------- the cases
class Case:
    def __init__(self, name, masks, join_tol=0, C=128, n=None, label_at=None, sv=None):
        masks = np.asarray(masks, np.uint8)
        self.name, self.masks = name, masks[None] if masks.ndim == 2 else masks
        self.join_tol, self.C = join_tol, C
        self.n = n                      # expected component counts, by construction (a list per frame), or None
        self.label_at = label_at        # ((b, y, x), label) known by construction, or None
        self.sv = sv                    # expected sum of values of frame 0's first component, or None

    def __repr__(self):
        return self.name


def _blocky(H, W, seed):
    rng = np.random.RandomState(seed)
    coarse = rng.choice(np.asarray([0, 10, 20], np.uint8), size=((H + 2) // 3, (W + 4) // 5), p=[0.5, 0.25, 0.25])
    return np.kron(coarse, np.ones((3, 5), np.uint8))[:H, :W]


def _frame(H=33, W=130):
    return np.zeros((H, W), np.uint8)


def _serpentine(H, W):
    m = _frame(H, W)
    m[0::2, :] = 60
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 60
    return m


def _spiral(H, W):
    m = _frame(H, W)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 70
    while True:
        moved = False
        while True:
            nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
            if not (0 <= nx < W and 0 <= ny < H) or m[ny, nx]:
                break
            if 0 <= fx < W and 0 <= fy < H and m[fy, fx]:
                break
            x, y = nx, ny
            m[y, x] = 70
            moved = True
        if not moved:
            return m
        dx, dy = -dy, dx


def _build_cases():
    cases = []
    add = lambda *a, **k: cases.append(Case(*a, **k))
    # sizes
    add("1x1", np.full((1, 1), 7), n=[1], label_at=((0, 0, 0), 1))
    add("1x200", _blocky(1, 200, 1))
    add("200x1", _blocky(200, 1, 2))
    add("16x64 one tile", _blocky(16, 64, 3))
    add("33x130", _blocky(33, 130, 4))
    add("33x130 tol 10", _blocky(33, 130, 4), join_tol=10)
    # empty and full
    add("empty", _frame(), n=[0])
    add("full", np.full((33, 130), 30), n=[1], label_at=((0, 32, 129), 1), sv=30 * 33 * 130)
    # a background column between two blobs of one value
    for gap in (63, 64, 65):
        m = _frame()
        m[2:31, 40:91] = 20
        m[:, gap] = 0
        add("gap at x = %d" % gap, m, n=[2], label_at=((0, 30, 90), 1 + 2 * 130 + gap + 1))
    # diagonal-only contact across a tile corner
    m = _frame(); m[15, 63] = m[16, 64] = 50
    add("diagonal", m, n=[1], label_at=((0, 16, 64), 1 + 15 * 130 + 63), sv=100)
    m = _frame(); m[15, 64] = m[16, 63] = 50
    add("anti-diagonal", m, n=[1], label_at=((0, 16, 63), 1 + 15 * 130 + 64), sv=100)
    # two values touching along a tile border: |v1 - v2| = 7
    mv = _frame(); mv[2:31, 40:64] = 20; mv[2:31, 64:91] = 27
    mh = _frame(); mh[5:16, 10:120] = 27; mh[16:26, 10:120] = 20
    for name, m in (("vertical", mv), ("horizontal", mh)):
        add("touch %s tol 0" % name, m, join_tol=0, n=[2])
        add("touch %s tol 7" % name, m, join_tol=7, n=[1])
        add("touch %s tol 6" % name, m, join_tol=6, n=[2])
    # 10, 14, 18 in a chain, across two borders
    m = _frame(); m[14:18, 60:64] = 10; m[14:18, 64:128] = 14; m[14:18, 128:130] = 18
    add("chain tol 4", m, join_tol=4, n=[1], sv=4 * (4 * 10 + 64 * 14 + 2 * 18), label_at=((0, 17, 129), 1 + 14 * 130 + 60))
    add("chain tol 3", m, join_tol=3, n=[3])
    # long merge chains over every tile of 48 x 192
    add("serpentine", _serpentine(48, 192), n=[1], label_at=((0, 46, 100), 1))
    add("spiral", _spiral(48, 192), n=[1], label_at=((0, 47, 0), 1))
    m = _frame(48, 192); m[3:48, 100] = 80; m[1:48, 150] = 80; m[47, 100:151] = 80
    add("U", m, n=[1], label_at=((0, 3, 100), 1 + 1 * 192 + 150))
    # checkerboards
    yy, xx = np.mgrid[0:33, 0:130]
    add("checkerboard", np.where((xx + yy) % 2 == 0, 40, 0), n=[1], label_at=((0, 32, 128), 1))
    add("checkerboard two values", np.where((xx + yy) % 2 == 0, 40, 50), n=[2], label_at=((0, 32, 129), 2))
    # the cap: 130 isolated pixels, C = 128
    m = _frame()
    for i in range(130):
        m[2 * (i // 65), 2 * (i % 65)] = 1 + i
    add("cap", m, C=128, n=[130])
    add("cap C = 1", m, C=1, n=[130])
    # batch independence
    m = np.zeros((3, 16, 64), np.uint8); m[0, 15, :] = 9; m[1, 0, :] = 9
    add("batch", m, n=[1, 1, 0], label_at=((1, 0, 63), 1))
    # wide accumulators
    add("wide", np.full((1, 16384), 255), n=[1], sv=255 * 16384)
    # seeded noise
    noise = np.random.RandomState(5).choice(np.asarray([0, 10, 20, 30], np.uint8), size=(4, 33, 130), p=[0.5, 1 / 6, 1 / 6, 1 / 6])
    add("noise tol 0", noise, join_tol=0)
    add("noise tol 10", noise, join_tol=10)
    return cases


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_build_cases())


@functools.lru_cache(maxsize=None)
def expected(index):
    """(labels, comps) of case `index`, computed once."""
    c = cases()[index]
    labels, comps = fill(c.masks, c.join_tol)
    labels.setflags(write=False)
    return labels, comps


def case_ids():
    return [c.name for c in cases()]


def check_construction(index):
    """What a case promises by construction holds in the oracle's answer (a check of the case table and of the oracle)."""
    c = cases()[index]
    labels, comps = expected(index)
    if c.n is not None:
        assert [len(f) for f in comps] == list(c.n), c.name
    if c.label_at is not None:
        (b, y, x), want = c.label_at
        assert labels[b, y, x] == want, (c.name, labels[b, y, x], want)
    if c.sv is not None:
        assert comps[0][0][6] == c.sv, c.name


# ----------------------------------------------------------------------------- the full-size case
FULL_H, FULL_W, FULL_B, FULL_CELL = 384, 512, 4, 128


def fullsize_rows(seed=2026):
    """rows float64 [4,12,6], count [4]: one ellipse per 128 x 128 cell, a in [6, 56], b in [4, a], the centre such that the
    ellipse keeps 2 pixels from its cell's edge, angle in (-90, 90), rings 1 .. 11 (whole numbers)."""
    rng = np.random.RandomState(seed)
    rows = np.zeros((FULL_B, 12, 6), np.float64)
    for f in range(FULL_B):
        k = 0
        for cy0 in range(0, FULL_H, FULL_CELL):
            for cx0 in range(0, FULL_W, FULL_CELL):
                a = rng.uniform(6.0, 56.0)
                b = rng.uniform(4.0, a)
                cx = rng.uniform(cx0 + a + 2.0, cx0 + FULL_CELL - a - 2.0)
                cy = rng.uniform(cy0 + a + 2.0, cy0 + FULL_CELL - a - 2.0)
                ang = rng.uniform(-89.999, 89.999)
                rows[f, k] = (cx, cy, a, b, ang, float(rng.randint(1, 12)))
                k += 1
    return rows, np.full(FULL_B, 12, np.int32)


def roundtrip_errors(rows, count, fit_rows, fit_count, min_axis_gap=4.0):
    """Worst errors of a fit against the painted rows: (centre px, axes px, angle deg, share of rows whose angle was
    compared).  Fitted rows come in raster order of their first pixel, painted rows in any order: they are matched by the
    nearest centre.  Painted a < b is canonicalised (swap, + 90 deg); angles are compared modulo 180 and only where
    a - b >= min_axis_gap."""
    e_c = e_ax = e_ang = 0.0
    n_ang = n_all = 0
    for f in range(rows.shape[0]):
        assert fit_count[f] == count[f], (f, fit_count[f], count[f])
        fit = fit_rows[f, :fit_count[f]]
        for cx, cy, a, b, ang, rings in rows[f, :count[f]]:
            if a < b:
                a, b, ang = b, a, ang + 90.0
            g = fit[np.argmin((fit[:, 0] - cx) ** 2 + (fit[:, 1] - cy) ** 2)]
            assert g[5] == rings, (f, g[5], rings)
            e_c = max(e_c, float(np.hypot(g[0] - cx, g[1] - cy)))
            e_ax = max(e_ax, abs(g[2] - a), abs(g[3] - b))
            n_all += 1
            if a - b >= min_axis_gap:
                d = (g[4] - ang) % 180.0
                e_ang = max(e_ang, min(d, 180.0 - d))
                n_ang += 1
    return e_c, e_ax, e_ang, n_ang / max(n_all, 1)
