"""TEST INFRASTRUCTURE -- the tracking rule (include/spnet_hip.h "Antinode tracks") restated with Python
integers, sets and fractions, independently of spnet_amd/tracks.py: brute-force containment over EVERY pixel of the frame
(the quantisation is mask_ref's, itself independent of spnet_amd/masks.py), set intersections, fractions.Fraction for the
order, a plain walk along `next` for the chains.  Also the case table and the seeded sequence builders that
tests/test_tracks_cpu.py and tests/test_tracks_gpu.py share; oracle(case) is computed once per process.

Angles: every case uses angles that mask_ref.assert_trig_safe accepts (checked by the tests), so c and s are the same
integers on every libm and on the device.
"""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests.helpers import mask_ref as MR

NAN, INF = float("nan"), float("inf")
Q = MR.Q
Case = namedtuple("Case", "name H W K G iou_q rows count")       # rows float64 [N,K,6], count int64 [N]
Result = namedtuple("Result", "live area inter next prev track age")


# ----------------------------------------------------------------------------- the rule
def pixel_set(row, H, W):
    """frozenset of y * W + x over all pixels of the frame inside the row, or None for a row that is not live."""
    q = MR.quantise(row)
    if q is None:
        return None
    cxq, cyq, aq, bq, c, s, _ = q
    dx = np.array([16 * x + 8 - cxq for x in range(W)], dtype=object)[None, :]
    dy = np.array([16 * y + 8 - cyq for y in range(H)], dtype=object)[:, None]
    lhs = ((dx * c + dy * s) * bq) ** 2 + ((dy * c - dx * s) * aq) ** 2
    return frozenset(np.flatnonzero((lhs <= (aq * bq * 16384) ** 2).astype(bool).reshape(-1)).tolist())


def _best(cands, inter_of, area_self, area_of, iou_q):
    """The best eligible candidate (ascending order, so max() keeps the FIRST of equal ones), or None."""
    best, best_iou = None, None
    for m in cands:
        inter = inter_of(m)
        union = area_self + area_of(m) - inter
        if inter > 0 and 1024 * inter >= iou_q * union:
            iou = Fraction(inter, union)
            if best is None or iou > best_iou:
                best, best_iou = m, iou
    return best


def link(rows, count, H, W, G, iou_q):
    rows = np.asarray(rows, np.float64)
    N, K = rows.shape[:2]
    sets = [[pixel_set(rows[t, k], H, W) if k < min(max(int(count[t]), 0), K) else None for k in range(K)] for t in range(N)]
    live = np.array([[s is not None for s in fr] for fr in sets], bool).reshape(N, K)
    area = np.array([[len(s) if s is not None else 0 for s in fr] for fr in sets], np.int64).reshape(N, K)
    nxt, prv = np.full((N, K), -1, np.int64), np.full((N, K), -1, np.int64)
    inters = {}
    for d in range(1, G + 1):
        inter = np.zeros((max(N - d, 0), K, K), np.int64)
        for t in range(N - d):
            for i in range(K):
                for j in range(K):
                    if live[t, i] and live[t + d, j]:
                        inter[t, i, j] = len(sets[t][i] & sets[t + d][j])
        inters[d] = inter
        for t in range(N - d):
            F = [i for i in range(K) if live[t, i] and nxt[t, i] == -1]
            P = [j for j in range(K) if live[t + d, j] and prv[t + d, j] == -1]
            fwd = {i: _best(P, lambda j: int(inter[t, i, j]), int(area[t, i]), lambda j: int(area[t + d, j]), iou_q) for i in F}
            bwd = {j: _best(F, lambda i: int(inter[t, i, j]), int(area[t + d, j]), lambda i: int(area[t, i]), iou_q) for j in P}
            for i in F:
                j = fwd[i]
                if j is not None and bwd[j] == i:
                    nxt[t, i], prv[t + d, j] = (t + d) * K + j, t * K + i
    track, age = np.zeros((N, K), np.int64), np.zeros((N, K), np.int64)
    for head in range(N * K):
        if live.reshape(-1)[head] and prv.reshape(-1)[head] == -1:
            x, n = head, 0
            while x != -1:                                   # a plain walk along next
                track.reshape(-1)[x], age.reshape(-1)[x] = head + 1, n
                x, n = int(nxt.reshape(-1)[x]), n + 1
    return Result(live, area, inters, nxt, prv, track, age)


# ----------------------------------------------------------------------------- builders
def pack(frames, K, count=None):
    """A list (frames) of lists of rows -> (rows float64 [N,K,6], count int64 [N]); count: overrides per frame (None keeps
    len(rows))."""
    rows, cnt = np.zeros((len(frames), K, 6), np.float64), np.zeros(len(frames), np.int64)
    for t, fr in enumerate(frames):
        assert len(fr) <= K
        if fr:
            rows[t, :len(fr)] = np.asarray(fr, np.float64)
        cnt[t] = len(fr)
    if count is not None:
        for t, c in enumerate(count):
            if c is not None:
                cnt[t] = c
    return rows, cnt


def drift_sequence(seed, N, K, H, W, n_obj, step=2.0, p_absent=0.0, a_range=(4.0, 12.0)):
    """A seeded sequence: n_obj ellipses that drift `step` pixels a frame in a direction of their own (sixteenth-pixel
    positions, angles on the augmentation's quantum) and are absent from a frame with probability p_absent; the order of a
    frame's rows is shuffled, so a detection's index changes from frame to frame."""
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(0, W, n_obj), rng.uniform(0, H, n_obj)
    th = rng.uniform(0, 2 * np.pi, n_obj)
    a = rng.uniform(a_range[0], a_range[1], n_obj)
    b = a * rng.uniform(0.5, 1.0, n_obj)
    ang = Q * rng.randint(1, 18000, n_obj)
    rings = np.round(rng.uniform(0.5, 11.0, n_obj), 1)
    frames = []
    for t in range(N):
        fr = [(round(16 * (cx[o] + step * t * np.cos(th[o]))) / 16.0, round(16 * (cy[o] + step * t * np.sin(th[o]))) / 16.0,
               round(16 * a[o]) / 16.0, round(16 * b[o]) / 16.0, ang[o], rings[o] + 0.1 * t)
              for o in range(n_obj) if rng.uniform() >= p_absent]
        frames.append([fr[i] for i in rng.permutation(len(fr))])
    return pack(frames, K)


def _case(name, H, W, K, G, iou_q, frames, count=None):
    rows, cnt = pack(frames, K, count)
    return Case(name, H, W, K, G, iou_q, rows, cnt)


@functools.lru_cache(maxsize=None)
def cases():
    c = []
    E1, E2, E3 = (20, 20, 10, 6, 30, 2.0), (55, 30, 8, 8, 0, 3.5), (64, 16, 7, 4, 100, 5.0)
    c.append(_case("identical frames", 48, 80, 4, 1, 256, [[E1, E2, E3]] * 3))
    c.append(_case("one frame", 48, 80, 4, 1, 256, [[E1, E2, (NAN, 1, 1, 1, 0, 1)]]))
    c.append(_case("two frames", 17, 70, 4, 1, 256, [[(10, 8, 6, 4, 0, 1)], [(12, 9, 6, 4, 0, 2)]]))
    # a fixed step of 9 px a frame, entering over the left edge: the IoU of the clipped sets is 0.202, 0.484, 0.373 and from
    # then on, wholly inside, 0.363 (162 / 446) -- it falls through 379 / 1024 = 0.3701 between frames 3 and 4
    c.append(_case("drift across the threshold", 33, 130, 4, 1, 379, [[(-8 + 9 * t, 16, 12, 8, 0, 1 + t)] for t in range(9)]))
    c.append(_case("two that cross", 48, 80, 4, 1, 205,
                   [[(16 + 6 * t, 20, 7, 5, 0, 2.0), (64 - 6 * t, 26, 7, 5, 0, 6.0)] for t in range(9)]))
    flick = [[E1], [E1], [], [E1], [E1]]
    c.append(_case("flicker, gap 1", 48, 80, 4, 1, 256, flick))
    c.append(_case("flicker, gap 2", 48, 80, 4, 2, 256, flick))
    c.append(_case("flicker beside a free detection", 48, 80, 4, 2, 256, [[E1], [E1], [E2], [E1], [E1, E2]]))
    # mirror images about x = 40 (pixel centres at x + 0.5: pixel x maps to 79 - x): equal counts on both sides
    c.append(_case("exact tie", 48, 80, 4, 1, 102,
                   [[(40, 24, 8, 8, 0, 1)], [(35, 24, 8, 8, 0, 2), (45, 24, 8, 8, 0, 3)], [(40, 24, 8, 8, 0, 4)]]))
    # i = 0 has only j = 0 to prefer; j = 0 prefers i' = 1: no link for i in that pass
    c.append(_case("non-mutual best", 48, 80, 4, 1, 102, [[(30, 24, 8, 8, 0, 1), (44, 24, 8, 8, 0, 2)], [(40, 24, 8, 8, 0, 3)]]))
    # 16 x 64 = 1,024 pixels: an ellipse over the whole frame has area 1024, so IoU with a row inside it is n / 1024
    whole, small = (32, 8, 100, 100, 0, 1), (30.5, 7.5, 5, 4, 0, 2)
    n = len(pixel_set(small, 16, 64))
    assert len(pixel_set(whole, 16, 64)) == 1024 and 1 < n < 1023
    c.append(_case("exactly at the threshold", 16, 64, 4, 1, n, [[whole], [small]]))
    c.append(_case("one count below the threshold", 16, 64, 4, 1, n + 1, [[whole], [small]]))
    good, good2 = (30, 20, 9, 6, 45, 2.0), (60, 30, 6, 6, 0, 4.0)
    c.append(_case("dead rows", 48, 80, 4, 2, 256,
                   [[good, (NAN, 20, 9, 6, 45, 2), (30, 20, INF, 6, 45, 2), (30, 20, 0, 6, 45, 2)],
                    [good, (32768, 20, 9, 6, 45, 2), good2, good2],
                    [good, good2],
                    [good, good2, (30, 20, 9, 6, 45, NAN), (30, -32768, 9, 6, 45, 2)],
                    [good, good2, (30, 20, 9, -INF, 45, 2), (30, 20, 9, 0.03, 45, 2)]],
                   count=[None, 2, -3, 9, None]))
    c.append(_case("wholly outside the frame", 17, 70, 4, 2, 1, [[(200, 100, 10, 5, 30, 5), (-40, -40, 6, 6, 0, 1)]] * 3))
    c.append(_case("clipped by each edge", 33, 130, 4, 1, 256,
                   [[(2 + t, 16, 9, 5, 20, 2), (127 - t, 14, 9, 5, 160, 3), (60, 1 + t, 6, 10, 10, 4), (70, 31 - t, 6, 10, 100, 5)]
                    for t in range(3)]))
    c.append(_case("covers the whole frame", 17, 70, 4, 1, 1024, [[(35, 8, 200, 200, 0, 1)], [(30, 9, 150, 220, 45, 1)]]))
    rng = np.random.RandomState(5)
    pile = [[(round(16 * rng.uniform(24, 40)) / 16.0, round(16 * rng.uniform(4, 12)) / 16.0, round(16 * rng.uniform(2, 30)) / 16.0,
              round(16 * rng.uniform(2, 12)) / 16.0, Q * rng.randint(1, 18000), 1.0 + k % 9) for k in range(128)] for _ in range(2)]
    c.append(_case("128 rows piled on one tile", 16, 64, 128, 1, 256, pile))
    c.append(_case("one chain through 40 frames", 16, 64, 4, 1, 256,
                   [[(10 + t, 8, 6, 5, 0, 1 + 0.1 * t)] + ([(50, 8, 4, 4, 0, 2)] if t % 7 == 3 else []) for t in range(40)]))
    c.append(_case("one chain through 33 frames", 17, 70, 4, 2, 256,
                   [([(60, 8, 3, 3, 0, 2)] if t % 5 == 1 else []) + [(10 + t, 8, 6, 5, 0, 1)] for t in range(33)]))
    r, n_ = drift_sequence(7, 3, 72, 48, 80, 72, step=1.5, p_absent=0.1, a_range=(3.0, 9.0))
    c.append(Case("72 rows a frame, gap 3", 48, 80, 72, 3, 205, r, n_))
    r, n_ = drift_sequence(9, 9, 4, 33, 130, 4, step=2.5, p_absent=0.3)
    c.append(Case("seeded flicker, gap 4", 33, 130, 4, 4, 154, r, n_))
    r, n_ = drift_sequence(11, 9, 4, 17, 70, 4, step=1.0, p_absent=0.2, a_range=(3.0, 8.0))
    c.append(Case("seeded flicker, gap 3", 17, 70, 4, 3, 307, r, n_))
    return tuple(c)


def case_named(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def oracle(index):
    """link() of cases()[index], computed once and shared; the arrays are read-only."""
    c = cases()[index]
    res = link(c.rows, c.count, c.H, c.W, c.G, c.iou_q)
    for a in (res.live, res.area, res.next, res.prev, res.track, res.age) + tuple(res.inter.values()):
        a.setflags(write=False)
    return res
