"""TEST INFRASTRUCTURE -- two oracles, independent of spnet_amd:

the tracking score (include/spnet_hip.h "Tracking score") restated with Python sets and fractions.Fraction --
the pixel sets are tests/helpers/tracks_ref.py's brute-force ones, the mutual best is a max over Fractions, the identity
statistics a plain walk over the frames -- and the strike rule (include/spnet_hip.h "Strike sequences") in plain Python
integers, one slot at a time.  Also the case table tests/test_track_score_cpu.py and tests/test_track_score_gpu.py share;
oracle(index) is computed once per process."""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests.helpers import tracks_ref as TR

NAN = float("nan")
Case = namedtuple("Case", "name H W iou_q M rows_t count_t ident rows_p count_p track")
Result = namedtuple("Result", "match frame_counts ident_stats")
M32 = 0xFFFFFFFF


# ----------------------------------------------------------------------------- the score
def _best(cands, inter_of, area_self, area_of, iou_q):
    best, best_iou = None, None
    for m in cands:                                              # ascending: the first of equal ones stays
        inter = inter_of(m)
        union = area_self + area_of(m) - inter
        if inter > 0 and 1024 * inter >= iou_q * union:
            iou = Fraction(inter, union)
            if best is None or iou > best_iou:
                best, best_iou = m, iou
    return best


def score(rows_t, count_t, ident, rows_p, count_p, track, H, W, iou_q, M):
    rows_t, rows_p = np.asarray(rows_t, np.float64), np.asarray(rows_p, np.float64)
    N, Kt, Kp = rows_t.shape[0], rows_t.shape[1], rows_p.shape[1]

    def sets(rows, count, K):
        return [[TR.pixel_set(rows[n, k], H, W) if k < min(max(int(count[n]), 0), K) else None for k in range(K)]
                for n in range(N)]
    St, Sp = sets(rows_t, count_t, Kt), sets(rows_p, count_p, Kp)
    match = np.full((N, Kt), -1, np.int64)
    counts = np.zeros((N, 3), np.int64)
    stats = [[0, 0, 0, 0, -1] for _ in range(M + 1)]
    stats[0][4] = 0
    last, gap = {}, {}
    for n in range(N):
        seen, T = set(), []
        for i in range(Kt):
            g = int(ident[n][i])
            if St[n][i] is not None and 1 <= g <= M and g not in seen:
                seen.add(g)
                T.append(i)
        P = [j for j in range(Kp) if Sp[n][j] is not None and int(track[n][j]) > 0]
        fwd = {i: _best(P, lambda j: len(St[n][i] & Sp[n][j]), len(St[n][i]), lambda j: len(Sp[n][j]), iou_q) for i in T}
        bwd = {j: _best(T, lambda i: len(St[n][i] & Sp[n][j]), len(Sp[n][j]), lambda i: len(St[n][i]), iou_q) for j in P}
        for i in T:
            j = fwd[i]
            if j is not None and bwd[j] == i:
                match[n, i] = j
        tp = int((match[n] >= 0).sum())
        counts[n] = (tp, len(T) - tp, len(P) - tp)
        for i in T:
            g, s = int(ident[n][i]), stats[int(ident[n][i])]
            s[0] += 1
            if match[n, i] < 0:
                gap[g] = s[1] > 0
                continue
            tr = int(track[n][match[n, i]])
            if s[1] > 0 and tr != last[g]:
                s[2] += 1
            if gap.get(g):
                s[3] += 1
            if s[1] == 0:
                s[4] = n
            s[1] += 1
            last[g], gap[g] = tr, False
    return Result(match, counts, np.asarray(stats, np.int64))


def _case(name, H, W, iou_q, M, truth, pred, Kt=4, Kp=4, count_t=None, count_p=None):
    """truth: per frame a list of (row, ident); pred: per frame a list of (row, track)."""
    rows_t, ct = TR.pack([[r for r, _ in fr] for fr in truth], Kt, count_t)
    rows_p, cp = TR.pack([[r for r, _ in fr] for fr in pred], Kp, count_p)
    ident, track = np.zeros((len(truth), Kt), np.int64), np.zeros((len(pred), Kp), np.int64)
    for n, fr in enumerate(truth):
        ident[n, :len(fr)] = [g for _, g in fr]
    for n, fr in enumerate(pred):
        track[n, :len(fr)] = [g for _, g in fr]
    return Case(name, H, W, iou_q, M, rows_t, ct, ident, rows_p, cp, track)


@functools.lru_cache(maxsize=None)
def cases():
    c = []
    E1, E2, E3 = (20, 20, 10, 6, 30, 2.0), (55, 30, 8, 8, 0, 3.5), (64, 16, 7, 4, 100, 5.0)
    E1s = (22, 21, 10, 6, 30, 2.5)
    c.append(_case("an empty frame", 48, 80, 256, 3, [[(E1, 1)], [], [(E1, 1)]], [[(E1s, 5)], [], [(E1s, 5)]]))
    c.append(_case("truth only", 48, 80, 256, 3, [[(E1, 1), (E2, 2)]] * 2, [[], []]))
    c.append(_case("prediction only", 48, 80, 256, 3, [[], []], [[(E1, 1), (E2, 2)]] * 2))
    # mirror images about x = 40: equal counts on both sides; once two predictions on one truth, once two truths on one
    c.append(_case("exact tie, two predictions", 48, 80, 102, 2,
                   [[((40, 24, 8, 8, 0, 1), 1)]], [[((35, 24, 8, 8, 0, 2), 7), ((45, 24, 8, 8, 0, 3), 8)]]))
    c.append(_case("exact tie, two truths", 48, 80, 102, 2,
                   [[((35, 24, 8, 8, 0, 2), 1), ((45, 24, 8, 8, 0, 3), 2)]], [[((40, 24, 8, 8, 0, 1), 7)]]))
    whole, small = (32, 8, 100, 100, 0, 1), (30.5, 7.5, 5, 4, 0, 2)
    n = len(TR.pixel_set(small, 16, 64))
    c.append(_case("exactly at iou_q", 16, 64, n, 1, [[(whole, 1)]], [[(small, 3)]]))
    c.append(_case("one count below iou_q", 16, 64, n + 1, 1, [[(whole, 1)]], [[(small, 3)]]))
    c.append(_case("two predictions on one truth", 48, 80, 205, 2, [[(E1, 1)]] * 2,
                   [[((26, 22, 10, 6, 30, 1), 4), (E1s, 9)], [(E1s, 9), ((26, 22, 10, 6, 30, 1), 4)]]))
    c.append(_case("non-mutual best", 48, 80, 102, 2, [[((30, 24, 8, 8, 0, 1), 1), ((44, 24, 8, 8, 0, 2), 2)]],
                   [[((40, 24, 8, 8, 0, 3), 6)]]))
    c.append(_case("an identity switch", 48, 80, 256, 2, [[(E1, 1), (E2, 2)]] * 5,
                   [[(E1s, 11), (E2, 12)], [(E1s, 11), (E2, 12)], [(E1s, 31), (E2, 12)], [(E1s, 31), (E2, 12)],
                    [(E1s, 11), (E2, 12)]]))
    c.append(_case("a fragment without a switch", 48, 80, 256, 2, [[(E1, 1), (E2, 2)]] * 6,
                   [[(E2, 12)], [(E1s, 11), (E2, 12)], [(E2, 12)], [(E2, 12)], [(E1s, 11)], [(E1s, 11), (E2, 12)]]))
    c.append(_case("a fragment with a switch", 48, 80, 256, 2, [[(E1, 1)]] * 4, [[(E1s, 11)], [], [(E1s, 21)], [(E1s, 21)]]))
    c.append(_case("a duplicate identity in a frame", 48, 80, 256, 3, [[(E2, 2), (E1, 2), (E3, 3)], [(E1, 2), (E2, 2)]],
                   [[(E1s, 11), (E2, 12), (E3, 13)]] * 2))
    c.append(_case("a duplicate behind a dead row", 48, 80, 256, 3, [[((NAN, 1, 1, 1, 0, 1), 2), (E1, 2), (E2, 2)]],
                   [[(E1s, 11), (E2, 12)]]))
    c.append(_case("ident above M and below 1", 48, 80, 256, 2, [[(E1, 3), (E2, 2), (E3, -1), (E3, 65537)]] * 2,
                   [[(E1s, 11), (E2, 12), (E3, 13)]] * 2))
    c.append(_case("track <= 0", 48, 80, 256, 2, [[(E1, 1), (E2, 2)]] * 2,
                   [[(E1s, 0), (E2, 12)], [(E1s, -7), (E2, -2147483648)]]))
    c.append(_case("count above K and below 0", 48, 80, 256, 4, [[(E1, 1), (E2, 2), (E3, 3), (E1s, 4)]] * 3,
                   [[(E1s, 11), (E2, 12), (E3, 13), (E3, 14)]] * 3, count_t=[9, -3, 2], count_p=[1000, 2, -1]))
    c.append(_case("Kt 2, Kp 7", 17, 65, 256, 7, [[((20, 8, 9, 5, 0, 1), 7), ((50, 8, 6, 6, 0, 2), 1)]] * 2,
                   [[((51, 9, 6, 6, 0, 2), 3), ((60, 3, 2, 2, 0, 1), 4), ((21, 8, 9, 5, 0, 1.5), 5)]] * 2, Kt=2, Kp=7))
    c.append(_case("Kt 1, Kp 2, one frame", 16, 64, 256, 1, [[((20, 8, 9, 5, 0, 1), 1)]],
                   [[((60, 3, 2, 2, 0, 1), 4), ((21, 8, 9, 5, 0, 1.5), 5)]], Kt=1, Kp=2))
    # one ellipse over the corner of four 64 x 16 tiles, one partly outside the frame
    c.append(_case("straddles four tiles", 48, 130, 256, 2, [[((64, 16, 12, 9, 40, 3), 1), ((128, 46, 9, 6, 20, 2), 2)]] * 2,
                   [[((127, 45, 9, 6, 20, 2.5), 5), ((63, 17, 12, 9, 40, 3.5), 6)]] * 2))
    # 9 frames of a seeded drift on each side, shuffled rows, absences: every statistic moves
    rt, ct = TR.drift_sequence(21, 9, 7, 48, 130, 5, step=1.0, p_absent=0.15, a_range=(5.0, 10.0))
    rp, cp = TR.drift_sequence(21, 9, 128, 48, 130, 5, step=1.0, p_absent=0.15, a_range=(5.0, 10.0))
    rng = np.random.RandomState(3)
    c.append(Case("seeded, Kt 7, Kp 128", 48, 130, 205, 7, rt, ct, rng.randint(0, 8, (9, 7)), rp, cp, rng.randint(0, 4, (9, 128))))
    rt, ct = TR.drift_sequence(22, 2, 128, 17, 65, 100, step=1.0, a_range=(2.0, 6.0))
    rp, cp = TR.drift_sequence(23, 2, 7, 17, 65, 7, step=1.0, a_range=(2.0, 6.0))
    c.append(Case("seeded, Kt 128, Kp 7, M 65536", 17, 65, 102, 65536, rt, ct,
                  np.where(rng.uniform(size=(2, 128)) < 0.2, 65536, rng.randint(1, 40, (2, 128))), rp, cp, rng.randint(0, 3, (2, 7))))
    return tuple(c)


def case_named(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def oracle(index):
    c = cases()[index]
    res = score(c.rows_t, c.count_t, c.ident, c.rows_p, c.count_p, c.track, c.H, c.W, c.iou_q, c.M)
    for a in res:
        a.setflags(write=False)
    return res


# ----------------------------------------------------------------------------- the strike rule
def mix(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7feb352d) & M32
    x ^= x >> 15
    x = (x * 0x846ca68b) & M32
    return x ^ (x >> 16)


def draw(key, k):
    return mix(key ^ ((k * 0x85ebca6b + 0xc2b2ae35) & M32))


def randint(u, lo, hi):
    return lo + ((u * max(hi - lo + 1, 1)) >> 32)


def envelope(t, onset, rise, hold, decay):
    if t < onset:
        return 0
    peak = onset + rise
    if t < peak:
        return 256 * (t - onset + 1) // (rise + 1)
    after = peak + hold + 1
    if t < after:
        return 256
    return max(256 - 256 * (t - after + 1) // (decay + 1), 0)


def strike(waves0, nodes0, nnode0, T, seed, J, first_sequence=0, frames=None):
    """The strike rule slot by slot: (waves, nodes, nnode, ident) as nested Python lists of the frames `frames` (a list of
    (s, t); default all, sequence-major).  Floats appear only as base values carried over and as whole numbers."""
    S = len(nodes0)
    frames = [(s, t) for s in range(S) for t in range(T)] if frames is None else frames
    W, Nd, Nn, Id = [], [], [], []
    for s, t in frames:
        g = first_sequence + s
        skey = mix(mix((mix((seed & M32) ^ 0x51ed270b) + (g & M32)) & M32) ^ (g >> 32))
        nn = min(max(int(nnode0[s]), 0), 7)
        valid = [j < nn and float(nodes0[s][j][7]) != 0.0 for j in range(7)]
        struck = valid.index(True) if True in valid else 7
        fr, ids = [], []
        for j in range(7):
            rings = 0
            if valid[j]:
                ek = mix((skey + j) & M32)
                onset = 0 if j == struck else randint(draw(ek, 0), 0, T // 2)
                rise = 0 if j == struck else randint(draw(ek, 1), 1, max(T // 4, 1))
                hold, decay = randint(draw(ek, 2), 0, T // 4), randint(draw(ek, 3), 1, T)
                R = float(nodes0[s][j][5])
                R = 0 if R != R else int(min(max(R, 0.0), 255.0))
                rings = (R * envelope(t, onset, rise, hold, decay) + 128) >> 8
            if rings >= 1:
                jk = mix((skey + (((j + 1) << 12) | t)) & M32)
                b = [float(v) for v in nodes0[s][j]]
                fr.append([b[0] + randint(draw(jk, 0), -J, J), b[1] + randint(draw(jk, 1), -J, J), b[2], b[3], b[4],
                           float(rings), b[6], 1.0])
                ids.append(1 + 7 * g + j)
            else:
                fr.append([0.0] * 8)
                ids.append(0)
        W.append([float(v) for v in waves0[s][:5]])
        Nd.append(fr)
        Nn.append(nn)
        Id.append(ids)
    return W, Nd, Nn, Id


def base_params(S, seed, H=384, W=512):
    """Seeded frame-0 parameters in spnet_fake_espi_params' layout WITHOUT the device: non-overlapping ellipses on a grid of
    cells, whole numbers, 1 .. 7 a sequence with a hole now and then (valid = 0) and one hostile sequence at the end."""
    rng = np.random.RandomState(seed)
    waves = np.stack([rng.randint(10, 200, S), rng.randint(W // 8, W // 2, S), rng.randint(15, 40, S),
                      3 * (rng.randint(0, 1 << 24, S) * 2.0 ** -24 - 0.5), rng.randint(H // 8, H // 3, S)], 1).astype(np.float32)
    nodes, nnode = np.zeros((S, 7, 8), np.float32), np.zeros(S, np.int32)
    for s in range(S):
        n = rng.randint(1, 8)
        cells = rng.permutation(12)[:n]
        for j, cell in enumerate(cells):
            cx, cy = (cell % 4) * (W // 4) + W // 8, (cell // 4) * (H // 3) + H // 6
            m = min(W // 8, H // 6) - 2                        # a circle of radius a stays inside its cell
            a = rng.randint(max(3, m // 3), m)
            b = rng.randint(max(2, a // 2), a + 1)
            nodes[s, j] = (cx, cy, a, b, rng.randint(1, 180), rng.randint(1, 12), rng.randint(0, 2), 1)
        nnode[s] = n
    return waves, nodes, nnode
