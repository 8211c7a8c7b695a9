"""Host restatement of spnet_fake_espi_params (csrc/espi_params.hip; the recipe is the comment above its prototype in
include/spnet_hip.h): the same counter RNG, the same multiply-shift integers, the same trig2 table, the box test in numpy
float32 with every product and sum rounded on its own.  Sequential over frames and antinodes, as the rejection loop is; the
candidates of one antinode are independent draws, so they are evaluated as arrays (the first 64, then the rest) and the first
passing one is taken -- the plain loop `for t in range(2000): ... break`, written with numpy.  No GPU, no library."""
import numpy as np

MAX_NODES, MAX_TRIES = 7, 2000
_M32 = 0xFFFFFFFF
_U32 = np.uint64(_M32)


def trig2_table():
    """[181][2] float32 = (cos^2, sin^2) of the whole degrees 0..180, computed in float64."""
    rad = np.radians(np.arange(181, dtype=np.float64))
    return np.stack([np.cos(rad) ** 2, np.sin(rad) ** 2], 1).astype(np.float32)


def mix(x):
    """The device mixer (rng_mix of csrc/counter_rng.h), restated, on uint32 arrays (or Python ints)."""
    if isinstance(x, int):
        x &= _M32
        x ^= x >> 16
        x = (x * 0x7feb352d) & _M32
        x ^= x >> 15
        x = (x * 0x846ca68b) & _M32
        x ^= x >> 16
        return x
    x = np.asarray(x, np.uint64) & _U32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & _U32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & _U32
    x ^= x >> np.uint64(16)
    return x


def frame_key(seed, g):
    return mix(mix(mix((seed & _M32) ^ 0x9e3779b9) + (g & _M32)) ^ ((g >> 32) & _M32))


def key(fkey, slot, t):
    if isinstance(t, int):
        return mix(fkey + ((slot << 12) | t))
    return mix(np.uint64(fkey) + (np.uint64(slot << 12) | np.asarray(t, np.uint64)))


def draw(k_, k):
    c = (k * 0x85ebca6b + 0xc2b2ae35) & _M32
    if isinstance(k_, int):
        return mix(k_ ^ c)
    return mix(k_ ^ np.uint64(c))


def randint(u, lo, hi):
    """lo + (u * max(hi - lo + 1, 1) >> 32); lo / hi ints or int64 arrays."""
    if isinstance(u, int):
        return lo + ((u * max(hi - lo + 1, 1)) >> 32)
    n = np.maximum(np.asarray(hi, np.int64) - lo + 1, 1).astype(np.uint64)
    return np.asarray(lo, np.int64) + ((u * n) >> np.uint64(32)).astype(np.int64)


def _candidates(fkey, j, t, H, W, trig2):
    """Every draw of tries t (int64 array) of antinode j, and their boxes (float32)."""
    kk = key(fkey, j + 1, t)
    first = t == 0
    a1 = np.where(first, randint(draw(kk, 0), 15, (2 * W) // 7), randint(draw(kk, 0), 25, W // 3))
    a2 = np.where(first, randint(draw(kk, 1), 15, (2 * H) // 7), randint(draw(kk, 1), 25, H // 3))
    a, b = np.maximum(a1, a2), np.minimum(a1, a2)
    rdrawn = randint(draw(kk, 2), 1, np.minimum(b // 8, 11))
    rcap = np.where(first, np.minimum(b // 4, rdrawn), b // 4)
    cx = randint(draw(kk, 3), a, W - a)
    cy = randint(draw(kk, 4), b, H - b)
    ang = np.where(first, randint(draw(kk, 5), 1, 179), randint(draw(kk, 5), 1, 180))
    c2, s2 = trig2[ang, 0], trig2[ang, 1]
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    fa2, fb2 = fa * fa, fb * fb
    dx = np.sqrt(fa2 * c2 + fb2 * s2)          # float32 throughout: numpy rounds every operation, np.sqrt is correctly rounded
    dy = np.sqrt(fa2 * s2 + fb2 * c2)
    assert dx.dtype == np.float32 and dy.dtype == np.float32
    fx, fy = cx.astype(np.float32), cy.astype(np.float32)
    return a, b, rcap, cx, cy, ang, (fx - dx, fy - dy, fx + dx, fy + dy)


def params(first_frame, N, seed=0, count_range=(1, 7), H=384, W=512):
    """-> dict(waves float32 [N,5], nodes float32 [N,7,8], nnode int32 [N], tries int32 [N,7], count int32 [N] (the number of
    antinodes DRAWN), boxes: per frame the list of accepted (x0, y0, x1, y1) float32)."""
    trig2 = trig2_table()
    waves = np.zeros((N, 5), np.float32)
    nodes = np.zeros((N, MAX_NODES, 8), np.float32)
    nnode = np.zeros(N, np.int32)
    tries = np.full((N, MAX_NODES), -2, np.int32)
    count = np.zeros(N, np.int32)
    all_boxes = []
    fW, fH = np.float32(W), np.float32(H)
    for f in range(N):
        fkey = frame_key(seed, first_frame + f)
        k0 = key(fkey, 0, 0)
        amp = randint(draw(k0, 0), 10, 200)
        wavelength = randint(draw(k0, 1), 100, W // 2)
        thick = randint(draw(k0, 2), 15, 40)
        u01 = np.float32(draw(k0, 3) >> 8) * np.float32(2.0 ** -24)
        slope = np.float32(3) * (u01 - np.float32(0.5))
        steep = int(abs(np.float32(1.5) * slope))
        spacing = randint(draw(k0, 4), thick + thick * steep, H // 3)
        count[f] = randint(draw(k0, 5), count_range[0], count_range[1])
        waves[f] = (amp, wavelength, thick, slope, spacing)
        boxes = []
        for j in range(int(count[f])):
            start = draw(key(fkey, j + 1, 0), 6) >> 31
            carry = np.int64(2 ** 31 - 1)
            tries[f, j] = -1
            for t0, t1 in ((0, 64), (64, MAX_TRIES)):
                t = np.arange(t0, t1, dtype=np.int64)
                a, b, rcap, cx, cy, ang, (x0, y0, x1, y1) = _candidates(fkey, j, t, H, W, trig2)
                rings = np.minimum(carry, np.minimum.accumulate(rcap))
                bad = (x0 < 0) | (x1 > fW) | (y0 < 0) | (y1 > fH)
                for q in boxes:
                    bad |= ~((x1 < q[0]) | (x0 > q[2]) | (y1 < q[1]) | (y0 > q[3]))
                ok = np.nonzero(~bad)[0]
                if len(ok):
                    i = int(ok[0])
                    nodes[f, len(boxes)] = (cx[i], cy[i], a[i], b[i], ang[i], rings[i], start, 1)
                    boxes.append((x0[i], y0[i], x1[i], y1[i]))
                    tries[f, j] = t0 + i
                    break
                carry = rings[-1]
        nnode[f] = len(boxes)
        all_boxes.append(boxes)
    return dict(waves=waves, nodes=nodes, nnode=nnode, tries=tries, count=count, boxes=all_boxes)
