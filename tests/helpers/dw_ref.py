"""Exact references for the depthwise 3x3 family (csrc/dwconv.hip) and the pooling layers (csrc/pool.hip).

numpy only, nothing of the code under test, in the spirit of tests/helpers/gemm_ref.py: operands are small integers (the
BatchNorm xhat of the fused sums is a half-integer at most), so every fmaf and every summation order is exact in fp32 and
the kernels must return the float64 result computed here bit for bit.  assert_exact() proves that for a case, on the CPU,
before anything is launched.  Everything is float64 on NHWC arrays, w is [3][3][C]; the loops run over the nine taps (and,
for the pools, over the output pixels).  Only avgpool3x3s1_same is not exact on the device (a rounded reciprocal): its
float64 result is compared within a derived bound (tests/test_pool_gpu.py).

Guards: place() puts a dense array at a 16-byte-aligned offset > 0 of a larger allocation (NaN around inputs, the
sentinel around and inside outputs), check_placed() demands the expected values and an untouched surrounding."""
import numpy as np

from tests.helpers import gemm_ref as G

LIMIT, NAN, SENTINEL = G.LIMIT, G.NAN, G.SENTINEL
FRONT, TAIL = 8, 64               # guard floats before / behind every placed array


# ---- geometry ----------------------------------------------------------------------------------------------------------------
def same_geom(n, s):
    """(out, pad_before) of TensorFlow's SAME for a 3-wide window: the smaller half of an odd padding in front"""
    out = -(-n // s)
    return out, max((out - 1) * s + 3 - n, 0) // 2


def valid_geom(n):
    return (n - 3) // 2 + 1, 0


def _padded(x, s, fill=0.0):
    """x padded so that tap (kh, kw) of output (oh, ow) is xp[:, oh*s + kh, ow*s + kw]; (xp, OH, OW, pt, pl)"""
    B, H, W, C = x.shape
    (OH, pt), (OW, pl) = same_geom(H, s), same_geom(W, s)
    hp, wp = max((OH - 1) * s + 3, H + pt), max((OW - 1) * s + 3, W + pl)
    xp = np.full((B, hp, wp, C), fill, np.float64)
    xp[:, pt:pt + H, pl:pl + W] = x
    return xp, OH, OW, pt, pl


def _tap(xp, kh, kw, OH, OW, s):
    return xp[:, kh:kh + (OH - 1) * s + 1:s, kw:kw + (OW - 1) * s + 1:s]


# ---- depthwise 3x3, TF-SAME, stride 1 | 2 ------------------------------------------------------------------------------------
def dw_fwd(x, w, stride=1):
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    xp, OH, OW, _, _ = _padded(x, stride)
    y = np.zeros((x.shape[0], OH, OW, x.shape[3]))
    for kh in range(3):
        for kw in range(3):
            y += _tap(xp, kh, kw, OH, OW, stride) * w[kh, kw]
    return y


def dw_bwd_data(dy, w, H, W, stride=1):
    dy, w = np.asarray(dy, np.float64), np.asarray(w, np.float64)
    B, OH, OW, C = dy.shape
    dxp, oh, ow, pt, pl = _padded(np.zeros((B, H, W, C)), stride)
    assert (oh, ow) == (OH, OW)
    for kh in range(3):
        for kw in range(3):
            _tap(dxp, kh, kw, OH, OW, stride)[...] += dy * w[kh, kw]
    return dxp[:, pt:pt + H, pl:pl + W].copy()


def dw_bwd_weight(x, dy, stride=1):
    x, dy = np.asarray(x, np.float64), np.asarray(dy, np.float64)
    xp, OH, OW, _, _ = _padded(x, stride)
    dw = np.zeros((3, 3, x.shape[3]))
    for kh in range(3):
        for kw in range(3):
            dw[kh, kw] = (_tap(xp, kh, kw, OH, OW, stride) * dy).sum((0, 1, 2))
    return dw


class Fused:
    """the fused backward of the stride-1 forms (spnet_dwconv3x3_tiled_bwd / _stream_bwd):
         a   = x*scale + shift when the affine is given, else x          xin = relu(a) if relu_in else a
         dx  = dwT(dy, w) * (a > 0 if relu_in) + add                     dw = sum xin (x) dy
         bn sums: sum dx and sum dx * ((pre - mean) * invstd), pre = bn_x when given, otherwise x"""

    def __init__(self, dy, x, w, relu_in=0, add=None, scale=None, shift=None, mean=None, invstd=None, bn_x=None):
        f = lambda t: None if t is None else np.asarray(t, np.float64)
        dy, x, w, add, scale, shift, mean, invstd, bn_x = map(f, (dy, x, w, add, scale, shift, mean, invstd, bn_x))
        B, H, W, C = x.shape
        self.a = x * scale + shift if scale is not None else x
        self.xin = np.maximum(self.a, 0.0) if relu_in else self.a
        self.y = dw_fwd(self.xin, w)
        g = dw_bwd_data(dy, w, H, W)
        if relu_in:
            g = g * (self.a > 0)
        self.dx = g + (add if add is not None else 0.0)
        self.dy = dy
        self.dw = dw_bwd_weight(self.xin, dy)
        self.xhat = None
        if mean is not None:
            self.xhat = ((bn_x if bn_x is not None else x) - mean) * invstd

    def weight_rows(self, regions):
        """[len(regions)][9][C]: dk[kh][kw] = sum over the region's centre pixels q of xin[q] * dy[q - (kh-1, kw-1)]"""
        dzp = np.pad(self.dy, ((0, 0), (1, 1), (1, 1), (0, 0)))
        out = np.zeros((len(regions), 9, self.xin.shape[3]))
        for i, (b, h0, h1, w0, w1) in enumerate(regions):
            for kh in range(3):
                for kw in range(3):
                    out[i, kh * 3 + kw] = (self.xin[b, h0:h1, w0:w1] * dzp[b, h0 - kh + 2:h1 - kh + 2, w0 - kw + 2:w1 - kw + 2]).sum((0, 1))
        return out

    def bn_rows(self, regions):
        """[len(regions)][2][C]: sum dx | sum dx * xhat over the region"""
        out = np.zeros((len(regions), 2, self.xin.shape[3]))
        for i, (b, h0, h1, w0, w1) in enumerate(regions):
            out[i, 0] = self.dx[b, h0:h1, w0:w1].sum((0, 1))
            out[i, 1] = (self.dx[b, h0:h1, w0:w1] * self.xhat[b, h0:h1, w0:w1]).sum((0, 1))
        return out


# ---- partial-row layouts -----------------------------------------------------------------------------------------------------
def tiled_cfg(H, W):
    """dw_geom: cfg 1 = 6x8 pixel tiles x 64 channels when H <= 6 and W <= 8, else cfg 0 = 12x16 x 32 channels"""
    return 1 if (H <= 6 and W <= 8) else 0


def tiled_geom(H, W, C):
    """(cfg, TH, TW, channels per chunk, tile rows, tile columns, channel chunks)"""
    cfg = tiled_cfg(H, W)
    th, tw, cc = (6, 8, 64) if cfg else (12, 16, 32)
    return cfg, th, tw, cc, -(-H // th), -(-W // tw), -(-C // cc)


def tiled_regions(B, H, W):
    """one partial row per (b, tile row, tile column), tile column fastest: (b, h0, h1, w0, w1)"""
    _, th, tw, _, nth, ntw, _ = tiled_geom(H, W, 4)
    return [(b, i * th, min(H, (i + 1) * th), j * tw, min(W, (j + 1) * tw)) for b in range(B) for i in range(nth) for j in range(ntw)]


def stream_geom(B, H, W, C, rows_per_seg, backward=True):
    """dw_stream_geom restated: (strips, channel chunks, segments, rows per segment, waves); 8-column strips x 32 channels"""
    strips, cchunks = -(-W // 8), -(-(C // 4) // 8)
    base = B * strips * cchunks
    if rows_per_seg <= 0:
        segs = 1 if (backward or base >= 2048) else -(-4096 // base)
        rows_per_seg = max(-(-H // segs), 6)
    rows_per_seg = min(rows_per_seg, H)
    segs = -(-H // rows_per_seg)
    return strips, cchunks, segs, rows_per_seg, base * segs


def stream_regions(B, H, W, rows_per_seg):
    """one partial row per (b, row segment, column strip), strip fastest"""
    strips, _, segs, rps, _ = stream_geom(B, H, W, 4, rows_per_seg)
    return [(b, s * rps, min(H, (s + 1) * rps), j * 8, min(W, (j + 1) * 8)) for b in range(B) for s in range(segs) for j in range(strips)]


def chan_lanes(c4n):
    cl = 8
    while cl < c4n and cl < 64:
        cl <<= 1
    return cl


def strided_rows(B, OH, OW, C):
    """dws_rows restated: one partial row per 8 pixels of every thread row, at most 256"""
    by = 256 // chan_lanes(C // 4)
    return max(1, min(256, -(-(B * OH * OW) // (by * 8))))


# ---- pools -------------------------------------------------------------------------------------------------------------------
def _affine(x, ss):
    x = np.asarray(x, np.float64)
    if ss is None:
        return x
    ss = np.asarray(ss, np.float64)
    C = x.shape[-1]
    return x * ss[:C] + ss[C:]


def maxpool_fwd(x, same=True, residual=None, x_ss=None, r_ss=None):
    """(y, taps): 3x3 / stride 2, SAME (-inf padding) or VALID.  taps[b, oh, ow, c] = kh*3 + kw of the FIRST maximum in
    row-major window order over the in-image taps.  x_ss / r_ss: [scale | shift] applied on load."""
    v = _affine(x, x_ss)
    B, H, W, C = v.shape
    (OH, pt), (OW, pl) = (same_geom(H, 2), same_geom(W, 2)) if same else (valid_geom(H), valid_geom(W))
    y = np.full((B, OH, OW, C), -np.inf)
    taps = np.zeros((B, OH, OW, C), np.uint8)
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(3):
                for kw in range(3):
                    h, w = oh * 2 - pt + kh, ow * 2 - pl + kw
                    if 0 <= h < H and 0 <= w < W:
                        better = v[:, h, w] > y[:, oh, ow]
                        y[:, oh, ow] = np.where(better, v[:, h, w], y[:, oh, ow])
                        taps[:, oh, ow] = np.where(better, kh * 3 + kw, taps[:, oh, ow])
    if residual is not None:
        y = y + _affine(residual, r_ss)
    return y, taps


def pack_taps(taps):
    """one byte per channel, four per word, channel 4k in the low byte: [B*OH*OW*C/4] uint32"""
    t = taps.reshape(-1, 4).astype(np.uint32)
    return t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | (t[:, 3] << 24)


def maxpool_bwd(dy, taps, H, W, same=True):
    dy = np.asarray(dy, np.float64)
    B, OH, OW, C = dy.shape
    pt, pl = (same_geom(H, 2)[1], same_geom(W, 2)[1]) if same else (0, 0)
    dx = np.zeros((B, H, W, C))
    for oh in range(OH):
        for ow in range(OW):
            for kh in range(3):
                for kw in range(3):
                    h, w = oh * 2 - pt + kh, ow * 2 - pl + kw
                    if 0 <= h < H and 0 <= w < W:
                        dx[:, h, w] += np.where(taps[:, oh, ow] == kh * 3 + kw, dy[:, oh, ow], 0.0)
    return dx


POOL_PIXELS_PER_STEP = 32        # pixel rows of a workgroup of maxpool_bwd_bnsums_kernel


def maxpool_bn_rows(dx, yp, mean, invstd, rows):
    """[rows][2][C] of spnet_maxpool3x3s2_bwd_bnsums: pixel r = (b*H + h)*W + w belongs to partial row (r / 32) % rows
    (workgroup row y takes the pixels y*32 .. y*32 + 31, then strides by rows*32); sum dx | sum dx * xhat"""
    dx = np.asarray(dx, np.float64)
    C = dx.shape[-1]
    d = dx.reshape(-1, C)
    xhat = (np.asarray(yp, np.float64).reshape(-1, C) - np.asarray(mean, np.float64)) * np.asarray(invstd, np.float64)
    row = (np.arange(d.shape[0]) // POOL_PIXELS_PER_STEP) % rows
    out = np.zeros((rows, 2, C))
    for r in range(rows):
        out[r, 0] = d[row == r].sum(0)
        out[r, 1] = (d[row == r] * xhat[row == r]).sum(0)
    return out


def pool_bwd_rows(B, H, W, max_rows):
    """spnet_maxpool3x3s2_bwd_rows restated: at least four pixels per thread row, at most max_rows"""
    return max(1, min(max(max_rows, 1), -(-(B * H * W) // (32 * 4))))


def avgpool2_fwd(x):
    x = np.asarray(x, np.float64)
    B, H, W, C = x.shape
    OH, OW = H // 2, W // 2
    y = np.zeros((B, OH, OW, C))
    for i in range(2):
        for j in range(2):
            y += x[:, i:2 * OH:2, j:2 * OW:2]
    return y * 0.25


def avgpool2_bwd(dy, H, W):
    dy = np.asarray(dy, np.float64)
    B, OH, OW, C = dy.shape
    dx = np.zeros((B, H, W, C))
    for i in range(2):
        for j in range(2):
            dx[:, i:2 * OH:2, j:2 * OW:2] = 0.25 * dy
    return dx


def avg3_counts(H, W):
    """in-image entries of the 3x3 window around every pixel"""
    nh = np.minimum(np.arange(H) + 1, H - 1) - np.maximum(np.arange(H) - 1, 0) + 1
    nw = np.minimum(np.arange(W) + 1, W - 1) - np.maximum(np.arange(W) - 1, 0) + 1
    return (nh[:, None] * nw[None, :]).astype(np.float64)


def avgpool3_fwd(x):
    """(mean over the in-image window entries, the exact window sums), float64"""
    x = np.asarray(x, np.float64)
    H, W = x.shape[1:3]
    s = dw_fwd(x, np.ones((3, 3, x.shape[3])))
    return s / avg3_counts(H, W)[None, :, :, None], s


def avgpool3_bwd(dy):
    dy = np.asarray(dy, np.float64)
    H, W = dy.shape[1:3]
    return dw_fwd(dy / avg3_counts(H, W)[None, :, :, None], np.ones((3, 3, dy.shape[3])))


# ---- operand draws -----------------------------------------------------------------------------------------------------------
def ints(shape, lo, hi, seed):
    return G.int_operands(shape, lo, hi, seed).astype(np.float64)


def draw_dw(B, H, W, C, seed, v=2):
    """the operands of one stride-1 case: x, dy, add, bn_x, w, shift, mean in [-v, v]; scale from {-2, -1, 1, 2}; invstd from
    {0.5, 1, 2}.  a = x*scale + shift == 0 is made a real case: about one value in six, and x[0, 0, 0, 0] always, is set to
    the x that gives a == 0 (channel 0 has scale +-1, so that such an x exists for every shift)."""
    rs = np.random.RandomState(seed)
    d = {k: ints((B, H, W, C), -v, v, seed * 16 + i + 1) for i, k in enumerate(("x", "dy", "add", "bn_x"))}
    d["w"] = ints((3, 3, C), -v, v, seed * 16 + 5)
    d["shift"], d["mean"] = ints((C,), -v, v, seed * 16 + 6), ints((C,), -v, v, seed * 16 + 7)
    d["scale"] = rs.choice([-2.0, -1.0, 1.0, 2.0], size=C)
    d["scale"][0] = np.sign(d["scale"][0])
    d["invstd"] = rs.choice([0.5, 1.0, 2.0], size=C)
    root = -d["shift"] / d["scale"]                       # the x with a == 0, where it is an integer of the range
    ok = (root == np.rint(root)) & (np.abs(root) <= v)
    plant = (rs.random_sample((B, H, W, C)) < 1.0 / 6) & ok
    plant[0, 0, 0, 0] = True
    d["x"] = np.where(plant, np.broadcast_to(root, plant.shape), d["x"])
    return d


def zero_share(a):
    return float((np.asarray(a) == 0).mean())


def draw_pool(B, H, W, C, seed, same=True, sign=None):
    """integers in [-2, 2] for a max-pool case, with ties planted: in every other (window, channel) with two or more
    in-image taps the last in-image tap is set to the maximum of the others (sign [C] of +-1: the maximum of sign * x, for
    data that goes through an affine with a negative scale on load)"""
    x = ints((B, H, W, C), -2, 2, seed)
    sign = np.ones(C) if sign is None else np.asarray(sign, np.float64)
    (OH, pt), (OW, pl) = (same_geom(H, 2), same_geom(W, 2)) if same else (valid_geom(H), valid_geom(W))
    n = 0
    for oh in range(OH):
        for ow in range(OW):
            hs = [h for h in range(oh * 2 - pt, oh * 2 - pt + 3) if 0 <= h < H]
            ws = [w for w in range(ow * 2 - pl, ow * 2 - pl + 3) if 0 <= w < W]
            if len(hs) * len(ws) < 2:
                continue
            win = x[:, hs[0]:hs[-1] + 1, ws[0]:ws[-1] + 1] * sign
            win[:, -1, -1] = -np.inf                          # the maximum of the OTHER taps: the last tap then ties with it
            sel = (np.arange(C) + n) % 2 == 0
            x[:, hs[-1], ws[-1]] = np.where(sel, win.max((1, 2)) * sign, x[:, hs[-1], ws[-1]])
            n += 1
    return x


def tie_share(v, same=True):
    """share of the (window, channel) pairs with two or more in-image taps that hold their maximum more than once (1.0 when
    no window has two taps: nothing can tie there)"""
    v = np.asarray(v, np.float64)
    B, H, W, C = v.shape
    (OH, pt), (OW, pl) = (same_geom(H, 2), same_geom(W, 2)) if same else (valid_geom(H), valid_geom(W))
    tied = total = 0
    for oh in range(OH):
        for ow in range(OW):
            hs = [h for h in range(oh * 2 - pt, oh * 2 - pt + 3) if 0 <= h < H]
            ws = [w for w in range(ow * 2 - pl, ow * 2 - pl + 3) if 0 <= w < W]
            if len(hs) * len(ws) < 2:
                continue
            win = v[:, hs[0]:hs[-1] + 1, ws[0]:ws[-1] + 1].reshape(B, -1, C)
            tied += int(((win == win.max(1, keepdims=True)).sum(1) > 1).sum())
            total += B * C
    return tied / total if total else 1.0


def draw_ss(C, seed):
    """[scale | shift] of an affine applied on load: scale from {-2, -1, 1, 2}, shift in [-2, 2]"""
    rs = np.random.RandomState(seed)
    return np.concatenate([rs.choice([-2.0, -1.0, 1.0, 2.0], size=C), rs.randint(-2, 3, size=C).astype(np.float64)])


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def _check_units(arrays, unit):
    for a in arrays:
        if a is None:
            continue
        a = np.asarray(a, np.float64)
        if not np.array_equal(np.rint(a / unit), a / unit):
            raise ValueError("operand is not a multiple of %g" % unit)


def assert_exact_dw(dy, x, w, add=None, scale=None, shift=None, mean=None, invstd=None, bn_x=None, stride=1):
    """a test-authoring check, run on the CPU before any launch: every intermediate and every sum of the case -- whatever
    the order, whatever the ReLU does -- stays below 2^24 units, the unit being 1 for the integers and the smallest
    invstd (0.5) for the BatchNorm sums, whose terms are half-integers.  Bounds come from absolute values: |a|, the forward
    and data-gradient sums of |.| * |w|, and, over ALL pixels, the weight sums |xin| * |dy| and the two BatchNorm sums."""
    _check_units((dy, x, w, add, scale, shift, mean, bn_x), 1.0)
    f = lambda t: None if t is None else np.abs(np.asarray(t, np.float64))
    ady, ax, aw, aadd, asc, ash = map(f, (dy, x, w, add, scale, shift))
    a = ax * asc + ash if scale is not None else ax
    B, H, W, C = ax.shape
    bounds = [a.max(), dw_fwd(a, aw, stride).max()]
    g = dw_bwd_data(ady, aw, H, W, stride) + (aadd if add is not None else 0.0)
    bounds += [g.max(), dw_bwd_weight(a, ady, stride).max()]
    unit = 1.0
    if mean is not None:
        _check_units((invstd,), 0.5)
        unit = min(1.0, float(np.min(invstd)))
        pre = bn_x if bn_x is not None else x
        xhat = (np.abs(np.asarray(pre, np.float64)) + np.abs(np.asarray(mean, np.float64))) * np.abs(np.asarray(invstd, np.float64))
        bounds += [g.sum((0, 1, 2)).max(), (g * xhat).sum((0, 1, 2)).max()]
    b = max(bounds) / unit
    if not b < LIMIT:
        raise AssertionError("case is not exact in fp32: bound %g >= 2^24" % b)
    return b


def assert_exact_pool(x, dy, residual=None, x_ss=None, r_ss=None, yp=None, mean=None, invstd=None):
    """the same for a max-pool case: |v|, |y|, the data gradient (at most four windows meet in a pixel) and the two sums"""
    _check_units((x, dy, residual, x_ss, r_ss, yp, mean), 1.0)
    C = np.asarray(x).shape[-1]
    aff = lambda t, ss: None if t is None else _affine(np.abs(t), None if ss is None else np.abs(ss))
    bounds = [aff(x, x_ss).max() + (aff(residual, r_ss).max() if residual is not None else 0.0)]
    g = 4 * float(np.abs(dy).max())
    bounds.append(g)
    unit = 1.0
    if mean is not None:
        _check_units((invstd,), 0.5)
        unit = min(1.0, float(np.min(invstd)))
        n = np.asarray(yp).size // C
        bounds += [g * n, g * n * float((np.abs(yp).max() + np.abs(mean).max()) * np.abs(invstd).max())]
    b = max(bounds) / unit
    if not b < LIMIT:
        raise AssertionError("case is not exact in fp32: bound %g >= 2^24" % b)
    return b


# ---- guards ------------------------------------------------------------------------------------------------------------------
def place(arr, poison=NAN, front=FRONT, tail=TAIL, inside=None):
    """(buffer float32 [front + n + tail], offset): the array behind `front` poison floats (front % 4 == 0 and > 0: 16-byte
    aligned, not at the start of its allocation) and before `tail` of them; inside: fill the array's place with this instead"""
    a = np.asarray(arr, np.float32).ravel()
    if front % 4 or front <= 0:
        raise ValueError("place: front %d" % front)
    buf = np.full(front + a.size + tail, poison, np.float32)
    buf[front:front + a.size] = a if inside is None else inside
    return buf, front


def check_placed(buf, want, front=FRONT, tail=TAIL, sentinel=SENTINEL):
    """findings ([] = fine) about an output laid out by place(): the values (NaN == NaN), and the sentinel before and behind"""
    buf = np.asarray(buf, np.float32).ravel()
    want = np.asarray(want)
    if want.size == 0:                                        # an empty output: nothing but guards
        return check_guards(buf, 0, front, tail, sentinel)
    found = G.check_dense(buf[front:], want, tail, sentinel)
    hit = np.flatnonzero(buf[:front] != np.float32(sentinel))
    if hit.size:
        found.append("guard overwritten at %d elements in front of the array, first at -%d" % (hit.size, front - int(hit[0])))
    return found


def check_guards(buf, n, front=FRONT, tail=TAIL, sentinel=SENTINEL):
    """the same for a workspace whose contents are not specified: only the sentinel before and behind its n elements"""
    buf = np.asarray(buf, np.float32).ravel()
    found = []
    if buf.size != front + n + tail:
        return ["%d elements, expected %d + %d + %d" % (buf.size, front, n, tail)]
    for name, part in (("in front of", buf[:front]), ("behind", buf[front + n:])):
        hit = np.flatnonzero(part != np.float32(sentinel))
        if hit.size:
            found.append("guard overwritten at %d elements %s the workspace, first at %d" % (hit.size, name, int(hit[0])))
    return found


# ---- bf16x3 planes (csrc/x3t.h) ----------------------------------------------------------------------------------------------
def x3_offsets(R, K):
    """[R][K] element offsets inside one plane: ((r/16)*nk + k/32)*512 + (r%16)*32 + (((k%32)/8 ^ -((r%16)/4)) & 3)*8 + k%8"""
    nk = (K + 31) // 32
    r, k = np.arange(R)[:, None], np.arange(K)[None, :]
    r16 = r % 16
    return ((r // 16) * nk + k // 32) * 512 + r16 * 32 + ((((k % 32) // 8) ^ (-(r16 // 4))) & 3) * 8 + k % 8


def plane_elems(R, K):
    return ((R + 15) // 16) * ((K + 31) // 32) * 512


def check_planes(words, want, front, tail, sentinel_word):
    """findings about a plane set (uint16 words: `front` sentinel words, 3 planes, `tail` sentinel words) that must hold the
    [R][K] matrix `want` of integers below 2^8 in magnitude: the high plane equals it, the middle and low planes and
    every pad row / column are zero, the sentinel around the allocation is intact"""
    words = np.asarray(words).view(np.uint16).ravel()
    want = np.asarray(want, np.float64)
    R, K = want.shape
    ps = plane_elems(R, K)
    if words.size != front + 3 * ps + tail:
        return ["%d words, expected %d + %d + %d" % (words.size, front, 3 * ps, tail)]
    found = []
    body = words[front:front + 3 * ps].reshape(3, ps)
    val = (body.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    off = x3_offsets(R, K)
    bad = np.argwhere(val[0][off] != want)
    for r, k in bad[:8]:
        found.append("high plane differs at (%d, %d): got %r want %r" % (r, k, val[0][off[r, k]], want[r, k]))
    if len(bad) > 8:
        found.append("... %d elements differ in all" % len(bad))
    pad = np.ones(ps, bool)
    pad[off.ravel()] = False
    for name, hit in (("pad elements of the high plane", body[0][pad] != 0), ("middle plane", body[1] != 0), ("low plane", body[2] != 0)):
        if hit.any():
            found.append("%s: %d elements are not zero" % (name, int(hit.sum())))
    for name, part in (("in front of", words[:front]), ("behind", words[front + 3 * ps:])):
        if (part != sentinel_word).any():
            found.append("sentinel overwritten %s the planes" % name)
    return found
