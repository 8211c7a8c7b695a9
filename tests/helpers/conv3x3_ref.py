"""Exact reference for the implicit-GEMM passes of block1_conv2 (csrc/conv_gemm.hip): 3x3, stride 1, VALID, NHWC, HWIO.

numpy only, nothing of the code under test, in the spirit of tests/helpers/gemm_ref.py and dw_ref.py: operands are small
integers, assert_exact_conv3x3() proves on the CPU that sum |a||b| of every output of all three passes stays below 2^24,
and then every summation order -- FMA or not, split over pixel slices or not -- gives the same integers: the kernels must
return the int64 result bit for bit.  The three passes are written tap by tap:

  forward           y[b, oh, ow, co]  = sum_{kh, kw, ci} x[b, oh + kh, ow + kw, ci] * w[kh, kw, ci, co]
  data gradient     dx[b, oh + kh, ow + kw, ci] += sum_co dy[b, oh, ow, co] * w[kh, kw, ci, co]        (the same sum as a scatter)
  weight gradient   dw[kh, kw, ci, co] = sum_{b, oh, ow} x[b, oh + kh, ow + kw, ci] * dy[b, oh, ow, co]

dtype=np.int64 is the reference; np.float32 runs the same loops on float32 arrays (the one case above the slice cap, where
int64 products are slow: under the exactness condition both give the same integers, which tests/test_conv3x3_ref_cpu.py
confirms).  Guards come from dw_ref (place / check_placed / check_guards).

GEOMETRIES, CAP_GEOMETRY and draw() are the cases of tests/test_conv3x3_gpu.py; tests/test_conv3x3_ref_cpu.py proves every
one of them exact without a GPU."""
import numpy as np

from tests.helpers import gemm_ref as G

CIN, COUT = 32, 64
LIMIT = G.LIMIT
BK, BM_FWD, BM_DGRAD = 32, 128, 128          # pixels per K tile of the weight gradient; rows per tile of the other two
SLICE_PIXELS, SLICE_CAP = 32 * 64, 170       # spnet_conv3x3_wgrad_ws: at least 64 K tiles per slice, at most 170 slices

# (B, H, W) -> what the geometry is there for
GEOMETRIES = {
    (1, 3, 3): "one output pixel; no interior pixel; nt = 1",
    (2, 3, 34): "OH = 1, OW = 32 = BK; every wrap crosses an image",
    (3, 4, 5): "OW = 3; many wraps per 32-pixel step, across images",
    (1, 5, 35): "OW = 33 = BK + 1",
    (2, 10, 18): "forward M = 256: whole tiles, nothing clamped",
    (1, 3, 131): "forward M = 129 = 128 + 1: 127 clamped rows",
    (1, 8, 16): "dgrad M = 128: whole tile",
    (1, 35, 70): "P = 2244: two slices, 1152 and 1092 pixels; odd tile count; last tile 4 pixels",
    # (3,4,5) has 18 output pixels: one K tile, whose walk nothing reads.  These two make the weight gradient walk:
    (12, 4, 5): "OW = 3 with P = 72: three K tiles; every 32-pixel step wraps ten or eleven rows across five images",
    (40, 3, 3): "OH = OW = 1 with P = 40: two K tiles; a step is 32 row wraps, each of them an image wrap",
}
TWO_SLICES = (1, 35, 70)
CAP_GEOMETRY = (1, 600, 600)                 # P = 357604 > 170 * 2048: 170 slices of 2112 pixels, weight gradient only
PROBE_GEOMETRY = (1, 5, 7)                   # the single-pixel probes
VALUE = 3                                    # operands of GEOMETRIES are integers in [-3, 3]
CAP_VALUE = 2                                # [-2, 2] above the cap: sum |x||dy| <= 4 P = 1,430,416 < 2^24 at any density


def pixels(B, H, W):
    return B * (H - 2) * (W - 2)


def _cast(a, dtype):
    return G.as_int(a) if dtype == np.int64 else np.asarray(a, dtype)


def _tap(x, kh, kw, OH, OW):
    return x[:, kh:kh + OH, kw:kw + OW, :]


def fwd(x, w, dtype=np.int64):
    x, w = _cast(x, dtype), _cast(w, dtype)
    B, H, W, _ = x.shape
    OH, OW = H - 2, W - 2
    y = np.zeros((B, OH, OW, w.shape[3]), dtype)
    for kh in range(3):
        for kw in range(3):
            y += _tap(x, kh, kw, OH, OW) @ w[kh, kw]
    return y


def dgrad(dy, w, dtype=np.int64):
    dy, w = _cast(dy, dtype), _cast(w, dtype)
    B, OH, OW, _ = dy.shape
    dx = np.zeros((B, OH + 2, OW + 2, w.shape[2]), dtype)
    for kh in range(3):
        for kw in range(3):
            _tap(dx, kh, kw, OH, OW)[...] += dy @ w[kh, kw].T
    return dx


def wgrad(x, dy, dtype=np.int64):
    x, dy = _cast(x, dtype), _cast(dy, dtype)
    B, OH, OW, co = dy.shape
    ci = x.shape[3]
    dw = np.zeros((3, 3, ci, co), dtype)
    d2 = np.ascontiguousarray(dy.reshape(-1, co))
    for kh in range(3):
        for kw in range(3):
            dw[kh, kw] = np.ascontiguousarray(_tap(x, kh, kw, OH, OW)).reshape(-1, ci).T @ d2
    return dw


# ---- the host split rule of spnet_conv3x3_wgrad, restated --------------------------------------------------------------------
def wgrad_ws(B, H, W, cin=CIN, cout=COUT):
    """spnet_conv3x3_wgrad_ws: one [9*cin][cout] slab per slice of ceil(P / 2048) slices, 170 at most, one at least"""
    P = pixels(B, H, W)
    return max(1, min(SLICE_CAP, -(-P // SLICE_PIXELS))) * 9 * cin * cout


def split(B, H, W):
    """(ns, p_chunk) as spnet_conv3x3_wgrad launches: the slice length is P / (slabs of the workspace) rounded up, then up
    to whole K tiles of 32 pixels, and the slice count is recomputed from it (rounding can empty the last slices)"""
    P = pixels(B, H, W)
    ns = wgrad_ws(B, H, W) // (9 * CIN * COUT)
    p_chunk = -(-(-(-P // ns)) // BK) * BK
    return -(-P // p_chunk), p_chunk


def slices(B, H, W):
    """pixel count of every slice"""
    P = pixels(B, H, W)
    ns, p_chunk = split(B, H, W)
    return [min(P, (z + 1) * p_chunk) - z * p_chunk for z in range(ns)]


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def exact_bounds(x, w, dy):
    """max over the outputs of sum |a||b|, per pass.  float64 tap loops on the absolute values: integers far below 2^53"""
    ax, aw, ady = (np.abs(G.as_int(a)).astype(np.float64) for a in (x, w, dy))
    return {"fwd": float(fwd(ax, aw, np.float64).max()), "dgrad": float(dgrad(ady, aw, np.float64).max()),
            "wgrad": float(wgrad(ax, ady, np.float64).max())}


def assert_exact_conv3x3(x, w, dy):
    """a test-authoring check, run on the CPU before any launch: for every output of all three passes sum |a||b| < 2^24, so
    no partial sum of any order, fused or not, split over slices or not, leaves the integers fp32 holds exactly"""
    B, H, W, ci = np.shape(x)
    if np.shape(w) != (3, 3, ci, np.shape(dy)[3]) or np.shape(dy)[:3] != (B, H - 2, W - 2):
        raise ValueError("assert_exact_conv3x3: shapes %s %s %s" % (np.shape(x), np.shape(w), np.shape(dy)))
    b = exact_bounds(x, w, dy)
    for name, v in b.items():
        if not v < LIMIT:
            raise AssertionError("%s is not exact in fp32: bound %d >= 2^24" % (name, v))
    return b


# ---- operand draws -----------------------------------------------------------------------------------------------------------
def seed_of(geom):
    return 100 + 7 * (list(GEOMETRIES) + [CAP_GEOMETRY, PROBE_GEOMETRY]).index(geom)


def draw(geom, v=None, density=1.0):
    """(x, w, dy) of a geometry: integer-valued float32 in [-v, v] (gemm_ref.int_operands)"""
    B, H, W = geom
    if v is None:
        v = CAP_VALUE if geom == CAP_GEOMETRY else VALUE
    s = seed_of(geom)
    return (G.int_operands((B, H, W, CIN), -v, v, s, density), G.int_operands((3, 3, CIN, COUT), -v, v, s + 1, density),
            G.int_operands((B, H - 2, W - 2, COUT), -v, v, s + 2, density))


# ---- structural probes -------------------------------------------------------------------------------------------------------
def probe_pixels(H, W):
    """the four corners, the four edge midpoints and one interior pixel of an H x W plane"""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1), (H // 2, W // 2)]


def one_hot(shape, at, values):
    a = np.zeros(shape, np.float32)
    a[at] = values
    return a


def fwd_of_one_pixel(v, w, ih, iw, H, W):
    """forward of an input that is zero but for the channel vector v at (ih, iw): the nine taps laid out mirror-wise --
    output (ih - kh, iw - kw) holds v @ w[kh, kw] wherever that output exists.  int64 [H-2][W-2][COUT]"""
    v, w = G.as_int(v), G.as_int(w)
    y = np.zeros((H - 2, W - 2, w.shape[3]), np.int64)
    for kh in range(3):
        for kw in range(3):
            oh, ow = ih - kh, iw - kw
            if 0 <= oh < H - 2 and 0 <= ow < W - 2:
                y[oh, ow] = v @ w[kh, kw]
    return y


def dgrad_of_one_pixel(g, w, oh, ow, H, W):
    """data gradient of a dy that is zero but for g at (oh, ow): the nine taps laid out directly -- input (oh + kh, ow + kw)
    holds w[kh, kw] @ g.  int64 [H][W][CIN]"""
    g, w = G.as_int(g), G.as_int(w)
    dx = np.zeros((H, W, w.shape[2]), np.int64)
    for kh in range(3):
        for kw in range(3):
            dx[oh + kh, ow + kw] = w[kh, kw] @ g
    return dx


def wgrad_of_one_pixel(x, g, b, oh, ow):
    """weight gradient of a dy that is zero but for g at (b, oh, ow): that pixel's 3 x 3 x CIN window outer g"""
    x, g = G.as_int(x), G.as_int(g)
    return x[b, oh:oh + 3, ow:ow + 3, :, None] * g[None, None, None, :]
