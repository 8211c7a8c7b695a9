"""TEST INFRASTRUCTURE -- the row reductions of csrc/dwconv.hip (spnet_reduce_rows, _ws, _batched) and the movers of
csrc/gemm.hip (spnet_transpose_batched, spnet_gather_s2, spnet_scatter_add_s2) restated with numpy.

Reductions: the operands are integers (all ones, or seeded draws in [-7, 7]), so every order of the fp32 additions gives the
same sum; assert_exact() demands that every partial and total stays below 2^24.  reduce_model() restates the kernel's
assignment of rows to slices and row groups -- slice y of S takes the rows y + g S + 16 S k of group g < 16 -- so that the
planted DEFECTS are one-line variants of it; without a defect it is the plain column sum.

Movers: pure copies are compared on the int32 view (the sources hold NaN payloads and -0.0); scatter-add uses integers at
the sampled pixels and NaN payloads at the others, which must come back bit for bit."""
import numpy as np

LIMIT = 2.0 ** 24
ROWS = (1, 15, 16, 17, 128, 129, 511, 512, 513, 1000)
COLS = (1, 15, 16, 17, 40)
TWO_PASS_ROWS = 128                                      # more rows than this and a scratch: 32 slices first
SLICES = 32
DEFECTS = ("a row group dropped", "slice 31 dropped", "last column dropped", "stride 16 instead of 16 * gridDim.y")
EW_CAP_ITEMS = 8192 * 256


def reduce_data(P, L, kind):
    if kind == "ones":
        return np.ones((P, L), np.float32)
    return np.random.RandomState(97 * P + L).randint(-7, 8, (P, L)).astype(np.float32)


def assert_exact(x):
    assert np.array_equal(x, np.round(x)) and np.abs(x).astype(np.float64).sum(axis=0).max() < LIMIT


def _one_pass(x, S, defect):
    """[S][L]: slice y holds the sum of its rows"""
    P, L = x.shape
    out = np.zeros((S, L))
    for y in range(S):
        for g in range(16):
            if defect == "a row group dropped" and g == 15:
                continue
            step = 16 if defect == "stride 16 instead of 16 * gridDim.y" else 16 * S
            rows = np.arange(y + g * S, P, step)
            out[y] += x[rows].astype(np.float64).sum(axis=0)
    if defect == "last column dropped":
        out[:, L - 1] = np.nan                            # never written: whatever the buffer held
    return out


def reduce_model(x, two_pass, defect=None):
    """out[L] of the one-pass path, or of 32 slices folded by a second pass; NaN marks an element that is never written"""
    assert defect is None or defect in DEFECTS
    if not two_pass:
        return _one_pass(x, 1, None if defect == "slice 31 dropped" else defect)[0]
    slices = _one_pass(x, SLICES, defect)
    if defect == "slice 31 dropped":
        slices = slices[:31]
    return _one_pass(slices, 1, "last column dropped" if defect == "last column dropped" else None)[0]


def takes_two_passes(P, scratch):
    return P > TWO_PASS_ROWS and scratch


BATCH_JOBS = tuple(zip(ROWS, (40, 1, 17, 16, 15, 40, 1, 17, 16, 33)))        # (P, L): max_L 40 comes from two of them


# ---- movers ----------------------------------------------------------------------------------------------------------------
EXTENTS = (1, 31, 32, 33, 65)
TRANSPOSE_JOBS = tuple((r, c) for r in EXTENTS for c in EXTENTS if (r, c) != (65, 65))      # 65 rows and 65 columns: other jobs
S2_SHAPES = tuple((B, H, W, C) for B in (1, 3) for H in (1, 2, 7, 8) for W in (1, 2, 7, 8) for C in (4, 36))
S2_CAP = (1, 257, 257, 512)                              # 129 * 129 * 128 = 2,130,048 float4 items > 8192 * 256


PAYLOAD_PERIOD = (1 << 20) + 7


def payload_bits(n, seed):
    """int32 [n]: distinct small integers as floats, with quiet NaNs of either sign carrying a payload, -0.0, +0.0 and
    denormals mixed in (beyond PAYLOAD_PERIOD elements the pattern repeats, with a period that no tensor extent divides)"""
    if n > PAYLOAD_PERIOD:
        return np.resize(payload_bits(PAYLOAD_PERIOD, seed), n)
    k = np.arange(n, dtype=np.int64) + seed
    bits = (k % 251).astype(np.float32).view(np.int32).astype(np.int64)
    bits = np.where(k % 5 == 1, 0x7FC00000 | (k & 0x3FFFFF), bits)
    bits = np.where(k % 7 == 2, 0xFFC00000 | (k & 0x3FFFFF), bits)
    bits = np.where(k % 11 == 3, 0x80000000, bits)
    bits = np.where(k % 13 == 4, k & 0x7FFFFF, bits)
    return bits.astype(np.uint32).view(np.int32)


def as_floats(bits):
    return np.ascontiguousarray(bits, np.int32).view(np.float32)


def gather_s2(x):
    return np.ascontiguousarray(x[:, ::2, ::2, :])


def scatter_case(B, H, W, C, seed):
    """(dxs float32 integers [B][OH][OW][C], dx float32 [B][H][W][C]: integers at the even pixels, NaN payloads elsewhere,
    want int32 bits of dx afterwards)"""
    OH, OW = (H + 1) // 2, (W + 1) // 2
    n = B * H * W * C
    k = np.arange(n, dtype=np.int64)
    dx = as_floats((0x7FC00000 | ((k * 3 + seed) & 0x3FFFFF) | ((k & 1) << 31)).astype(np.uint32).view(np.int32)).reshape(B, H, W, C).copy()
    dx[:, ::2, ::2, :] = ((np.arange(B * OH * OW * C) * 7 + seed) % 31 - 15).astype(np.float32).reshape(B, OH, OW, C)
    dxs = ((np.arange(B * OH * OW * C) * 5 + seed) % 15 - 7).astype(np.float32).reshape(B, OH, OW, C)
    want = dx.copy()
    want[:, ::2, ::2, :] += dxs
    return dxs, dx, want.view(np.int32)
