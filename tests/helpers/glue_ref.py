"""Exact references for the Inception-ResNet-v2 glue (csrc/conv_general.hip) and the DenseNet121 glue (csrc/densenet.hip).

numpy only, nothing of the code under test, in the spirit of tests/helpers/gemm_ref.py and dw_ref.py: operands are small
integers (values in +-3, integer means, invstd in {0.5, 1, 2}, scales that are powers of two or small integers), so every
fmaf, every contraction and every summation order is exact in fp32 and a kernel must return the int64 / float64 result
computed here bit for bit.  An assert_exact_* per family proves that for a case, on the CPU, before anything is launched.
The few places that round (spnet_resadd at scale 0.17, spnet_dense_coeffs, spnet_dense_consumer_fin) are restated
rounding by rounding with bn_ref.fma32; spnet_dense_producer_fin off its exact cases is the one float64 comparison
(producer_fin_bound).

Partial-row layouts, as include/spnet_hip.h documents them:
  the two bnsums producers     pixel r belongs to partial row (r / 32) % rows
  the DenseNet column sums     partial row p holds the pixels 64p .. 64p+63"""
import numpy as np

from tests.helpers import bn_ref as BN
from tests.helpers import dw_ref as D
from tests.helpers import gemm_ref as G

LIMIT, NAN, SENTINEL = G.LIMIT, G.NAN, G.SENTINEL
F32 = np.float32

# ---- launch geometry, restated -------------------------------------------------------------------------------------------
UNROLLED_TAPS = ((3, 3), (1, 7), (7, 1), (1, 3), (3, 1), (5, 5))      # grad_bnsums_kernel<0, KH, KW>, stride 1 only
EW_CAP_ITEMS = 8192 * 256          # spnet_ew_grid: more float4 items than this and the elementwise kernels grid-stride
BATCHED_CAP_ITEMS = 64 * 256       # spnet_copy_cols_batched: 64 workgroups per job
APPLY_CAP_ITEMS = 16384 * 256      # spnet_dense_apply_ld / spnet_dense_producer_fin
CONV7_FWD_CAP_PIXELS = 8192 * 16   # output pixels of spnet_dense_conv7 op 0
CONV7_DGRAD_CAP_PIXELS = 8192 * 256    # input pixels of op 1
BN_PIXELS, BN_QUADS = 32, 8        # grad_bnsums_kernel: 32 pixel rows x 8 channel quads per workgroup
DN_ROWS, DN_QUADS = 64, 64         # dn_colsums_kernel / dn_consumer_bwd_kernel: 64-row slabs, 64 channel quads
CONV7_K, CONV7_CO, CONV7_SLAB_PIXELS, CONV7_MAX_SLABS, CONV7_STEP = 147, 64, 2048, 512, 32


def unrolled(KH, KW, stride):
    """the adjoint gather of spnet_patches_bwd_bnsums takes the unrolled, branch-free tap loop"""
    return stride == 1 and (KH, KW) in UNROLLED_TAPS


def grad_bnsums_rows(npix, max_rows):
    """spnet_grad_bnsums_rows restated: one partial row per 32 pixels, at most max_rows, at least 1"""
    return max(1, min(max(max_rows, 1), -(-npix // BN_PIXELS)))


def dense_rows(M):
    return -(-M // DN_ROWS)


def conv7_out(n):
    return (n - 1) // 2 + 1


def conv7_slabs(B, H, W):
    return max(1, min(CONV7_MAX_SLABS, -(-(B * conv7_out(H) * conv7_out(W)) // CONV7_SLAB_PIXELS)))


def conv7_ws(B, H, W):
    """spnet_dense_conv7_ws restated: one [147][64] slab per 2048 output pixels, at most 512"""
    return conv7_slabs(B, H, W) * CONV7_K * CONV7_CO


# ---- patch matrix and its adjoint (one slice per tap; gemm_ref.patch_matrix is the pixel-by-pixel statement) ---------------
def _pad_geom(H, W, KH, KW, stride, same):
    OH, OW, pt, pl = G.conv_geometry(H, W, KH, KW, stride, same)
    if OH < 1 or OW < 1:
        raise ValueError("no output: %dx%d window %dx%d stride %d %s" % (H, W, KH, KW, stride, "same" if same else "valid"))
    return OH, OW, pt, pl, max((OH - 1) * stride + KH, H + pt), max((OW - 1) * stride + KW, W + pl)


def patch_matrix(x, KH, KW, stride, same):
    """[B*OH*OW][KH*KW*C], the dtype of x kept: == gemm_ref.patch_matrix (tests/test_glue_ref_cpu.py)"""
    x = np.asarray(x)
    B, H, W, C = x.shape
    OH, OW, pt, pl, HP, WP = _pad_geom(H, W, KH, KW, stride, same)
    xp = np.zeros((B, HP, WP, C), x.dtype)
    xp[:, pt:pt + H, pl:pl + W] = x
    col = np.zeros((B, OH, OW, KH, KW, C), x.dtype)
    for kh in range(KH):
        for kw in range(KW):
            col[:, :, :, kh, kw] = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
    return col.reshape(B * OH * OW, KH * KW * C)


def patch_adjoint(dcol, B, H, W, C, KH, KW, stride, same):
    """the transpose of patch_matrix: dx [B][H][W][C], dx[b, ih, iw] = sum of dcol[(b, oh, ow)][(kh, kw)] over the
    (oh, ow, kh, kw) with ih = oh*s + kh - pt, iw = ow*s + kw - pl"""
    dcol = np.asarray(dcol)
    OH, OW, pt, pl, HP, WP = _pad_geom(H, W, KH, KW, stride, same)
    d = dcol.reshape(B, OH, OW, KH, KW, C)
    dxp = np.zeros((B, HP, WP, C), dcol.dtype)
    for kh in range(KH):
        for kw in range(KW):
            dxp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride] += d[:, :, :, kh, kw]
    return dxp[:, pt:pt + H, pl:pl + W].copy()


# ---- gradient producers with BatchNorm sums ----------------------------------------------------------------------------------
def relu_mask(g, y, relu):
    """g where y > 0 (strict: +0.0 and -0.0 pass nothing), else +0"""
    g = np.asarray(g, np.float64)
    return np.where(np.asarray(y, np.float64) > 0, g, 0.0) if relu else g


def bn_rows(g, yp, mean, invstd, rows):
    """[rows][2][C] float64 of grad_bnsums_kernel: g, yp [M][C]; pixel r belongs to partial row (r // 32) % rows;
    sum g | sum g * xhat, xhat = (yp - mean) * invstd"""
    g, yp = np.asarray(g, np.float64), np.asarray(yp, np.float64)
    M, C = g.shape
    xhat = (yp.reshape(M, C) - np.asarray(mean, np.float64)) * np.asarray(invstd, np.float64)
    row = (np.arange(M) // BN_PIXELS) % rows
    out = np.zeros((rows, 2, C))
    for p in range(rows):
        out[p, 0] = g[row == p].sum(0)
        out[p, 1] = (g[row == p] * xhat[row == p]).sum(0)
    return out


# ---- elementwise glue ---------------------------------------------------------------------------------------------------------
def copy_cols(dst0, src, accumulate):
    src = np.asarray(src, np.float64)
    return np.asarray(dst0, np.float64) + src if accumulate else src.copy()


def copy_cols_batched(width, rows, srcs, fill=SENTINEL):
    """the destination [rows][width] of column-block jobs laid side by side, job j = srcs[j] [rows_j][cols_j] at the
    columns behind job j-1; `fill` where no job writes (rows_j < rows, or columns behind the last job)"""
    out = np.full((rows, width), fill, np.float64)
    off = 0
    for s in srcs:
        out[:s.shape[0], off:off + s.shape[1]] = s
        off += s.shape[1]
    return out


def resadd(x, up, scale, relu, exact=False):
    """fmaf(scale, up, x) (+ ReLU) as fp32.  exact=True: the float64 value, asserted to BE an fp32 (integers and a
    power-of-two scale); otherwise one correctly rounded fma per element (bn_ref.fma32: slow, small n only)"""
    s = F32(scale)
    if exact:
        e = np.asarray(x, np.float64) + np.float64(s) * np.asarray(up, np.float64)
        y = e.astype(F32)
        if not np.array_equal(y.astype(np.float64), e):
            raise AssertionError("resadd case is not exact in fp32")
    else:
        y = BN.fma32(s, np.asarray(up, F32), np.asarray(x, F32))
    return np.maximum(y, F32(0)) if relu else y


def resadd_bwd(y, g, scale, relu):
    """(dx, dup) as fp32: dx = g where y > 0 (relu) | g; dup = scale * dx, ONE fp32 product"""
    dx = relu_mask(g, y, relu).astype(F32)
    return dx, F32(scale) * dx


def pad_nhwc(x, pt, pb, pl, pr, backward=False):
    x = np.asarray(x)
    if backward:
        return x[:, pt:x.shape[1] - pb, pl:x.shape[2] - pr].copy()
    return np.pad(x, ((0, 0), (pt, pb), (pl, pr), (0, 0)))


# ---- conv1/conv of DenseNet: ZeroPadding2D(3) + Conv2D(64, 7, strides 2, valid) on 3 channels, int64 ----------------------------
def conv7_fwd(x, w):
    x, w = G.as_int(x), G.as_int(w)
    B, H, W, _ = x.shape
    col = patch_matrix(pad_nhwc(x, 3, 3, 3, 3), 7, 7, 2, 0)
    return (col @ w.reshape(CONV7_K, CONV7_CO)).reshape(B, conv7_out(H), conv7_out(W), CONV7_CO)


def conv7_dgrad(dy, w, H, W):
    dy, w = G.as_int(dy), G.as_int(w)
    B = dy.shape[0]
    dcol = dy.reshape(-1, CONV7_CO) @ w.reshape(CONV7_K, CONV7_CO).T
    return patch_adjoint(dcol, B, H + 6, W + 6, 3, 7, 7, 2, 0)[:, 3:3 + H, 3:3 + W].copy()


def conv7_wgrad(x, dy):
    x, dy = G.as_int(x), G.as_int(dy)
    col = patch_matrix(pad_nhwc(x, 3, 3, 3, 3), 7, 7, 2, 0)
    return (col.T @ dy.reshape(-1, CONV7_CO)).reshape(7, 7, 3, CONV7_CO)


def conv7_fwd_scatter(points, w, B, H, W):
    """conv7_fwd of an x that is zero except at points = [(b, h, w, ci, value)]: a scatter over those positions"""
    w = G.as_int(w)
    OH, OW = conv7_out(H), conv7_out(W)
    y = np.zeros((B, OH, OW, CONV7_CO), np.int64)
    for b, h, ww, ci, v in points:
        for kh in range(7):
            for kw in range(7):
                th, tw = h + 3 - kh, ww + 3 - kw              # = 2*oh, 2*ow
                if th >= 0 and tw >= 0 and th % 2 == 0 and tw % 2 == 0 and th // 2 < OH and tw // 2 < OW:
                    y[b, th // 2, tw // 2] += int(v) * w[kh, kw, ci]
    return y


def conv7_dgrad_scatter(points, w, B, H, W):
    """conv7_dgrad of a dy that is zero except at points = [(b, oh, ow, co, value)]"""
    w = G.as_int(w)
    dx = np.zeros((B, H, W, 3), np.int64)
    for b, oh, ow, co, v in points:
        for kh in range(7):
            for kw in range(7):
                h, ww = oh * 2 - 3 + kh, ow * 2 - 3 + kw
                if 0 <= h < H and 0 <= ww < W:
                    dx[b, h, ww] += int(v) * w[kh, kw, :, co]
    return dx


# ---- DenseNet BatchNorm glue -----------------------------------------------------------------------------------------------------
def dense_colsums(x):
    """[ceil(M/64)][2][C] int64: sum and sum of squares of each 64-row slab"""
    return G.col_stats(G.as_int(x), DN_ROWS)


def dense_coeffs(c, cld, gamma, beta, mean, invstd, bmean, bvar, mm, mv, eps, momentum, training):
    """(coef [3*cld], mm, mv) as fp32, bit for bit (restated as bn_ref.finalize_bits does): coef = [scale | 0 | shift],
    zero from channel c on.  training: scale = gamma*invstd (one fp32 product), shift = fmaf(-mean, scale, beta), moving
    <- momentum*moving + (1 - momentum)*batch (two fp32 products and one fp32 sum, each rounded on its own).
    inference: invstd = float32(1 / sqrt(float64(mv) + float64(eps))), mean = mm; mm, mv are returned unchanged."""
    f = lambda a: None if a is None else np.asarray(a, F32)[:c]
    gamma, beta, mean, invstd, bmean, bvar = map(f, (gamma, beta, mean, invstd, bmean, bvar))
    mm, mv = np.array(mm, F32), np.array(mv, F32)
    eps, momentum = F32(eps), F32(momentum)
    coef = np.zeros(3 * cld, F32)
    if training:
        scale = gamma * invstd
        shift = BN.fma32(-mean, scale, beta)
        one_m = F32(1.0) - momentum
        mm[:c] = momentum * mm[:c] + one_m * bmean
        mv[:c] = momentum * mv[:c] + one_m * bvar
    else:
        inv = (1.0 / np.sqrt(mv[:c].astype(np.float64) + np.float64(eps))).astype(F32)
        scale = gamma * inv
        shift = BN.fma32(-mm[:c], scale, beta)
    assert scale.dtype == F32 and shift.dtype == F32 and mm.dtype == F32
    coef[:c], coef[2 * cld:2 * cld + c] = scale, shift
    return coef, mm, mv


def dense_apply(x, scale, shift, relu):
    """act(scale*x + shift), float64 (exact on the integer draws: assert_exact_dense)"""
    a = np.asarray(x, np.float64) * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    return np.maximum(a, 0.0) if relu else a


def dense_consumer_bwd(dz, x, scale, shift, mean, invstd, gamma, relu, G0):
    """(g, G, partial [ceil(M/64)][2][c]) float64: g = dz where scale*x + shift > 0 (relu) | dz; G = G0 + gamma*g;
    partial row p = (sum g, sum g*xhat) over the pixels 64p .. 64p+63"""
    dz, x = np.asarray(dz, np.float64), np.asarray(x, np.float64)
    a = x * np.asarray(scale, np.float64) + np.asarray(shift, np.float64)
    g = np.where(a > 0, dz, 0.0) if relu else dz.copy()
    xhat = (x - np.asarray(mean, np.float64)) * np.asarray(invstd, np.float64)
    M, c = g.shape
    P = dense_rows(M)
    part = np.zeros((P, 2, c))
    for p in range(P):
        sl = slice(p * DN_ROWS, (p + 1) * DN_ROWS)
        part[p, 0], part[p, 1] = g[sl].sum(0), (g[sl] * xhat[sl]).sum(0)
    return g, np.asarray(G0, np.float64) + np.asarray(gamma, np.float64) * g, part


def dense_consumer_fin(partial, gamma, u0, v0):
    """(dgamma, dbeta, u, v) as fp32: the double sum over the partial rows, ONE cast, then u = fmaf(gamma, dbeta, u0),
    v = fmaf(gamma, dgamma, v0)"""
    s = np.asarray(partial, np.float64).sum(0)
    dbeta, dgamma = s[0].astype(F32), s[1].astype(F32)
    gamma = np.asarray(gamma, F32)
    return dgamma, dbeta, BN.fma32(gamma, dbeta, np.asarray(u0, F32)), BN.fma32(gamma, dgamma, np.asarray(v0, F32))


def dense_producer_fin(Gm, u, v, x, mean, invstd, M):
    """invstd * (G - u/M - xhat*v/M), float64, on the channel block handed in"""
    Gm, u, v, x, mean, invstd = (np.asarray(a, np.float64) for a in (Gm, u, v, x, mean, invstd))
    return invstd * (Gm - u / M - (x - mean) * invstd * v / M)


def producer_fin_bound(Gm, u, v, x, mean, invstd, M):
    """The expression has six fp32 roundings, contracted or not (1/M, u*rM, v*rM, the xhat product chain, the two
    differences, the outer product): |got - ref| <= 8 * 2^-24 * invstd * (|G| + |u|/M + |xhat|*|v|/M) per element"""
    Gm, u, v, x, mean, invstd = (np.asarray(a, np.float64) for a in (Gm, u, v, x, mean, invstd))
    return 8 * BN.U * invstd * (np.abs(Gm) + np.abs(u) / M + np.abs((x - mean) * invstd) * np.abs(v) / M)


# ---- operand draws -------------------------------------------------------------------------------------------------------------
def ints(shape, seed, v=3):
    return D.ints(shape, -v, v, seed)


def ramp(shape, start=1):
    """distinct positive integers: every misplaced element shows"""
    return (np.arange(int(np.prod(shape)), dtype=np.float64) + start).reshape(shape)


def draw_y(shape, seed):
    """a layer output for the ReLU mask: +0.0 and -0.0 a fifth each, the rest integers of both signs; the first element is
    always +0.0 and the second -0.0, so that the smallest tensors hold them too"""
    rs = np.random.RandomState(seed)
    y = rs.choice(np.array([0.0, -0.0, 1.0, 2.0, 3.0, -1.0, -2.0, -3.0]), size=shape, p=[0.2, 0.2, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1])
    y.flat[0] = 0.0
    if y.size > 1:
        y.flat[1] = -0.0
    return y


def draw_stats(C, seed):
    """(mean integers in +-3, invstd from {0.5, 1, 2})"""
    rs = np.random.RandomState(seed)
    return rs.randint(-3, 4, size=C).astype(np.float64), rs.choice([0.5, 1.0, 2.0], size=C)


def draw_affine(x, seed, share=0.2):
    """(x', scale, shift): scale from {-2, -1, 1, 2} (every fourth channel +-1, so that a root exists for every shift),
    shift integers in +-3, and x' = x with `share` of the values replaced by the root -shift/scale where that is an
    integer of the range: scale*x' + shift lands on exactly 0 there"""
    rs = np.random.RandomState(seed)
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    scale = rs.choice([-2.0, -1.0, 1.0, 2.0], size=C)
    scale[::4] = np.sign(scale[::4])
    shift = rs.randint(-3, 4, size=C).astype(np.float64)
    root = -shift / scale
    ok = (root == np.rint(root)) & (np.abs(root) <= 3)
    plant = (rs.random_sample(x.shape) < share) & ok
    return np.where(plant, np.broadcast_to(root, x.shape), x), scale, shift


def draw_gamma(C, seed):
    """powers of two and small integers, both signs"""
    return np.random.RandomState(seed).choice([0.5, 1.0, 2.0, -1.0, 3.0, -2.0], size=C)


def zero_share(a):
    return float((np.asarray(a) == 0).mean())


# ---- exactness -----------------------------------------------------------------------------------------------------------------
def _units(arrays, unit):
    for a in arrays:
        if a is None:
            continue
        a = np.asarray(a, np.float64) / unit
        if not np.array_equal(np.rint(a), a):
            raise ValueError("operand is not a multiple of %g" % unit)


def _below_limit(bound, what):
    if not bound < LIMIT:
        raise AssertionError("%s is not exact in fp32: bound %g >= 2^24" % (what, bound))
    return bound


def assert_exact_patches(x=None, dcol=None, taps=1):
    """the gather moves values (|x| < 2^24); the adjoint adds at most `taps` entries of dcol per pixel"""
    _units((x, dcol), 1.0)
    b = 0.0 if x is None else float(np.abs(x).max())
    if dcol is not None:
        b = max(b, taps * float(np.abs(dcol).max()))
    return _below_limit(b, "patch case")


def assert_exact_bnsums(g_abs, yp, mean, invstd):
    """g_abs [M][C] = an elementwise bound of |g| (the adjoint of |dcol|, or |src|): every sum over ANY set of pixels of
    |g| and of |g| * |xhat| stays below 2^24 units, the unit being min(1, min invstd) (xhat = integer * invstd)"""
    _units((g_abs, yp, mean), 1.0)
    _units((invstd,), 0.5)
    g_abs = np.abs(np.asarray(g_abs, np.float64))
    C = g_abs.shape[-1]
    unit = min(1.0, float(np.min(invstd)))
    xhat = (np.abs(np.asarray(yp, np.float64)).reshape(-1, C) + np.abs(np.asarray(mean, np.float64))) * np.asarray(invstd, np.float64)
    g = g_abs.reshape(-1, C)
    return _below_limit(max(g.sum(0).max(), (g * xhat).sum(0).max()) / unit, "bnsums case")


def assert_exact_elementwise(arrays, factor=1.0, unit=1.0):
    """sums of the given arrays' magnitudes (times factor) in multiples of unit: copy_cols(accumulate), resadd at a
    power-of-two scale, pad"""
    _units(arrays, unit)
    return _below_limit(factor * sum(float(np.abs(a).max()) for a in arrays) / unit, "elementwise case")


def assert_exact_conv7(x=None, w=None, dy=None, bound=None):
    """|x| * |w| summed over a window, |dy| * |w| over the windows that meet in a pixel, |x| * |dy| over ALL output pixels
    (bound: a closed-form one for the sparse cap cases, where the full products are not formed)"""
    _units((x, w, dy), 1.0)
    if bound is None:
        ax, aw, ady = (None if a is None else np.abs(np.asarray(a, np.float64)) for a in (x, w, dy))
        b = []
        if ax is not None and aw is not None:
            b.append(conv7_fwd(ax, aw).max())
        if ady is not None and aw is not None:
            b.append(conv7_dgrad(ady, aw, *(ax.shape[1:3] if ax is not None else (2 * ady.shape[1] - 1, 2 * ady.shape[2] - 1))).max())
        if ax is not None and ady is not None:
            b.append(conv7_wgrad(ax, ady).max())
        bound = float(max(b))
    return _below_limit(bound, "conv7 case")


def assert_exact_dense(x, scale=None, shift=None, dz=None, mean=None, invstd=None, gamma=None, G0=None, calls=1):
    """the DenseNet passes on integer draws: column sums of |x| and x^2 per case (any slab is below the whole), |scale*x| +
    |shift|, and for the consumer backward the sums of |dz| and |dz|*|xhat| over all pixels in units of min(0.5, ..) and
    |G0| + calls * |gamma| * |dz| in units of 0.5"""
    _units((x, shift, dz, mean, G0), 1.0)
    _units((scale, invstd, gamma), 0.5)
    ax = np.abs(np.asarray(x, np.float64))
    b = [ax.sum(0).max(), (ax * ax).sum(0).max()]
    if scale is not None:
        b.append((ax * np.abs(scale) + np.abs(shift)).max() / 0.5)
    if dz is not None:
        adz = np.abs(np.asarray(dz, np.float64))
        xhat = (ax + np.abs(mean)) * np.asarray(invstd, np.float64)
        unit = min(1.0, float(np.min(invstd)))
        b += [adz.sum(0).max(), (adz * xhat).sum(0).max() / unit]
        b.append(((0.0 if G0 is None else np.abs(G0)) + calls * np.abs(gamma) * adz).max() / 0.5)
    return _below_limit(float(max(b)), "dense case")


def assert_exact_producer_fin(Gm, u, v, x, mean, invstd, M):
    """M a power of two, u and v integers: every term is a multiple of 1/(4M) (invstd >= 0.5 twice, 1/M) -- exact when
    the bound of the sum, in those units, stays below 2^24"""
    if M & (M - 1):
        raise AssertionError("M = %d is no power of two" % M)
    _units((Gm, u, v, x, mean), 1.0)
    _units((invstd,), 0.5)
    Gm, u, v, x, mean, invstd = (np.abs(np.asarray(a, np.float64)) for a in (Gm, u, v, x, mean, invstd))
    b = (invstd * (Gm + u / M + (x + mean) * invstd * v / M)).max() * 4 * M
    return _below_limit(float(b), "producer_fin case")
