"""Float64 restatements of the reference's band-pass mix-up (spnet/augmentation.py:10-62) for the tests.

literal():   the reference's steps as written, with cv2's (H, W, 2) real / imaginary layout emulated in numpy: the
             fftshift over ALL axes (which also swaps the two planes), the 0/1 uint8 mask on both planes, the unscaled
             inverse, cv2.magnitude, cv2.normalize(NORM_MINMAX) and np.clip.
windowed():  the same result from the 16 x 16 window alone (the formulation csrc/bandpass.hip computes).
fft_pipeline(dtype=np.float32): literal() run through scipy.fft in single precision -- the yardstick for the device's
             error against float64.
Below reference_draw: what the kernel-by-kernel tests need -- mixed() (a host-built window table), emulate_project /
emulate_apply (the kernel's arithmetic order in float32) and the derived error bounds project_bound / recon_bound.
"""
import random

import numpy as np

DBL_EPSILON = np.finfo(np.float64).eps
FLIPS = [-1, 0, 1, 2]


def cv2_flip(t, code):
    if code == 0:
        return t[::-1]
    if code == 1:
        return t[:, ::-1]
    if code == -1:
        return t[::-1, ::-1]
    return t


def cv2_dft(img):
    d = np.fft.fft2(np.asarray(img, np.float64))
    return np.stack([d.real, d.imag], -1)


def cv2_idft(a):
    """cv2.idft of a 2-channel array without DFT_SCALE: the unscaled inverse, complex output."""
    z = np.fft.ifft2(a[..., 0] + 1j * a[..., 1]) * (a.shape[0] * a.shape[1])
    return np.stack([z.real, z.imag], -1)


def cv2_normalize_minmax(x, lo=0.0, hi=255.0):
    smin, smax = float(x.min()), float(x.max())
    scale = (hi - lo) * (1.0 / (smax - smin) if smax - smin > DBL_EPSILON else 0.0)
    return x * scale + (lo - smin * scale)


def literal(f, t, flip, s):
    """f: fake frame [H,W], t: real frame [H,W] (unflipped), flip in FLIPS, s = the scale 3 * rand."""
    f = np.asarray(f, np.float64)
    t = np.asarray(t, np.float64)
    if flip != 2:
        t = cv2_flip(t, flip)
    dft_shift_true = np.fft.fftshift(cv2_dft(t))
    dft_shift_fake = np.fft.fftshift(cv2_dft(f))
    rows, cols = f.shape
    crow, ccol = rows // 2, cols // 2
    wl = 8
    mask = np.zeros((rows, cols, 2), np.uint8)
    mask[crow - wl:crow + wl, ccol - wl:ccol + wl] = 1
    fshift = s * dft_shift_true * mask + (1 - mask) * dft_shift_fake
    back = cv2_idft(np.fft.ifftshift(fshift))
    mag = np.sqrt(back[..., 0] ** 2 + back[..., 1] ** 2)
    return np.clip(cv2_normalize_minmax(mag), 0, 255)


def _window_mats(H, W):
    k = np.arange(-8, 8)
    eh = np.exp(-2j * np.pi * (np.outer(k, np.arange(H)) % H) / H)      # [16, H]
    ew = np.exp(-2j * np.pi * (np.outer(np.arange(W), k) % W) / W)      # [W, 16]
    return eh, ew


def _mm(a, b):
    """a @ b, real float64, in plain loops: a threaded GEMM takes 10 to 100 times as long on matrices this thin"""
    return np.einsum("ij,jk->ik", a, b)


def _cmm(a, b):
    """a @ b for complex or real float64 operands, as real products"""
    ar, ai, br, bi = np.real(a), np.imag(a), np.real(b), np.imag(b)
    if not np.iscomplexobj(b):
        return _mm(ar, br) + 1j * _mm(ai, br)
    if not np.iscomplexobj(a):
        return _mm(ar, br) + 1j * _mm(ar, bi)
    return (_mm(ar, br) - _mm(ai, bi)) + 1j * (_mm(ar, bi) + _mm(ai, br))


def window(img):
    """F[k, l] for k, l in [-8, 8): [16,16] complex, row k + 8, column l + 8."""
    img = np.asarray(img, np.float64)
    eh, ew = _window_mats(*img.shape)
    return _cmm(_cmm(eh, img), ew)


def windowed(f, t, flip, s):
    f = np.asarray(f, np.float64)
    H, W = f.shape
    g = s * window(cv2_flip(np.asarray(t, np.float64), flip)) - window(f)
    eh, ew = _window_mats(H, W)
    y = f + (eh.conj().T @ g @ ew.conj().T) / (H * W)
    return np.clip(cv2_normalize_minmax(np.abs(y)), 0, 255)


def fft_pipeline(f, t, flip, s, dtype=np.float32):
    """literal() in `dtype` through scipy.fft (complex64 for float32)."""
    import scipy.fft as sf
    f = np.asarray(f, dtype)
    t = np.ascontiguousarray(cv2_flip(np.asarray(t, dtype), flip))
    H, W = f.shape
    T = np.fft.fftshift(sf.fft2(t, workers=1))
    F = np.fft.fftshift(sf.fft2(f, workers=1))
    mask = np.zeros((H, W), bool)
    mask[H // 2 - 8:H // 2 + 8, W // 2 - 8:W // 2 + 8] = True
    mixed = np.where(mask, dtype(s) * T, F)
    y = sf.ifft2(np.fft.ifftshift(mixed), workers=1) * dtype(H * W)
    mag = np.abs(y).astype(dtype)
    lo, hi = mag.min(), mag.max()
    scale = dtype(255.0 / (float(hi) - float(lo))) if float(hi) - float(lo) > DBL_EPSILON else dtype(0)
    return np.clip((mag - lo) * scale, 0, 255)


def reference_draw(files):
    """The reference's three RNG calls (augmentation.py:24-27, 51) over the given file list."""
    f = random.choice(files)
    flip = np.random.choice([-1, 0, 1, 2])
    s = np.random.rand() * 3
    return f, int(flip), s


def to_u8(x):
    """cv2.imwrite's conversion of the float result: round half to even, saturate."""
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


# ---- the kernels of csrc/bandpass.hip one by one (tests/test_bandpass_kernels_gpu.py) -------------------------------------
# mixed() / to_pixel32():            the float64 reference with a host-built window table, the kernel's input conversion
# emulate_project / emulate_apply:   a float32 restatement of the kernel's arithmetic order (CPU evidence for the bounds)
# project_bound / mix_bound / recon_bound: a-priori rounding-error bounds, derived below, never fitted
BP_RB, BP_TPB = 64, 256          # rows per block, columns per column tile (csrc/bandpass.hip)
U32 = 2.0 ** -24                 # unit roundoff of float32
REF_EPS = 2.0 ** -40             # everything done in float64 on either side: the twiddles before rounding, this reference
K16 = np.arange(-8, 8)
SHAPES = [(16, 16), (64, 256), (65, 257), (130, 513), (16, 2048), (2048, 16), (47, 331)]
EDGE_ROWS, EDGE_COLS = (0, 1, 63, 64), (0, 1, 255, 256, 511, 512)


def edge_positions(H, W):
    """every pairing of the edge rows {0, 1, 63, 64, H-1} and edge columns {0, 1, 255, 256, 511, 512, W-1} inside the frame"""
    rows = sorted({r for r in EDGE_ROWS + (H - 1,) if r < H})
    cols = sorted({c for c in EDGE_COLS + (W - 1,) if c < W})
    return [(r, c) for r in rows for c in cols]


def to_pixel32(v):
    """x_kind 2 -> pixel units as the kernel converts: fl(fl(fl(v * 0.5) + 0.5) * 255)"""
    v = np.asarray(v, np.float32)
    return (v * np.float32(0.5) + np.float32(0.5)) * np.float32(255.0)


def network_value_of(pixel):
    """a float32 network value whose to_pixel32 is exactly `pixel`, or None"""
    lo = hi = np.float32(2.0 * (pixel / 255.0) - 1.0)
    for _ in range(8):                                            # the neighbours, outwards
        for cand in (lo, hi):
            if float(to_pixel32(cand)) == float(pixel):
                return np.float32(cand)
        lo, hi = np.nextafter(lo, np.float32(-2)), np.nextafter(hi, np.float32(2))
    return None


def mixed(f, table_row, s):
    """windowed() with the real frame's window given: table_row [16,16] complex (or [16,16,2]), s the scale."""
    f = np.asarray(f, np.float64)
    T = np.asarray(table_row)
    if T.shape == (16, 16, 2):
        T = T[..., 0].astype(np.float64) + 1j * T[..., 1].astype(np.float64)
    H, W = f.shape
    g = float(s) * T - window(f)
    eh, ew = _window_mats(H, W)
    y = f + _cmm(_cmm(eh.conj().T, g), ew.conj().T) / (H * W)
    return np.clip(cv2_normalize_minmax(np.abs(y)), 0, 255)


def twiddle32(j, n):
    """(cos, sin)(2 pi j / n) for integer phases j in [0, n), evaluated in float64 and rounded to float32; exact at the
    quarter turns, as sincospi is (cos(pi/2) in radians is 6e-17, not 0)."""
    j = np.asarray(j, np.int64)
    a = 2.0 * np.pi * j.astype(np.float64) / n
    c, s = np.cos(a), np.sin(a)
    quarter = (4 * j) % n == 0
    q = (4 * j) // n % 4
    c = np.where(quarter, np.array([1.0, 0.0, -1.0, 0.0])[q], c)
    s = np.where(quarter, np.array([0.0, 1.0, 0.0, -1.0])[q], s)
    return c.astype(np.float32), s.astype(np.float32)


def emulate_project(d, flip=None, mutant=None):
    """bp_project_kernel + bp_finish_kernel (table NULL) in float32 numpy, the kernel's order: per 64-row block the 16 row
    sums of every column (rows in order), per 256-column tile the 16 column sums of those (columns in order), tiles in
    order, blocks in order; every product and sum rounded on its own (the device may contract some into FMAs: not
    bit-identical, the same error model).  d [N,H,W] float32 in pixel units -> [N,16,16,2].
    mutant (each a bug a correct bound must catch): 'phase' = the column phase of column 256, the first of the second
    tile, one step off; 'nr' = the last row block runs all 64 rows, reading past the frame into the next one."""
    d = np.ascontiguousarray(d, np.float32)
    N, H, W = d.shape
    if flip is not None:
        d = np.stack([cv2_flip(d[n], int(flip[n])) for n in range(N)])
    nb, nt = -(-H // BP_RB), -(-W // BP_TPB)
    rows, cols = nb * BP_RB, nt * BP_TPB
    flat = np.concatenate([d.reshape(-1), np.zeros(rows * W, np.float32)])
    v = np.zeros((N, rows, W), np.float32)
    for n in range(N):
        take = rows if mutant == "nr" else H
        v[n, :take] = flat[n * H * W:n * H * W + take * W].reshape(take, W)
    v = v.reshape(N, nb, BP_RB, W)
    cH, sH = twiddle32((np.arange(rows)[:, None] * K16[None, :]) % H, H)
    cH, sH = cH.reshape(nb, BP_RB, 16), (-sH).reshape(nb, BP_RB, 16)               # exp(-2 pi i k r / H)
    ar = np.zeros((N, nb, 16, cols), np.float32)
    ai = np.zeros((N, nb, 16, cols), np.float32)
    for rl in range(BP_RB):
        x = v[:, :, rl, None, :]
        ar[..., :W] += x * cH[None, :, rl, :, None]
        ai[..., :W] += x * sH[None, :, rl, :, None]
    ar, ai = ar.reshape(N, nb, 16, nt, BP_TPB), ai.reshape(N, nb, 16, nt, BP_TPB)
    ph = (np.arange(cols)[:, None] * K16[None, :]) % W
    if mutant == "phase" and cols > BP_TPB:
        ph[BP_TPB] = (ph[BP_TPB] + 1) % W
    cW, sW = twiddle32(ph, W)
    cW, sW = cW.reshape(nt, BP_TPB, 16), sW.reshape(nt, BP_TPB, 16)
    tr = np.zeros((N, nb, 16, nt, 16), np.float32)
    ti = np.zeros((N, nb, 16, nt, 16), np.float32)
    for cl in range(min(BP_TPB, W)):
        vx, vy, wx, wy = ar[..., cl, None], ai[..., cl, None], cW[:, cl, :], sW[:, cl, :]
        tr += vx * wx + vy * wy
        ti += vy * wx - vx * wy
    accr = np.zeros((N, nb, 16, 16), np.float32)
    acci = np.zeros((N, nb, 16, 16), np.float32)
    for t in range(nt):
        accr += tr[:, :, :, t, :]
        acci += ti[:, :, :, t, :]
    fr = np.zeros((N, 16, 16), np.float32)
    fi = np.zeros((N, 16, 16), np.float32)
    for b in range(nb):
        fr += accr[:, b]
        fi += acci[:, b]
    return np.stack([fr, fi], -1)


def mix_g32(table_rows, s, F, H, W):
    """bp_finish_kernel with a table: G = fl(fl(fl(s * T) - F) * fl(1 / (H W))), all [N,16,16,2] float32"""
    sv = np.asarray(s, np.float32).reshape(-1, 1, 1, 1)
    return (sv * np.asarray(table_rows, np.float32) - np.asarray(F, np.float32)) * np.float32(1.0 / (float(H) * W))


def emulate_apply(x, table, row, s, mutant=None):
    """spnet_bandpass_apply's four launches in float32 numpy: x [N,H,W] float32 pixel units, table [n_table,16,16,2],
    row [N], s [N] -> out_f (f_kind 0) [N,H,W] float32.  mutant: those of emulate_project, or 'sign' = the column twiddle
    of the reconstruction conjugated."""
    x = np.ascontiguousarray(x, np.float32)
    N, H, W = x.shape
    table = np.asarray(table, np.float32)
    d = x - x[:, :1, :1]
    F = emulate_project(d, mutant=mutant)
    G = mix_g32(table[np.clip(np.asarray(row), 0, len(table) - 1)], s, F, H, W)
    cH, sH = twiddle32((np.arange(H)[:, None] * K16[None, :]) % H, H)               # [H,16 k]
    qr = np.zeros((N, H, 16), np.float32)
    qi = np.zeros((N, H, 16), np.float32)
    for kk in range(16):
        ax, ay = G[:, kk, None, :, 0], G[:, kk, None, :, 1]
        wx, wy = cH[None, :, kk, None], sH[None, :, kk, None]
        qr += ax * wx - ay * wy
        qi += ax * wy + ay * wx
    cW, sW = twiddle32((np.arange(W)[:, None] * K16[None, :]) % W, W)               # [W,16 l]
    if mutant == "sign":
        sW = -sW
    yr, yi = d.copy(), np.zeros_like(d)
    for ll in range(16):
        ax, ay = qr[:, :, ll, None], qi[:, :, ll, None]
        wx, wy = cW[None, None, :, ll], sW[None, None, :, ll]
        yr += ax * wx - ay * wy
        yi += ax * wy + ay * wx
    mag = np.sqrt(yr * yr + yi * yi)
    lo, hi = mag.min((1, 2), keepdims=True), mag.max((1, 2), keepdims=True)
    rng = hi - lo
    scale = np.where(rng.astype(np.float64) > DBL_EPSILON, np.float32(255.0) / np.where(rng > 0, rng, np.float32(1)), np.float32(0))
    return np.clip((mag - lo) * scale.astype(np.float32), np.float32(0), np.float32(255))


def gamma(n):
    """Higham's gamma_n: a product of n factors (1 + delta_i), |delta_i| <= u, is 1 + theta with |theta| <= n u / (1 - n u)"""
    return n * U32 / (1.0 - n * U32)


def _chain_adds(d):
    """The additions of NON-ZERO terms on the longest chain of each of the projection's four sums (adding an exact zero is
    exact, and so is the first addition to a zero accumulator): a sum of z non-zero terms puts at most z - 1 roundings
    on any one of them."""
    H, W = d.shape
    nb, nt = -(-H // BP_RB), -(-W // BP_TPB)
    nz = np.zeros((nb * BP_RB, nt * BP_TPB), bool)
    nz[:H, :W] = d != 0
    seg = nz.reshape(nb, BP_RB, nt, BP_TPB).sum(1)                 # [nb,nt,256]: non-zero rows of a column within a block
    col = seg > 0
    tile = col.any(-1)                                             # [nb,nt]
    z = (int(seg.max()), int(col.sum(-1).max()), int(tile.sum(-1).max()), int(tile.any(-1).sum()))
    return sum(max(v - 1, 0) for v in z)


def project_bound(d, centred=False):
    """|device - float64| of every real and imaginary part of the projected window, [16,16,2], for the frame d [H,W] (the
    values the kernel sums: pixel units, after the flip, after centring when centred).

    Re F[k][l] = sum_{r,c} d (cos a cos b - sin a sin b), Im F = -sum d (sin a cos b + cos a sin b), a = 2 pi k r / H,
    b = 2 pi l c / W: every complex product is TWO real terms per part.  The kernel evaluates each part as a recursive
    float32 sum, so by the standard forward bound (Higham, Accuracy and Stability, ch. 4) its error is at most
    gamma_n * sum |terms|, n the number of roundings on the longest chain one term passes through:
      1  the row twiddle rounded to float32            1  the product d * twiddle
      +  the row sum's additions (at most 63)          1  the column twiddle rounded to float32
      1  the product with it                           1  the sum of the part's two products
      +  the column sum's additions (at most 255)      +  the tile sum's and the block sum's additions
      1  when centred: the subtraction d = f - f[0][0]
    with the additions counted per case by _chain_adds: a single-pixel frame has none, so its bound is gamma_5 * A * (|cos cos|
    + |sin sin|), a few ulp of A.  An FMA removes a rounding, never adds one.  sum |terms| is taken in float64 with the
    absolute twiddles.  REF_EPS * sum |d| covers what is done in float64 (the twiddles before rounding, the reference)."""
    d = np.abs(np.asarray(d, np.float64))
    H, W = d.shape
    eh, ew = _window_mats(H, W)
    n = 5 + _chain_adds(d) + (1 if centred else 0)
    ch, sh, cw, sw = np.abs(eh.real), np.abs(eh.imag), np.abs(ew.real), np.abs(ew.imag)
    cd, sd = _mm(ch, d), _mm(sh, d)
    terms = np.stack([_mm(cd, cw) + _mm(sd, sw), _mm(sd, cw) + _mm(cd, sw)], -1)
    return gamma(n) * terms + REF_EPS * d.sum()


def mix_bound(T, s, F, eF, H, W):
    """|device - exact| of the parts of G = (s T - F) / (H W), [16,16,2]: T [16,16,2] the table row, F the exact window of
    the centred frame and eF its project_bound.  g = fl(fl(fl(s T) - F') * inv'), F' = F + eF, inv' = fl(1 / (H W)):
    with a = s T (1 + d1), b = (a - F')(1 + d2), g = b inv (1 + d3)(1 + d4):
      |b - (s T - F)| <= (u |s T| + eF)(1 + u) + u |s T - F|,     |g - G| <= inv ((1 + gamma_2) |b - (s T - F)| + gamma_2 |s T - F|)"""
    sT = np.abs(float(s) * np.asarray(T, np.float64))
    diff = np.abs(float(s) * np.asarray(T, np.float64) - F)
    db = (U32 * sT + eF) * (1 + U32) + U32 * diff
    return ((1 + gamma(2)) * db + gamma(2) * diff) / (float(H) * W)


def recon_bound(G, d, dG=None, centred=True):
    """The reconstruction and normalisation of ONE frame in float64, with the bound on |device out_f (f_kind 0) - it|.
    G [16,16,2]: the window the reconstruction kernel reads (already divided by H W), taken as exact; dG (or None = 0): a
    bound on the parts of the device's G against it (mix_bound); d [H,W]: the centred frame.
    -> dict(ref [H,W] the normalised output, bound [H,W], range, ymax = max |y|).

    y = d + sum_l Q[r][l] e(l c / W), Q[r][l] = sum_k G[k][l] e(k r / H).  A part of y is a sum over (k, l) of two products
    per part of G, each at most |G part| in size, so sum |terms| <= S = sum (|Re G| + |Im G|) (+ sum dG).  Roundings on the
    longest chain: Q: the row twiddle, the product, the sum of the two products, z_k - 1 additions (z_k = the non-zero
    rows of a window column, 16 when dG is given); y: the column twiddle, the product, the sum of the two, z_l additions
    onto d (z_l = non-zero window columns).  d itself passes through the z_l additions and, when centred, its own
    subtraction.  Hence per part
      e_y = gamma_(6 + z_k - 1 + z_l) S + sum dG + gamma_(z_l + centred) |d| + REF_EPS (S + |d|).
    |y| = sqrtf(yr yr + yi yi): two squares, a sum, a root that is within 1 ulp = 2 u -- at most gamma_4 relative, after the
    parts' errors moved it by at most sqrt(2) e_y: e_m = sqrt(2) e_y + gamma_4 (|y| + sqrt(2) e_y).
    Normalisation, E = max e_m: min and max are each within E, range' = fl(max' - min') within 2 E + u range of range,
    scale' = 255 / range' within rel = t / (1 - t) + 3 u of 255 / range (t = the relative error of range'; the division
    counted as within 2.5 ulp), and o' = fl(fl(m' - min') * scale'):
      |o' - o| <= scale (e_m + E + u (m - min + e_m + E)) (1 + eta) + o eta,  eta = (1 + rel)(1 + u) - 1.
    The clamp to [0, 255] moves o' no further from o.  t >= 1/2 (a range lost in rounding error) gives an infinite bound:
    the test then says nothing, which is why the reconstruction cases must keep range >= ymax / 4."""
    G = np.asarray(G, np.float64)
    d = np.asarray(d, np.float64)
    H, W = d.shape
    eh, ew = _window_mats(H, W)
    y = d + _cmm(_cmm(eh.conj().T, G[..., 0] + 1j * G[..., 1]), ew.conj().T)
    nzg = (G != 0).any(-1)
    zk, zl = (16, 16) if dG is not None else (int(nzg.sum(0).max()), int(nzg.any(0).sum()))
    dG = np.zeros_like(G) if dG is None else np.asarray(dG, np.float64)
    S = np.abs(G).sum() + dG.sum()
    e_y = gamma(6 + max(zk - 1, 0) + zl) * S + dG.sum() + gamma(zl + (1 if centred else 0)) * np.abs(d) + REF_EPS * (S + np.abs(d))
    mag = np.abs(y)
    e_m = np.sqrt(2.0) * e_y + gamma(4) * (mag + np.sqrt(2.0) * e_y) + 1e-18
    E = e_m.max()
    lo, hi = mag.min(), mag.max()
    rng = hi - lo
    res = dict(range=rng, ymax=hi)
    if not rng > DBL_EPSILON:
        res.update(ref=np.zeros_like(mag), bound=np.full(mag.shape, np.inf if E > 0 else 0.0))
        return res
    ref = np.clip((mag - lo) * (255.0 / rng), 0, 255)
    t = (2 * E + U32 * (rng + 2 * E)) / rng
    if t >= 0.5:
        res.update(ref=ref, bound=np.full(mag.shape, np.inf))
        return res
    eta = (1 + t / (1 - t) + 3 * U32) * (1 + U32) - 1
    m = mag - lo
    bound = (255.0 / rng) * (e_m + E + U32 * (m + e_m + E)) * (1 + eta) + ref * eta + REF_EPS * 255
    res.update(ref=ref, bound=bound)
    return res


def apply_bound(f, table_row, s):
    """spnet_bandpass_apply of one frame f [H,W] (pixel units, the float32 values the kernel reads) with window table_row
    [16,16,2] and scale s, end to end: projection of the centred frame (project_bound), the mix (mix_bound), reconstruction
    and normalisation (recon_bound with the exact G as reference).  ref equals mixed(f, table_row, s)."""
    f = np.asarray(f, np.float64)
    H, W = f.shape
    d = f - f[0, 0]
    Fc = window(d)
    F = np.stack([Fc.real, Fc.imag], -1)
    integer = bool(np.all(f == np.rint(f)))                      # integers below 2^24 subtract exactly
    eF = project_bound(d, centred=not integer)
    dG = mix_bound(table_row, s, F, eF, H, W)
    G = (float(s) * np.asarray(table_row, np.float64) - F) / (float(H) * W)
    return recon_bound(G, d, dG=dG, centred=not integer)


def ratio(err, bound):
    """largest observed error / bound; 0 / 0 counts as 0, anything above a zero bound as inf"""
    err, bound = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bound, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max())


# ---- the cases, shared by the CPU tests (the bounds hold for the emulation) and the GPU tests (and for the device) --------
IMPULSE = 200.0
S_VALUES = (0.0, 0.5, 3.0 * (1.0 - 2.0 ** -24))
# reconstruction alone: (k, l, re, im) of the table row's non-zero coefficients, corners and edges of the window, one at
# (0, 0) that dominates: |y| stays within 1 +- 0.6 of it, so the range is a large part of max |y|
RECON_CASES = [
    [(0, 0, 1.0, 0.0), (-8, -8, 0.36, -0.48)],
    [(0, 0, 0.6, 0.8), (7, 7, 0.3, 0.0), (-8, 7, 0.0, -0.3)],
    [(0, 0, -1.0, 0.0), (0, -8, 0.15, 0.0), (7, 0, 0.0, 0.15), (-8, 0, -0.09, 0.12)],
]


def impulse_frame(H, W, r, c, A=IMPULSE, dtype=np.float32):
    f = np.zeros((H, W), dtype)
    f[r, c] = A
    return f


def recon_table(H, W):
    """[3,16,16,2] float32: RECON_CASES scaled to 100 grey levels at the (0, 0) coefficient after the division by H W"""
    t = np.zeros((len(RECON_CASES), 16, 16, 2), np.float32)
    for i, case in enumerate(RECON_CASES):
        for k, l, re, im in case:
            t[i, k + 8, l + 8] = (100.0 * H * W * re, 100.0 * H * W * im)
    return t


def dense_frames(N, H, W, seed):
    """integer-valued noise in [0, 255]"""
    return np.random.RandomState(seed).randint(0, 256, (N, H, W)).astype(np.float32)


def dense_table(n, H, W, seed):
    """a window table that is no projection of anything: every part drawn on its own, of the size a real frame's low
    frequencies have (up to ~ 20 grey levels per coefficient after the division by H W)"""
    return (np.random.RandomState(seed).normal(0, 20.0, (n, 16, 16, 2)) * (H * W)).astype(np.float32)
