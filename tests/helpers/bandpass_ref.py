"""Float64 restatements of the reference's band-pass mix-up (spnet/augmentation.py:10-62) for the tests.

literal():   the reference's steps as written, with cv2's (H, W, 2) real / imaginary layout emulated in numpy: the
             fftshift over ALL axes (which also swaps the two planes), the 0/1 uint8 mask on both planes, the unscaled
             inverse, cv2.magnitude, cv2.normalize(NORM_MINMAX) and np.clip.
windowed():  the same result from the 16 x 16 window alone (the formulation csrc/bandpass.hip computes).
fft_pipeline(dtype=np.float32): literal() run through scipy.fft in single precision -- the yardstick for the device's
             error against float64.
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


def window(img):
    """F[k, l] for k, l in [-8, 8): [16,16] complex, row k + 8, column l + 8."""
    img = np.asarray(img, np.float64)
    eh, ew = _window_mats(*img.shape)
    return eh @ img @ ew


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
