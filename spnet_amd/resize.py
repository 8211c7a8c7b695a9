"""PIL.Image.resize(size, ANTIALIAS) of one-channel 8-bit frames, bit for bit -- the resize of the reference's input codec
(spnet/utils.py:335-337) as integer tap tables (host, numpy) + one HIP launch per batch (csrc/resize.hip).

Pillow's 8-bit resampler (Resample.c) is integer arithmetic once its taps exist.  For one axis, input length I, output
length O, Lanczos (a = 3):

  scale = I / O, fs = max(scale, 1), support = 3 * fs, ss = 1 / fs; for output index o:
  center = (o + 0.5) * scale, lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), I),
  w[j] = L((j + lo - center + 0.5) * ss), j < hi - lo, L(x) = sinc(x) * sinc(x / 3) on -3 <= x < 3, else 0; float64,
  divided by their sum (accumulated in tap order);
  k[j] = int(w[j] * 2**22 + 0.5) (w >= 0) | int(w[j] * 2**22 - 0.5) (w < 0)                       -- int32 taps
  out = clip((2**21 + sum_j pixel[lo + j] * k[j]) >> 22, 0, 255)          -- int32 accumulator, arithmetic shift

horizontally first, then vertically over the uint8 result of the first pass; a pass whose size does not change is
skipped.  lanczos_taps() is the first three lines, resize_u8_host() the rest in numpy (tests, documentation),
resize_u8_device() the same on the GPU.  Nothing here imports torch or the HIP library until the device entry is called.
"""
import math
from functools import lru_cache

import numpy as np

PRECISION_BITS = 32 - 8 - 2
TAP_LIMIT = 1 << 23          # the kernel multiplies with 24-bit operands: |tap| < 2**23 (a normalised tap is about <= 1.0 = 2**22)


def _lanczos(x):
    if not (-3.0 <= x < 3.0):
        return 0.0
    if x == 0.0:
        return 1.0
    a = x * math.pi
    b = (x / 3.0) * math.pi     # sinc(x / 3): x / 3 is formed first, then scaled by pi
    return (math.sin(a) / a) * (math.sin(b) / b)


@lru_cache(maxsize=64)
def _taps_cached(I, O):
    scale = I / O
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    rows = []
    for o in range(O):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), I)
        w = [_lanczos((j + lo - center + 0.5) * ss) for j in range(hi - lo)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((lo, [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w]))
    taps = max(len(k) for _, k in rows)
    tab = np.zeros((O, 2 + taps), np.int32)
    for o, (lo, k) in enumerate(rows):
        tab[o, 0], tab[o, 1] = lo, len(k)
        tab[o, 2:2 + len(k)] = k
    if np.abs(tab[:, 2:]).max(initial=0) >= TAP_LIMIT:
        raise ValueError("lanczos_taps(%d, %d): a tap does not fit 24 bits" % (I, O))
    tab.setflags(write=False)
    return tab


def lanczos_taps(I, O):
    """int32 [O][2 + taps]: (first input index, tap count, taps ..., zero padded) of Pillow's Lanczos resampling of an
    axis of length I to length O; taps = the largest tap count of the pair.  Read-only, cached."""
    I, O = int(I), int(O)
    if I < 1 or O < 1:
        raise ValueError("lanczos_taps: lengths must be >= 1, got %d -> %d" % (I, O))
    return _taps_cached(I, O)


def accumulator_bound(tab):
    """Largest |value| the int32 accumulator of one output can reach with this table: 255 * sum|k| + 2**21."""
    return 255 * int(np.abs(tab[:, 2:].astype(np.int64)).sum(axis=1).max()) + (1 << (PRECISION_BITS - 1))


def _pass_last_axis(a, tab):
    """One resampling pass over the last axis of uint8 `a` with int32 wrap-around accumulation, as C computes it."""
    O = tab.shape[0]
    out = np.empty(a.shape[:-1] + (O,), np.uint8)
    for o in range(O):
        lo, cnt = int(tab[o, 0]), int(tab[o, 1])
        acc = (a[..., lo:lo + cnt].astype(np.int64) * tab[o, 2:2 + cnt].astype(np.int64)).sum(axis=-1) + (1 << (PRECISION_BITS - 1))
        acc = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)                 # the C `int` accumulator
        out[..., o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def _size(size):
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    OH, OW = size
    return int(OH), int(OW)


def resize_u8_host(frames, size):
    """numpy restatement of Image.fromarray(f).resize((OW, OH), Image.LANCZOS) for uint8 frames [..., H, W]; size =
    (OH, OW) or one int.  Horizontal pass, then vertical over its uint8 result; an unchanged axis is not resampled."""
    a = np.ascontiguousarray(frames)
    if a.dtype != np.uint8 or a.ndim < 2:
        raise TypeError("resize_u8_host expects uint8 frames [..., H, W]")
    OH, OW = _size(size)
    H, W = a.shape[-2:]
    if OW != W:
        a = _pass_last_axis(a, lanczos_taps(W, OW))
    if OH != H:
        a = np.swapaxes(_pass_last_axis(np.swapaxes(a, -1, -2), lanczos_taps(H, OH)), -1, -2)
    return np.ascontiguousarray(a)


# ----------------------------------------------------------------------------- device
_DEVICE_TABLES = {}


def _device_table(I, O, dev):
    """Device copy of lanczos_taps(I, O) (None for an unchanged axis: the kernel skips that pass), cached per device."""
    if I == O:
        return None, 0
    key = (I, O, str(dev))
    hit = _DEVICE_TABLES.get(key)
    if hit is None:
        import torch
        tab = lanczos_taps(I, O)
        hit = _DEVICE_TABLES[key] = (torch.from_numpy(np.array(tab)).to(dev), tab.shape[1] - 2)
    return hit


def warm(I, O, device):
    """Put the table of one axis pair on `device` now (a synchronising host-to-device copy, once per pair and device):
    afterwards resize_u8_device over that pair only enqueues, e.g. inside a graph capture.  Returns (table, taps)."""
    import torch
    return _device_table(int(I), int(O), torch.device(device))


def resize_u8_device(frames_u8, size, out_f=None, out_u8=None):
    """Device tensors: uint8 frames [N, H, W(, 1)] -> [N, OH, OW] resized as Pillow does, in ONE launch on the current
    stream.  out_u8 (uint8) and / or out_f (float32 network input, == spnet_u8_to_input of the uint8 result) are written
    when given; with neither, a new uint8 tensor is made.  Returns (out_u8, out_f).  Enqueue-only: nothing is
    synchronised once the tables of the size pair are on the device (the first call per pair and device copies them
    from the host, which synchronises: call warm(W, OW, dev) and warm(H, OH, dev) before capturing into a graph)."""
    import torch
    from . import _lib as L
    OH, OW = _size(size)
    if frames_u8.dtype != torch.uint8 or not frames_u8.is_cuda:
        raise TypeError("resize_u8_device expects a uint8 device tensor")
    if frames_u8.dim() == 4 and frames_u8.shape[-1] == 1:
        frames_u8 = frames_u8[..., 0]
    if frames_u8.dim() != 3:
        raise ValueError("resize_u8_device expects frames [N, H, W(, 1)], got %s" % (tuple(frames_u8.shape),))
    frames_u8 = frames_u8.contiguous()
    N, H, W = (int(v) for v in frames_u8.shape)
    dev = frames_u8.device
    if out_f is None and out_u8 is None:
        out_u8 = torch.empty((N, OH, OW), dtype=torch.uint8, device=dev)
    for t, dt, name in ((out_u8, torch.uint8, "out_u8"), (out_f, torch.float32, "out_f")):
        if t is None:
            continue
        if t.dtype != dt or t.device != dev or not t.is_contiguous() or t.numel() != N * OH * OW:
            raise ValueError("resize_u8_device: %s must be a contiguous %s tensor of %d x %d x %d elements on %s"
                             % (name, dt, N, OH, OW, dev))
    if N == 0:
        return out_u8, out_f
    xt, xtaps = _device_table(W, OW, dev)
    yt, ytaps = _device_table(H, OH, dev)
    with torch.cuda.device(dev):
        L.spnet_resize_u8(frames_u8.data_ptr(), N, H, W, L.ptr(xt), xtaps, L.ptr(yt), ytaps, OH, OW, L.ptr(out_u8),
                          L.ptr(out_f), L.current_stream())
    return out_u8, out_f
