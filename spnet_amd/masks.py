"""Ring-count segmentation masks from ellipse rows, and a pixel-level metric on them (csrc/masks.hip).

The reference's roadmap (segmentation/README.md) names "segmentation masks from ellipses", the ring count stored as an
integer ("multiply ring counts by 10 & truncate"), as the bridge to its successor; it holds no script that does it, so the
value map below is those words, not a pinned reference output.

THE RULE (include/spnet_hip.h states it for the kernel).  A mask is uint8 [H, W], background 0, painted from
rows (cx, cy, a, b, angle_deg, rings) in order; the LAST row that contains a pixel gives its value.  Per row, in whole numbers:

  cxq, cyq, aq, bq = rint(16 v)                      1/16 pixel, ties to even
  c, s = rint(2^14 cos(t)), rint(2^14 sin(t))        t = (-angle_deg) * (pi / 180), fp64 (image y points down)
  value = min(255, max(0, trunc(10 * rings)))        fp64

Pixel (x, y) has its centre at (16 x + 8, 16 y + 8); with dx, dy from (cxq, cyq), u = dx c + dy s, v = -dx s + dy c it is
inside iff (u bq)^2 + (v aq)^2 <= (aq bq 2^14)^2, evaluated exactly.  A row paints nothing if one of its six values is not
finite, if aq <= 0 or bq <= 0, or if |cx|, |cy|, a or b is 32,768 or more.  A row of value 0 paints zeros.

  ring_masks_device       rows -> uint8 [B,H,W] on the GPU (one launch)
  masks_from_predictions  de-normalised grids [B, 576] -> the same, one row per predictor
  compare_masks_device    two mask stacks -> five pixel counts and three ratios
  write_masks             PNG files, by Pillow or by the device encoder (png.write_png_device)
  ring_masks_host         the rule in numpy (exact; slow): what the product uses where there is no GPU

Nothing here imports torch or the HIP library until a device function is called.
"""
import math

import numpy as np

from .augmentation import MAX_OBJECTS, pad_metadata

SUBPIXEL = 16
CENTER = 8
TRIG_ONE = 1 << 14
COORD_LIMIT = 32768.0
MAX_K = 128                 # csrc/masks.hip MK_MAX_K
MAX_DIM = 16384
COUNT_NAMES = ("bg_bg", "hit", "miss", "pred_only", "true_only")
DEFAULT_TOL = 5             # half a ring, the window calc_errors uses


# ----------------------------------------------------------------------------- the rule on the host
def quantise_row(row):
    """(cxq, cyq, aq, bq, c, s, value) of one row as Python ints, or None when the row paints nothing."""
    cx, cy, a, b, ang, rings = (float(v) for v in row)
    if not all(math.isfinite(v) for v in (cx, cy, a, b, ang, rings)):
        return None
    if not (abs(cx) < COORD_LIMIT and abs(cy) < COORD_LIMIT and a < COORD_LIMIT and b < COORD_LIMIT):
        return None
    aq, bq = round(16.0 * a), round(16.0 * b)                 # round(): ties to even, as rint
    if aq <= 0 or bq <= 0:
        return None
    t = (-ang) * (math.pi / 180.0)
    t10 = 10.0 * rings
    value = 255 if t10 >= 255.0 else 0 if t10 <= 0.0 else int(t10)
    return (round(16.0 * cx), round(16.0 * cy), aq, bq, round(TRIG_ONE * math.cos(t)), round(TRIG_ONE * math.sin(t)), value)


def row_box(row):
    """The pixel box (x0, y0, x1, y1), inclusive, outside which the row paints nothing (the kernel's culling box; the
    argument that it holds every painted pixel is in csrc/masks.hip)."""
    cx, cy, a, b = (float(v) for v in row[:4])
    A = max(a, b)
    R = math.ceil(A) + 1 + (1 if A > 16384.0 else 0)
    fx, fy = math.floor(cx), math.floor(cy)
    return fx - R, fy - R, fx + R, fy + R


def _paint_row_host(mask, row, use_box=True):
    q = quantise_row(row)
    if q is None:
        return
    cxq, cyq, aq, bq, c, s, value = q
    H, W = mask.shape
    x0, y0, x1, y1 = 0, 0, W - 1, H - 1
    if use_box:
        bx0, by0, bx1, by1 = row_box(row)
        x0, y0, x1, y1 = max(x0, bx0), max(y0, by0), min(x1, bx1), min(y1, by1)
    if x1 < x0 or y1 < y0:
        return
    dx = (SUBPIXEL * np.arange(x0, x1 + 1, dtype=np.int64) + CENTER - cxq)[None, :]
    dy = (SUBPIXEL * np.arange(y0, y1 + 1, dtype=np.int64) + CENTER - cyq)[:, None]
    P = (dx * c + dy * s) * bq                                # |.| < 2^54: exact in int64
    Q = (dy * c - dx * s) * aq
    R = (aq * bq) << 14
    # float64 decides where it can (its relative error is below 1e-15), Python integers the pixels within 1e-9 of the rim
    level = (P.astype(np.float64) ** 2 + Q.astype(np.float64) ** 2) / float(R) ** 2
    inside = level < 1.0 - 1e-9
    RR = R * R
    for j, i in zip(*np.nonzero(np.abs(level - 1.0) <= 1e-9)):
        inside[j, i] = int(P[j, i]) ** 2 + int(Q[j, i]) ** 2 <= RR
    mask[y0:y1 + 1, x0:x1 + 1][inside] = value


def _host_rows(rows, count=None):
    if count is None:
        meta = rows
        if isinstance(meta, tuple):
            rows, count = meta
        else:
            rows, count = pad_metadata(meta, max(MAX_OBJECTS, max((len(m) for m in meta), default=0)))
    rows = np.asarray(rows, np.float64)
    count = np.asarray(count).astype(np.int64)
    if rows.ndim != 3 or rows.shape[2] != 6 or count.shape != (rows.shape[0],):
        raise ValueError("masks: rows are float64 [B,K,6] with count [B], got %s and %s" % (rows.shape, count.shape))
    return rows, count


def _check_size(H, W, K=1):
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM and 1 <= K <= MAX_K):
        raise ValueError("masks: H, W are 1 .. %d and K is 1 .. %d, got H %d, W %d, K %d" % (MAX_DIM, MAX_K, H, W, K))


def ring_masks_host(rows, count=None, H=384, W=512, use_box=True):
    """The rule in numpy: rows float64 [B,K,6] with count [B] (clamped to 0 .. K), or a list of label lists.  Returns uint8
    [B,H,W].  Exact (pixels near a rim are decided in Python integers), and slow.  use_box=False tests every pixel of the
    frame against every row: the same masks, since the box holds every painted pixel."""
    rows, count = _host_rows(rows, count)
    B, K = rows.shape[:2]
    H, W = int(H), int(W)
    _check_size(H, W, max(K, 1))
    out = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        for k in range(min(max(int(count[b]), 0), K)):
            _paint_row_host(out[b], rows[b, k], use_box)
    return out


def metrics_from_counts(bg_bg, hit, miss, pred_only, true_only):
    """The dict compare_masks_device returns, from the five summed counts.  A ratio whose denominator is 0 is None."""
    c = dict(zip(COUNT_NAMES, (int(bg_bg), int(hit), int(miss), int(pred_only), int(true_only))))
    total = sum(c.values())
    both = c["hit"] + c["miss"]
    union = both + c["pred_only"] + c["true_only"]
    c["pixel_acc"] = (c["bg_bg"] + c["hit"]) / total if total else None
    c["object_iou"] = both / union if union else None
    c["ring_acc"] = c["hit"] / both if both else None
    return c


def compare_masks_host(pred, truth, tol=DEFAULT_TOL):
    """compare_masks_device in numpy, for where there is no GPU."""
    p, t = np.asarray(pred, np.uint8).astype(np.int64), np.asarray(truth, np.uint8).astype(np.int64)
    if p.shape != t.shape:
        raise ValueError("compare_masks: shapes %s and %s" % (p.shape, t.shape))
    _check_tol(tol)
    both, close = (p > 0) & (t > 0), np.abs(p - t) <= tol
    return metrics_from_counts(np.count_nonzero((p == 0) & (t == 0)), np.count_nonzero(both & close),
                               np.count_nonzero(both & ~close), np.count_nonzero((p > 0) & (t == 0)),
                               np.count_nonzero((p == 0) & (t > 0)))


def _check_tol(tol):
    if not (isinstance(tol, (int, np.integer)) and 0 <= tol <= 255):
        raise ValueError("compare_masks: tol is an integer 0 .. 255, got %r" % (tol,))


# ----------------------------------------------------------------------------- the device side
def _default_device(device):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("masks: the device rasteriser needs a GPU (ring_masks_host is the host rule)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def ring_masks_device(rows, count=None, H=384, W=512, out=None, device=None):
    """uint8 [B,H,W] device tensor of masks, one launch on the current stream.  rows: a float64 device tensor [B,K,6] with
    count int32 [B] (augmentation.pad_metadata's / fake_espi.rows_from_params' layout, K <= 128), or a host list of label
    lists (or pad_metadata's pair), which is padded and uploaded.  out: a contiguous uint8 device tensor [B,H,W] to fill."""
    import torch
    from . import _lib as L
    if not isinstance(rows, torch.Tensor):
        r, c = _host_rows(rows, count)
        dev = _default_device(device if out is None else out.device)
        rows, count = torch.from_numpy(np.ascontiguousarray(r)).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev)
    if not (isinstance(count, torch.Tensor) and rows.is_cuda and count.is_cuda and rows.dtype == torch.float64 and
            count.dtype == torch.int32 and rows.dim() == 3 and rows.shape[2] == 6 and tuple(count.shape) == (rows.shape[0],)):
        raise TypeError("ring_masks_device expects rows float64 [B,K,6] and count int32 [B] on the device")
    rows, count = rows.contiguous(), count.contiguous()
    B, K = int(rows.shape[0]), int(rows.shape[1])
    H, W = int(H), int(W)
    _check_size(H, W, K)
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.uint8, device=rows.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.uint8 and out.device == rows.device and
              tuple(out.shape) == (B, H, W) and out.is_contiguous()):
        raise ValueError("ring_masks_device: out is a contiguous uint8 tensor [%d,%d,%d] on %s" % (B, H, W, rows.device))
    if B:
        with torch.cuda.device(rows.device):
            L.spnet_ring_masks(rows.data_ptr(), count.data_ptr(), B, K, H, W, out.data_ptr(), L.current_stream())
    return out


def prediction_rows(Y_denorm, xp=np):
    """[B, 8 n] de-normalised grids -> rows float64 [B, n, 6] = (cx, cy, a, b, deg(atan2(sin2t, cos2t) / 2), rings) per
    predictor, a = 0 where noobj >= 0.5 (such a row paints nothing).  xp: numpy, or torch for a tensor (any device)."""
    Y = Y_denorm.double() if xp is not np else np.asarray(Y_denorm, np.float64)
    g = Y.reshape(Y.shape[0], -1, 8)
    cx, cy, a, b, cos2t, sin2t, noobj, rings = (g[..., i] for i in range(8))
    if xp is np:
        angle = np.rad2deg(np.arctan2(sin2t, cos2t) / 2.0)
        a = np.where(noobj >= 0.5, 0.0, a)
    else:
        angle = xp.rad2deg(xp.atan2(sin2t, cos2t) / 2.0)
        a = xp.where(noobj >= 0.5, xp.zeros_like(a), a)
    return xp.stack([cx, cy, a, b, angle, rings], -1)


def masks_from_predictions(Y_denorm, H=384, W=512, device=None):
    """uint8 [B,H,W] device masks of de-normalised grids [B, 576] (host array or tensor on any device): one row per
    predictor (K = 72 in the default grid), built with torch ops on the device and painted by the same kernel."""
    import torch
    if not isinstance(Y_denorm, torch.Tensor):
        Y_denorm = torch.from_numpy(np.ascontiguousarray(np.asarray(Y_denorm)))
    if not Y_denorm.is_cuda:
        Y_denorm = Y_denorm.to(_default_device(device))
    if Y_denorm.dim() != 2 or Y_denorm.shape[1] % 8 or not Y_denorm.shape[1]:
        raise ValueError("masks_from_predictions expects [B, 8 n] grids, got %s" % (tuple(Y_denorm.shape),))
    rows = prediction_rows(Y_denorm, torch).contiguous()
    B, K = int(rows.shape[0]), int(rows.shape[1])
    count = torch.full((B,), K, dtype=torch.int32, device=rows.device)
    return ring_masks_device(rows, count, H, W)


def mask_counts_device(pred, truth, tol=DEFAULT_TOL):
    """int32 device tensor [N,5] of per-frame counts (COUNT_NAMES) of two uint8 device stacks [N, ...] of one shape."""
    import torch
    from . import _lib as L
    for t in (pred, truth):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() >= 2):
            raise TypeError("compare_masks_device expects two uint8 device tensors [N, ...]")
    if pred.shape != truth.shape or pred.device != truth.device:
        raise ValueError("compare_masks_device: %s on %s against %s on %s"
                         % (tuple(pred.shape), pred.device, tuple(truth.shape), truth.device))
    _check_tol(tol)
    pred, truth = pred.contiguous(), truth.contiguous()
    N = int(pred.shape[0])
    counts = torch.zeros((N, 5), dtype=torch.int32, device=pred.device)
    n_pixels = pred.numel() // N if N else 0
    if N and n_pixels:
        with torch.cuda.device(pred.device):
            L.spnet_mask_compare(pred.data_ptr(), truth.data_ptr(), N, n_pixels, int(tol), counts.data_ptr(), L.current_stream())
    return counts


def compare_masks_device(pred, truth, tol=DEFAULT_TOL):
    """Pixel-level comparison of predicted and true masks (uint8 device tensors [N,H,W]): the five counts summed over the
    frames -- bg_bg, hit (both above 0 and within tol), miss (both above 0, further apart), pred_only, true_only -- and
    pixel_acc = (bg_bg + hit) / total, object_iou = (hit + miss) / (hit + miss + pred_only + true_only), ring_acc = hit /
    (hit + miss); a ratio whose denominator is 0 is None.  tol = 5 is half a ring."""
    return metrics_from_counts(*mask_counts_device(pred, truth, tol).sum(0).tolist())      # torch sums int32 in int64


# ----------------------------------------------------------------------------- files
def write_masks(masks, paths, png="pillow", pool=None):
    """One 8-bit grey PNG per mask.  masks: uint8 [N,H,W], host array or device tensor.  png: "pillow" (default), or
    "device" / "device-lz": encoded where the masks are by png.write_png_device (the LZ77 stage suits flat regions).
    pool: a caller's ThreadPoolExecutor for the device modes."""
    paths = list(paths)
    if png not in ("pillow", "device", "device-lz"):
        raise ValueError("write_masks: png is 'pillow', 'device' or 'device-lz', got %r" % (png,))
    if len(masks) != len(paths):
        raise ValueError("write_masks: %d masks, %d paths" % (len(masks), len(paths)))
    if png == "pillow":
        from PIL import Image
        host = masks.cpu().numpy() if hasattr(masks, "is_cuda") else np.asarray(masks)
        if host.dtype != np.uint8 or host.ndim != 3:
            raise TypeError("write_masks expects uint8 [N,H,W]")
        for m, p in zip(host, paths):
            Image.fromarray(m).save(p)
        return
    import torch
    from .png import write_png_device
    if not isinstance(masks, torch.Tensor):
        masks = torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint8))
    if not masks.is_cuda:
        masks = masks.to(_default_device(None))
    write_png_device(masks, paths, pool=pool, lz77=(png == "device-lz"))
