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

THE WAY BACK (csrc/mask_fit.hip; include/spnet_hip.h "Mask fitting"): ellipse rows from a mask.  Two pixels are
adjacent iff they are 8-neighbours, both nonzero, and their values differ by at most join_tol (0 .. 255; 0 joins equal values
only, 255 anything nonzero).  A component is a connected component of that graph; its label, for every one of its pixels, is
1 + (y W + x) of its FIRST pixel in raster order, background 0; components are ordered by label; each has eight int64 sums
(n, sum x, sum y, sum x^2, sum y^2, sum xy, sum v, first = label - 1).  rows_from_sums turns the sums into rows in float64, on
the host, for the device path and the host path alike -- so the two agree bit for bit.

  label_components_device / _host     uint8 [B,H,W] -> int32 labels [B,H,W]
  component_sums_device / _host       -> (n_components int32 [B] -- the TRUE count --, sums int64 [B,C,8])
  rows_from_sums                      sums -> (rows float64 [B,C,6], count int32 [B]): pad_metadata's layout
  ellipses_from_masks_device / _host  masks -> (rows, count)
  read_masks                          PNG files -> uint8 [N,H,W], by Pillow or by png.read_png_device

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


def inside_row_host(row, H, W, use_box=True, q=None):
    """The pixels of an H x W frame inside one row, as (x0, y0, bool [h, w]): the window's corner and the test on every
    pixel of the window (the row's box cut to the frame; the whole frame without use_box).  None where the row paints
    nothing or its window is empty.  q: quantise_row(row), if the caller has it."""
    q = quantise_row(row) if q is None else q
    if q is None:
        return None
    cxq, cyq, aq, bq, c, s, _ = q
    x0, y0, x1, y1 = 0, 0, W - 1, H - 1
    if use_box:
        bx0, by0, bx1, by1 = row_box(row)
        x0, y0, x1, y1 = max(x0, bx0), max(y0, by0), min(x1, bx1), min(y1, by1)
    if x1 < x0 or y1 < y0:
        return None
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
    return x0, y0, inside


def _paint_row_host(mask, row, use_box=True):
    q = quantise_row(row)
    win = inside_row_host(row, mask.shape[0], mask.shape[1], use_box, q)
    if win is None:
        return
    x0, y0, inside = win
    mask[y0:y0 + inside.shape[0], x0:x0 + inside.shape[1]][inside] = q[6]


def host_rows(rows, count=None):
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


def check_size(H, W, K=1):
    if not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM and 1 <= K <= MAX_K):
        raise ValueError("masks: H, W are 1 .. %d and K is 1 .. %d, got H %d, W %d, K %d" % (MAX_DIM, MAX_K, H, W, K))


def ring_masks_host(rows, count=None, H=384, W=512, use_box=True):
    """The rule in numpy: rows float64 [B,K,6] with count [B] (clamped to 0 .. K), or a list of label lists.  Returns uint8
    [B,H,W].  Exact (pixels near a rim are decided in Python integers), and slow.  use_box=False tests every pixel of the
    frame against every row: the same masks, since the box holds every painted pixel."""
    rows, count = host_rows(rows, count)
    B, K = rows.shape[:2]
    H, W = int(H), int(W)
    check_size(H, W, max(K, 1))
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
def host_array(a):
    """A device tensor brought to the host; anything else through np.asarray."""
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def default_device(device):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("masks: the device rasteriser needs a GPU (ring_masks_host is the host rule)")
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


ROWS_TEXT = "%s expects rows float64 [%s,K,6] and count int32 [%s] on the device"


def device_rows(rows, count, device, text, every_row=False, upload=True):
    """The gate of every entry that reads rows on the device: contiguous (rows float64 [N,K,6], count int32 [N], N, K).
    Host input -- an array with its count, pad_metadata's pair or a list of label lists -- goes through host_rows and is
    uploaded to `device`, unless upload is False (then it is an error like any other).  every_row: count None means that
    every row counts (without it, None with an array is host_rows' business and None with a tensor is an error).
    TypeError(text) for anything else."""
    import torch
    if isinstance(rows, torch.Tensor):
        if count is None and every_row:                     # made where the rows are: nothing leaves the device
            count = torch.full((int(rows.shape[0]),), int(rows.shape[1]) if rows.dim() == 3 else 0, dtype=torch.int32,
                               device=rows.device)
    elif upload:
        if count is None and every_row and not isinstance(rows, (list, tuple)):
            count = np.full(np.asarray(rows).shape[0], np.asarray(rows).shape[1], np.int64)
        r, c = host_rows(rows, count)
        dev = default_device(device)
        rows, count = torch.from_numpy(np.ascontiguousarray(r)).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev)
    if not (isinstance(rows, torch.Tensor) and isinstance(count, torch.Tensor) and rows.is_cuda and count.is_cuda and
            rows.dtype == torch.float64 and count.dtype == torch.int32 and rows.dim() == 3 and rows.shape[2] == 6 and
            tuple(count.shape) == (rows.shape[0],)):
        raise TypeError(text)
    return rows.contiguous(), count.contiguous(), int(rows.shape[0]), int(rows.shape[1])


def check_grids(Y, who, batch="N"):
    if Y.ndim != 2 or Y.shape[1] % 8 or not Y.shape[1]:
        raise ValueError("%s expects [%s, 8 n] grids, got %s" % (who, batch, tuple(Y.shape)))


def device_grids(Y_denorm, device, who, batch="N"):
    """De-normalised grids [N, 8 n] as a device tensor: a host array or a tensor elsewhere is uploaded to `device`."""
    import torch
    if not isinstance(Y_denorm, torch.Tensor):
        Y_denorm = torch.from_numpy(np.ascontiguousarray(np.asarray(Y_denorm)))
    if not Y_denorm.is_cuda:
        Y_denorm = Y_denorm.to(default_device(device))
    check_grids(Y_denorm, who, batch)
    return Y_denorm


def ring_masks_device(rows, count=None, H=384, W=512, out=None, device=None):
    """uint8 [B,H,W] device tensor of masks, one launch on the current stream.  rows: a float64 device tensor [B,K,6] with
    count int32 [B] (augmentation.pad_metadata's / fake_espi.rows_from_params' layout, K <= 128), or a host list of label
    lists (or pad_metadata's pair), which is padded and uploaded.  out: a contiguous uint8 device tensor [B,H,W] to fill."""
    import torch
    from . import _lib as L
    rows, count, B, K = device_rows(rows, count, device if out is None else out.device, ROWS_TEXT % ("ring_masks_device", "B", "B"))
    H, W = int(H), int(W)
    check_size(H, W, K)
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
    rows = prediction_rows(device_grids(Y_denorm, device, "masks_from_predictions", "B"), torch)
    count = torch.full((int(rows.shape[0]),), int(rows.shape[1]), dtype=torch.int32, device=rows.device)
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
        host = host_array(masks)
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
        masks = masks.to(default_device(None))
    write_png_device(masks, paths, pool=pool, lz77=(png == "device-lz"))


# ----------------------------------------------------------------------------- the way back: components, sums, rows
N_SUMS = 8
SUM_NAMES = ("n", "sx", "sy", "sxx", "syy", "sxy", "sv", "first")


def _check_fit(join_tol, max_components=1, min_pixels=1):
    if not (isinstance(join_tol, (int, np.integer)) and 0 <= join_tol <= 255):
        raise ValueError("masks: join_tol is an integer 0 .. 255, got %r" % (join_tol,))
    if not (isinstance(max_components, (int, np.integer)) and 1 <= max_components <= MAX_K):
        raise ValueError("masks: max_components is an integer 1 .. %d, got %r" % (MAX_K, max_components))
    if not (isinstance(min_pixels, (int, np.integer)) and min_pixels >= 1):
        raise ValueError("masks: min_pixels is an integer >= 1, got %r" % (min_pixels,))


def _host_masks(masks):
    m = np.asarray(masks)
    if m.dtype != np.uint8 or m.ndim != 3:
        raise TypeError("masks: expected uint8 [B,H,W], got %s %s" % (m.dtype, m.shape))
    if m.shape[0]:
        check_size(m.shape[1], m.shape[2])
    return m


def _label_frame_host(mask, join_tol):
    """One frame.  A union-find over RUNS: a run is a maximal stretch of a row whose consecutive pixels are adjacent; runs
    are numbered in raster order of their first pixel, two runs of neighbouring rows are linked where a pixel of one is
    adjacent (by the rule: value test included) to a pixel of the other, and every root is its tree's smallest run -- whose
    first pixel is the component's first pixel."""
    H, W = mask.shape
    v = mask.astype(np.int16)
    nz = v != 0
    if not nz.any():
        return np.zeros((H, W), np.int32)
    link_w = np.zeros((H, W), bool)
    link_w[:, 1:] = nz[:, 1:] & nz[:, :-1] & (np.abs(v[:, 1:] - v[:, :-1]) <= join_tol)
    start = (nz & ~link_w).ravel()
    first_pixel = np.flatnonzero(start)                          # of every run, ascending
    run_of = (np.cumsum(start) - 1).reshape(H, W)                # of every nonzero pixel (meaningless on background)
    ea, eb = [], []
    for cur, up in (((slice(1, None), slice(1, None)), (slice(None, -1), slice(None, -1))),       # NW
                    ((slice(1, None), slice(None)), (slice(None, -1), slice(None))),              # N
                    ((slice(1, None), slice(None, -1)), (slice(None, -1), slice(1, None)))):      # NE
        ok = nz[cur] & nz[up] & (np.abs(v[cur] - v[up]) <= join_tol)
        ea.append(run_of[cur][ok])
        eb.append(run_of[up][ok])
    n_runs = first_pixel.size
    pairs = np.unique(np.concatenate(ea).astype(np.int64) * n_runs + np.concatenate(eb))
    ea, eb = pairs // n_runs, pairs % n_runs
    parent = np.arange(n_runs, dtype=np.int64)
    while ea.size:                                               # every round merges at least one pair of trees
        ra, rb = parent[ea], parent[eb]                          # roots: the forest is flat at the top of a round
        differ = ra != rb
        if not differ.any():
            break
        np.minimum.at(parent, np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ])     # the larger root under a smaller
        while True:                                              # flatten: depths halve
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return np.where(nz, first_pixel[parent[run_of]] + 1, 0).astype(np.int32)


def label_components_host(masks, join_tol=0):
    """The labelling rule in numpy: uint8 [B,H,W] -> int32 [B,H,W].  What the product uses where there is no GPU."""
    masks = _host_masks(masks)
    _check_fit(join_tol)
    out = np.zeros(masks.shape, np.int32)
    for b in range(masks.shape[0]):
        out[b] = _label_frame_host(masks[b], int(join_tol))
    return out


def _sums_frame_host(mask, labels):
    """int64 [n,8] of one frame's components in label order (all of them)."""
    W = mask.shape[1]
    idx = np.flatnonzero(labels.ravel() > 0)
    if not idx.size:
        return np.zeros((0, N_SUMS), np.int64)
    lab = labels.ravel()[idx].astype(np.int64)
    order = np.argsort(lab, kind="stable")
    lab, idx = lab[order], idx[order]
    starts = np.flatnonzero(np.concatenate([[True], lab[1:] != lab[:-1]]))
    y, x = np.divmod(idx.astype(np.int64), W)
    v = mask.ravel()[idx].astype(np.int64)
    cols = [np.ones_like(x), x, y, x * x, y * y, x * y, v]
    return np.stack([np.add.reduceat(c, starts) for c in cols] + [lab[starts] - 1], 1)


def component_sums_host(masks, join_tol=0, max_components=MAX_K, labels=None):
    """(n_components int32 [B] -- the true count, which may exceed max_components --, sums int64 [B,C,8]: the first
    min(n, C) components of every frame in label order, the other slots zero).  labels: label_components_host's, if the
    caller has them."""
    masks = _host_masks(masks)
    _check_fit(join_tol, max_components)
    if labels is None:
        labels = label_components_host(masks, join_tol)
    labels = np.asarray(labels)
    if labels.shape != masks.shape:
        raise ValueError("component_sums: labels %s for masks %s" % (labels.shape, masks.shape))
    B, C = masks.shape[0], int(max_components)
    n, sums = np.zeros(B, np.int32), np.zeros((B, C, N_SUMS), np.int64)
    for b in range(B):
        s = _sums_frame_host(masks[b], labels[b])
        n[b] = s.shape[0]
        sums[b, :min(s.shape[0], C)] = s[:C]
    return n, sums


def rows_from_sums(sums, n_components, min_pixels=1):
    """Ellipse rows of components: (rows float64 [B,C,6] = (cx, cy, a, b, angle_deg, rings), count int32 [B]), in
    pad_metadata's layout.  The ONE float64 function of the fit, shared by the device path and the host path (numpy on the
    host; torch tensors are brought to the host and the result goes back to their device), so both give the same bits.
    With N = n, mx = sx / N, my = sy / N: mu20 = sxx / N - mx^2 + 1/12 (1/12: a pixel is a unit square), mu02 likewise,
    mu11 = sxy / N - mx my; l1 >= l2 the eigenvalues of [[mu20, mu11], [mu11, mu02]]; cx = mx + 0.5, cy = my + 0.5 (the
    painter puts pixel centres at x + 0.5); a = 2 sqrt(l1), b = 2 sqrt(max(l2, 0)) (a filled ellipse of semi-axis a has
    variance a^2 / 4); angle_deg = -deg(atan2(2 mu11, mu20 - mu02) / 2) (image y points down: the painter's convention);
    rings = sv / (10 N).  Only the first min(n_components, C) slots of a frame count; of those, components with fewer than
    min_pixels pixels are dropped, the rest are packed to the front in order, the rows behind them are zero."""
    as_torch = hasattr(sums, "is_cuda")
    if as_torch:
        import torch
        device = sums.device
        sums, n_components = sums.cpu().numpy(), n_components.cpu().numpy()
    s, n = np.asarray(sums), np.asarray(n_components)
    if s.dtype != np.int64 or s.ndim != 3 or s.shape[2] != N_SUMS or n.shape != (s.shape[0],):
        raise ValueError("rows_from_sums: sums are int64 [B,C,8] with n_components [B], got %s %s and %s"
                         % (s.dtype, s.shape, n.shape))
    _check_fit(0, min_pixels=min_pixels)
    B, C = s.shape[:2]
    slot = np.arange(C)[None, :]
    valid = (slot < np.minimum(n.astype(np.int64), C)[:, None]) & (s[..., 0] >= int(min_pixels))
    f = s.astype(np.float64)
    N = np.where(valid, f[..., 0], 1.0)
    mx, my = f[..., 1] / N, f[..., 2] / N
    mu20 = f[..., 3] / N - mx * mx + 1.0 / 12.0
    mu02 = f[..., 4] / N - my * my + 1.0 / 12.0
    mu11 = f[..., 5] / N - mx * my
    mean, half = 0.5 * (mu20 + mu02), 0.5 * (mu20 - mu02)
    r = np.sqrt(half * half + mu11 * mu11)
    a = 2.0 * np.sqrt(np.maximum(mean + r, 0.0))
    b = 2.0 * np.sqrt(np.maximum(mean - r, 0.0))
    angle = -np.degrees(0.5 * np.arctan2(2.0 * mu11, mu20 - mu02)) + 0.0          # + 0.0: no negative zero
    rings = f[..., 6] / (10.0 * N)
    rows = np.stack([mx + 0.5, my + 0.5, a, b, angle, rings], -1)
    order = np.argsort(~valid, axis=1, kind="stable")                             # kept components first, in order
    rows = np.take_along_axis(rows, order[..., None], 1)
    count = valid.sum(1).astype(np.int32)
    rows[slot >= count[:, None]] = 0.0
    if as_torch:
        return torch.from_numpy(rows).to(device), torch.from_numpy(count).to(device)
    return rows, count


def _overflow_check(n, C, overflow):
    if overflow not in ("raise", "truncate"):
        raise ValueError("masks: overflow is 'raise' or 'truncate', got %r" % (overflow,))
    over = np.flatnonzero(np.asarray(n) > C)
    if overflow == "raise" and over.size:
        raise ValueError("masks: frame %d holds %d components, more than max_components = %d (overflow='truncate' keeps "
                         "the first %d in raster order)" % (over[0], n[over[0]], C, C))


def ellipses_from_masks_host(masks, join_tol=0, min_pixels=1, max_components=MAX_K, overflow="raise"):
    """(rows float64 [B,C,6], count int32 [B]) of masks uint8 [B,H,W], in numpy.  ValueError naming the frame that holds
    more than max_components components, unless overflow="truncate"."""
    _check_fit(join_tol, max_components, min_pixels)
    n, sums = component_sums_host(masks, join_tol, max_components)
    _overflow_check(n, int(max_components), overflow)
    return rows_from_sums(sums, n, min_pixels)


def _device_masks(masks):
    import torch
    if not isinstance(masks, torch.Tensor):
        masks = torch.from_numpy(np.ascontiguousarray(_host_masks(masks)))
    if not masks.is_cuda:
        masks = masks.to(default_device(None))
    if masks.dtype != torch.uint8 or masks.dim() != 3:
        raise TypeError("masks: expected a uint8 tensor [B,H,W], got %s %s" % (masks.dtype, tuple(masks.shape)))
    if masks.shape[0]:
        check_size(int(masks.shape[1]), int(masks.shape[2]))
    return masks.contiguous()


def label_components_device(masks, join_tol=0):
    """int32 [B,H,W] device tensor of labels (spnet_mask_label: three launches on the current stream, for any mask).
    masks: a uint8 device tensor [B,H,W], or a host array, which is uploaded."""
    import torch
    from . import _lib as L
    _check_fit(join_tol)
    masks = _device_masks(masks)
    B, H, W = (int(v) for v in masks.shape)
    labels = torch.empty((B, H, W), dtype=torch.int32, device=masks.device)
    if B and H and W:
        with torch.cuda.device(masks.device):
            L.spnet_mask_label(masks.data_ptr(), B, H, W, int(join_tol), labels.data_ptr(), L.current_stream())
    return labels


def component_sums_device(masks, join_tol=0, max_components=MAX_K, labels=None):
    """(n_components int32 [B], sums int64 [B,C,8]) device tensors, see component_sums_host (spnet_mask_moments: two
    launches behind label_components_device's three).  labels: label_components_device's, if the caller has them."""
    import torch
    from . import _lib as L
    _check_fit(join_tol, max_components)
    masks = _device_masks(masks)
    if labels is None:
        labels = label_components_device(masks, join_tol)
    if not (isinstance(labels, torch.Tensor) and labels.dtype == torch.int32 and labels.device == masks.device and
            labels.shape == masks.shape and labels.is_contiguous()):
        raise ValueError("component_sums_device: labels are a contiguous int32 tensor %s on %s"
                         % (tuple(masks.shape), masks.device))
    B, H, W = (int(v) for v in masks.shape)
    C = int(max_components)
    n = torch.empty((B,), dtype=torch.int32, device=masks.device)
    sums = torch.empty((B, C, N_SUMS), dtype=torch.int64, device=masks.device)
    if B and H and W:
        with torch.cuda.device(masks.device):
            L.spnet_mask_moments(masks.data_ptr(), labels.data_ptr(), B, H, W, C, n.data_ptr(), sums.data_ptr(),
                                 L.current_stream())
    return n, sums


def ellipses_from_masks_device(masks, join_tol=0, min_pixels=1, max_components=MAX_K, overflow="raise"):
    """ellipses_from_masks_host with the labelling and the sums on the GPU: (rows float64 [B,C,6], count int32 [B]) device
    tensors, ready for ring_masks_device, augmentation.encode_targets_device (K <= 16 there) and the overlay planner.  The
    B x C x 8 sums come to the host for rows_from_sums (a few KB; the component counts have to come anyway, for the
    ValueError that names a frame with more than max_components components -- overflow="truncate" keeps the first
    max_components in raster order instead) and the rows go back: the same bits as the host path."""
    _check_fit(join_tol, max_components, min_pixels)
    n, sums = component_sums_device(masks, join_tol, max_components)
    _overflow_check(n.cpu().numpy(), int(max_components), overflow)
    return rows_from_sums(sums, n, min_pixels)


def read_masks(paths, device_decode=False):
    """uint8 [N,H,W] of 8-bit grey PNG mask files: a host array by Pillow, or with device_decode a device tensor by
    png.read_png_device.  A missing file is a FileNotFoundError that names it; all files have one size."""
    import os
    paths = list(paths)
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError("read_masks: no mask file %s" % p)
    if device_decode:
        from .png import read_png_device
        return read_png_device(paths)
    from PIL import Image
    out = []
    for p in paths:
        with Image.open(p) as img:
            if img.mode not in ("L", "P", "1"):
                raise ValueError("read_masks: %s is not an 8-bit grey image (mode %s)" % (p, img.mode))
            out.append(np.asarray(img.convert("L") if img.mode == "1" else img, np.uint8))
        if out[-1].shape != out[0].shape:
            raise ValueError("read_masks: %s is %s, the first file %s" % (p, out[-1].shape, out[0].shape))
    return np.stack(out) if out else np.zeros((0, 1, 1), np.uint8)
