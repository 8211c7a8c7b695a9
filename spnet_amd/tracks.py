"""Antinode tracks: which ellipse of frame t + d is the same antinode as one of frame t, and from that a ring count per
antinode over time (csrc/tracks.hip).  The reference's result -- the sympathetic notes ramp up in the video before they are
heard -- is such a curve; the reference linked its detections by hand.

THE RULE (include/spnet_hip.h "Antinode tracks" states it for the kernels).  Input is rows float64 [N,K,6] =
(cx, cy, a, b, angle_deg, rings) with count [N] (clamped to 0 .. K), frames in time order: pad_metadata's layout, the one
masks.ring_masks_device reads.  Detection (t, k) is LIVE iff k < count[t] and masks.quantise_row accepts the row.  Its pixel
set S(t, k) is what the mask rule calls inside that row ALONE on an H x W frame; area = |S|.  For a gap d = 1 .. max_gap:
inter_d[t][i][j] = |S(t,i) & S(t+d,j)|, union = area_i + area_j - inter.  A pair is ELIGIBLE iff inter > 0 and
1024 inter >= iou_q union (iou_q = the IoU threshold in 1/1024, converted once); candidate p is BETTER than q iff
inter_p union_q > inter_q union_p, the lower index winning a tie.  Passes d = 1, 2, .. in order; in pass d, for every frame
pair (t, t+d), i -> j is linked iff j is the best eligible detection of frame t+d that has no predecessor yet for i AND i is
the best eligible detection of frame t that has no successor yet for j.  next / prev hold flat indices t K + k, -1 for none;
track = 1 + the flat index of the chain's head, age = the number of members before; both 0 for a dead row.  All integers:
the device and the host give the same arrays, for any chunking.

NOT HANDLED: splits and merges (a chain has one successor); antinodes that move more than their own size between frames (no
overlap, no link); re-identification after more than max_gap frames.

  link_tracks_device       rows -> (track, age, next, prev, area) int32 device tensors [N,K]
  link_tracks_host         the same in numpy (exact; slow): what the product uses where there is no GPU
  tracks_from_predictions  de-normalised grids [N, 8 n] -> (rows, track, age, next, prev, area), through masks.prediction_rows
  track_table              one record per live detection of every kept track
  track_summary            one record per kept track: frames, length, mean and maximal ring count
  write_tracks             both as CSV files

Nothing here imports torch or the HIP library until a device function is called.
"""
import os

import numpy as np

from . import masks as MK

MAX_K = MK.MAX_K
MAX_GAP = 8                 # csrc/tracks_core.h
IOU_ONE = 1024
MAX_FLAT = (1 << 31) - 2
DEFAULT_IOU, DEFAULT_GAP, DEFAULT_MIN_LEN = 0.25, 1, 3          # choices, not measurements
TABLE_FIELDS = ("frame", "name", "track", "age", "cx", "cy", "a", "b", "angle", "rings")
SUMMARY_FIELDS = ("track", "first_frame", "last_frame", "n", "mean_rings", "max_rings", "frame_of_max")


def iou_to_q(iou):
    """The IoU threshold in 1/1024, 1 .. 1024: the one place where the float becomes the rule's integer."""
    iou = float(iou)
    if not iou == iou:
        raise ValueError("tracks: iou is a number, got %r" % (iou,))
    return min(IOU_ONE, max(1, round(IOU_ONE * iou)))


def _check(N, K, H, W, max_gap):
    MK._check_size(H, W, max(K, 1))
    if not (isinstance(max_gap, (int, np.integer)) and 1 <= max_gap <= MAX_GAP):
        raise ValueError("tracks: max_gap is an integer 1 .. %d, got %r" % (MAX_GAP, max_gap))
    if N * K > MAX_FLAT:
        raise ValueError("tracks: N * K = %d exceeds %d" % (N * K, MAX_FLAT))


def pair_chunks(N, K, d, ws_bytes):
    """[(t0, n_pairs), ...] covering the pairs (t, t + d), t = 0 .. N-d-1, so that int32 [n_pairs][K][K] fits ws_bytes
    (one pair at least)."""
    per = max(1, int(ws_bytes) // (4 * K * K))
    return [(t0, min(per, N - d - t0)) for t0 in range(0, max(N - d, 0), per)]


# ----------------------------------------------------------------------------- the rule on the host
def _windows_host(rows, count, H, W):
    """live bool [N,K], area int32 [N,K], and per frame the list of (k, x0, y0, inside) of its rows with a window."""
    N, K = rows.shape[:2]
    live, area = np.zeros((N, K), bool), np.zeros((N, K), np.int32)
    wins = []
    for t in range(N):
        ws = []
        for k in range(min(max(int(count[t]), 0), K)):
            q = MK.quantise_row(rows[t, k])
            if q is None:
                continue
            live[t, k] = True
            win = MK._inside_row_host(rows[t, k], H, W, True, q)
            if win is not None and win[2].any():
                area[t, k] = int(win[2].sum())
                ws.append((k,) + win)
        wins.append(ws)
    return live, area, wins


def _overlap_host(wins, t0, n_pairs, d, K):
    """inter int32 [n_pairs,K,K] of the pairs (t, t + d), t = t0 .. t0 + n_pairs - 1."""
    inter = np.zeros((n_pairs, K, K), np.int32)
    for p in range(n_pairs):
        for i, ax, ay, A in wins[t0 + p]:
            for j, bx, by, B in wins[t0 + p + d]:
                x0, y0 = max(ax, bx), max(ay, by)
                x1, y1 = min(ax + A.shape[1], bx + B.shape[1]), min(ay + A.shape[0], by + B.shape[0])
                if x1 > x0 and y1 > y0:
                    inter[p, i, j] = np.count_nonzero(A[y0 - ay:y1 - ay, x0 - ax:x1 - ax] & B[y0 - by:y1 - by, x0 - bx:x1 - bx])
    return inter


def _best_host(I, a_self, a_other, open_self, open_other, iou_q):
    """Per row of I int64 [n_self, n_other]: the best eligible open column, -1 for none (ascending scan, strictly better
    replaces: the lower index wins a tie)."""
    U = a_self[:, None] + a_other[None, :] - I
    ok = (I > 0) & (I <= a_self[:, None]) & (I <= a_other[None, :]) & (IOU_ONE * I >= iou_q * U)
    ok &= open_self[:, None] & open_other[None, :]
    best = np.full(I.shape[0], -1, np.int64)
    bi, bu = np.zeros(I.shape[0], np.int64), np.ones(I.shape[0], np.int64)
    for m in np.flatnonzero(ok.any(0)):
        take = ok[:, m] & ((best < 0) | (I[:, m] * bu > bi * U[:, m]))             # products below 2^62
        best[take], bi[take], bu[take] = m, I[take, m], U[take, m]
    return best


def _link_host(inter, area, live, t0, d, iou_q, nxt, prv):
    K = area.shape[1]
    for p in range(inter.shape[0]):
        ta, tb = t0 + p, t0 + p + d
        I = inter[p].astype(np.int64)
        if not I.any():
            continue
        aa, ab = area[ta].astype(np.int64), area[tb].astype(np.int64)
        oa, ob = live[ta] & (nxt[ta] == -1), live[tb] & (prv[tb] == -1)
        fwd = _best_host(I, aa, ab, oa, ob, iou_q)
        bwd = _best_host(I.T, ab, aa, ob, oa, iou_q)
        for i in np.flatnonzero(fwd >= 0):
            j = fwd[i]
            if bwd[j] == i:
                nxt[ta, i] = tb * K + j
                prv[tb, j] = ta * K + i


def _rank_host(prv, live):
    """(track, age) int32 [N,K] by pointer jumping over prev; a prev entry counts only where it points into an earlier
    frame, as on the device."""
    N, K = prv.shape
    x = np.arange(N * K, dtype=np.int64)
    p = prv.reshape(-1).astype(np.int64)
    anc = np.where((p >= 0) & (p < (x // max(K, 1)) * K), p, x)
    dist = (anc != x).astype(np.int64)
    for _ in range(max(1, int(np.ceil(np.log2(max(N, 2)))))):
        anc, dist = anc[anc], dist + dist[anc]
    flat = live.reshape(-1)
    return (np.where(flat, anc + 1, 0).astype(np.int32).reshape(N, K), np.where(flat, dist, 0).astype(np.int32).reshape(N, K))


def link_tracks_host(rows, count=None, H=384, W=512, iou=DEFAULT_IOU, max_gap=DEFAULT_GAP, ws_bytes=256 << 20,
                     return_inter=False):
    """The rule in numpy: (track, age, next, prev, area) int32 [N,K].  rows float64 [N,K,6] with count [N], or a list of label
    lists; count None with an array: every row counts.  ws_bytes chunks the pairs of a pass exactly as the device path does
    (the result does not depend on it).  return_inter: also {d: inter int32 [N-d,K,K]}."""
    if count is None and not isinstance(rows, (list, tuple)):
        count = np.full(np.asarray(rows).shape[0], np.asarray(rows).shape[1], np.int64)
    rows, count = MK._host_rows(rows, count)
    N, K = rows.shape[:2]
    H, W = int(H), int(W)
    _check(N, K, H, W, max_gap)
    iou_q = iou_to_q(iou)
    live, area, wins = _windows_host(rows, count, H, W)
    nxt, prv = np.full((N, K), -1, np.int32), np.full((N, K), -1, np.int32)
    inters = {}
    for d in range(1, int(max_gap) + 1):
        kept = []
        for t0, n in pair_chunks(N, K, d, ws_bytes):
            inter = _overlap_host(wins, t0, n, d, K)
            _link_host(inter, area, live, t0, d, iou_q, nxt, prv)
            if return_inter:
                kept.append(inter)
        if return_inter:
            inters[d] = np.concatenate(kept) if kept else np.zeros((0, K, K), np.int32)
    track, age = _rank_host(prv, live)
    out = (track, age, nxt, prv, area)
    return out + (inters,) if return_inter else out


# ----------------------------------------------------------------------------- the device side
def link_tracks_device(rows, count=None, H=384, W=512, iou=DEFAULT_IOU, max_gap=DEFAULT_GAP, ws_bytes=256 << 20,
                       return_inter=False, device=None):
    """(track, age, next, prev, area) int32 device tensors [N,K] on the current stream.  rows: a float64 device tensor
    [N,K,6] with count int32 [N] (None: every row counts), or a host array / list of label lists, which is uploaded.
    Per pass d the frame pairs are taken ws_bytes of `inter` at a time (int32 [n_pairs][K][K]: 20 KB a pair at K = 72): one
    overlap launch and one link launch per chunk; the result is identical for any chunking.  return_inter: also
    {d: inter int32 [N-d,K,K]} (copies: for tests and inspection, not for a movie)."""
    import torch
    from . import _lib as L
    if not isinstance(rows, torch.Tensor):
        if count is None and not isinstance(rows, (list, tuple)):
            count = np.full(np.asarray(rows).shape[0], np.asarray(rows).shape[1], np.int64)
        r, c = MK._host_rows(rows, count)
        dev = MK._default_device(device)
        rows, count = torch.from_numpy(np.ascontiguousarray(r)).to(dev), torch.from_numpy(c.astype(np.int32)).to(dev)
    if count is None:
        count = torch.full((int(rows.shape[0]),), int(rows.shape[1]) if rows.dim() == 3 else 0, dtype=torch.int32,
                           device=rows.device)
    if not (isinstance(count, torch.Tensor) and rows.is_cuda and count.is_cuda and rows.dtype == torch.float64 and
            count.dtype == torch.int32 and rows.dim() == 3 and rows.shape[2] == 6 and tuple(count.shape) == (rows.shape[0],)):
        raise TypeError("link_tracks_device expects rows float64 [N,K,6] and count int32 [N] on the device")
    rows, count = rows.contiguous(), count.contiguous()
    N, K = int(rows.shape[0]), int(rows.shape[1])
    H, W = int(H), int(W)
    _check(N, K, H, W, max_gap)
    iou_q = iou_to_q(iou)
    dev = rows.device
    area, track, age = (torch.empty((N, K), dtype=torch.int32, device=dev) for _ in range(3))
    nxt, prv = (torch.full((N, K), -1, dtype=torch.int32, device=dev) for _ in range(2))
    inters = {}
    if N:
        with torch.cuda.device(dev):
            st = L.current_stream()
            rp, cp = rows.data_ptr(), count.data_ptr()
            L.spnet_track_area(rp, cp, N, K, H, W, area.data_ptr(), st)
            for d in range(1, int(max_gap) + 1):
                chunks = pair_chunks(N, K, d, ws_bytes)
                inter = torch.empty((max((n for _, n in chunks), default=0), K, K), dtype=torch.int32, device=dev)
                kept = []
                for t0, n in chunks:                    # stream order: a chunk's link reads inter before the next overlap
                    L.spnet_track_overlap(rp, cp, N, K, H, W, t0, n, d, inter.data_ptr(), st)
                    L.spnet_track_link(inter.data_ptr(), area.data_ptr(), rp, cp, N, K, t0, n, d, iou_q, nxt.data_ptr(),
                                       prv.data_ptr(), st)
                    if return_inter:
                        kept.append(inter[:n].clone())
                if return_inter:
                    inters[d] = torch.cat(kept) if kept else torch.zeros((0, K, K), dtype=torch.int32, device=dev)
            ws = torch.empty((int(L.spnet_track_rank_ws(N, K)),), dtype=torch.uint8, device=dev)
            L.spnet_track_rank(prv.data_ptr(), rp, cp, N, K, track.data_ptr(), age.data_ptr(), ws.data_ptr(), st)
    elif return_inter:
        inters = {d: torch.zeros((0, K, K), dtype=torch.int32, device=dev) for d in range(1, int(max_gap) + 1)}
    out = (track, age, nxt, prv, area)
    return out + (inters,) if return_inter else out


def tracks_from_predictions(Y_denorm, H=384, W=512, iou=DEFAULT_IOU, max_gap=DEFAULT_GAP, ws_bytes=256 << 20, host=False,
                            device=None):
    """(rows, track, age, next, prev, area) of de-normalised grids [N, 8 n] in time order (host array or tensor on any
    device): one row per predictor through masks.prediction_rows, dead where noobj >= 0.5.  On the GPU (a host array is
    uploaded; rows of a device tensor never leave it) unless host=True, which runs the numpy rule and returns arrays."""
    if host:
        Y = Y_denorm.cpu().numpy() if hasattr(Y_denorm, "is_cuda") else np.asarray(Y_denorm)
        if Y.ndim != 2 or Y.shape[1] % 8 or not Y.shape[1]:
            raise ValueError("tracks_from_predictions expects [N, 8 n] grids, got %s" % (Y.shape,))
        rows = np.ascontiguousarray(MK.prediction_rows(Y))
        return (rows,) + link_tracks_host(rows, None, H, W, iou, max_gap, ws_bytes)
    import torch
    if not isinstance(Y_denorm, torch.Tensor):
        Y_denorm = torch.from_numpy(np.ascontiguousarray(np.asarray(Y_denorm)))
    if not Y_denorm.is_cuda:
        Y_denorm = Y_denorm.to(MK._default_device(device))
    if Y_denorm.dim() != 2 or Y_denorm.shape[1] % 8 or not Y_denorm.shape[1]:
        raise ValueError("tracks_from_predictions expects [N, 8 n] grids, got %s" % (tuple(Y_denorm.shape),))
    rows = MK.prediction_rows(Y_denorm, torch).contiguous()
    return (rows,) + link_tracks_device(rows, None, H, W, iou, max_gap, ws_bytes)


# ----------------------------------------------------------------------------- tables (numpy on N * K integers)
def _host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def _kept(rows, track, age, min_len):
    rows, track, age = np.asarray(_host(rows), np.float64), _host(track).astype(np.int64), _host(age).astype(np.int64)
    if rows.ndim != 3 or rows.shape[2] != 6 or track.shape != rows.shape[:2] or age.shape != track.shape:
        raise ValueError("tracks: rows [N,K,6] with track and age [N,K], got %s, %s and %s" % (rows.shape, track.shape, age.shape))
    if not (isinstance(min_len, (int, np.integer)) and min_len >= 1):
        raise ValueError("tracks: min_len is an integer >= 1, got %r" % (min_len,))
    K = rows.shape[1]
    flat = np.flatnonzero(track.reshape(-1) > 0)
    ids = track.reshape(-1)[flat]
    uniq, inverse, n = np.unique(ids, return_inverse=True, return_counts=True)
    flat, ids = flat[n[inverse] >= min_len], ids[n[inverse] >= min_len]
    order = np.lexsort((flat, ids))                         # by (track, frame): a track has one member a frame
    flat, ids = flat[order], ids[order]
    return rows.reshape(-1, 6)[flat], ids, age.reshape(-1)[flat], flat // max(K, 1)


def track_table(rows, track, age, names=None, min_len=1):
    """One record (frame, name, track, age, cx, cy, a, b, angle, rings) per live detection of a track with at least min_len
    members, ordered by (track, frame).  names: one per frame (file names); "" without."""
    r, ids, ages, frames = _kept(rows, track, age, min_len)
    if names is not None and len(names) < (int(frames.max()) + 1 if frames.size else 0):
        raise ValueError("track_table: %d names for %d frames" % (len(names), int(frames.max()) + 1))
    return [(int(f), "" if names is None else str(names[f]), int(i), int(g)) + tuple(float(v) for v in row)
            for row, i, g, f in zip(r, ids, ages, frames)]


def track_summary(rows, track, age, min_len=1):
    """One record (track, first_frame, last_frame, n, mean_rings, max_rings, frame_of_max) per track with at least min_len
    members, in track order; frame_of_max is the FIRST frame that reaches the maximum."""
    r, ids, _, frames = _kept(rows, track, age, min_len)
    out = []
    starts = np.flatnonzero(np.concatenate([[True], ids[1:] != ids[:-1]])) if ids.size else np.zeros(0, np.int64)
    for s, e in zip(starts, list(starts[1:]) + [ids.size]):
        rings = r[s:e, 5]
        out.append((int(ids[s]), int(frames[s]), int(frames[e - 1]), int(e - s), float(rings.mean()), float(rings.max()),
                    int(frames[s + int(np.argmax(rings))])))
    return out


def summary_path(path):
    root, ext = os.path.splitext(path)
    return root + "_summary" + ext


def write_tracks(path, rows, track, age, names=None, min_len=1):
    """The table as CSV at `path` and the summary at `path` with _summary before the extension (header lines: TABLE_FIELDS,
    SUMMARY_FIELDS; floats by repr, so they read back exactly).  Returns (table, summary)."""
    table, summary = track_table(rows, track, age, names, min_len), track_summary(rows, track, age, min_len)
    for p, fields, records in ((path, TABLE_FIELDS, table), (summary_path(path), SUMMARY_FIELDS, summary)):
        with open(p, "w") as f:
            f.write(",".join(fields) + "\n")
            for rec in records:
                f.write(",".join(repr(v) if isinstance(v, float) else str(v) for v in rec) + "\n")
    return table, summary
