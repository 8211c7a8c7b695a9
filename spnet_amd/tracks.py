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

THE SCORE (include/spnet_hip.h "Tracking score"; csrc/track_score.hip): linked tracks against ground-truth
identities, in the rule's own vocabulary -- per frame truth and prediction matched where each is the other's best eligible
candidate, per identity present and matched frames, identity switches, fragments and the first matched frame.

  score_tracks_device      truth + predicted tracks -> (match, frame_counts, ident_stats) int32 device tensors
  score_tracks_host        the same in numpy (match_tracks_host, ident_stats_host)
  track_score              those integers -> the dictionary (MOTA, precision, recall, ...): one function for both paths
  write_truth_tracks / read_truth_tracks / truth_arrays     ground truth as a table in TABLE_FIELDS, and back
  write_track_score        the dictionary and the per-identity statistics as CSV files

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
    MK.check_size(H, W, max(K, 1))
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
    live = live_rows_host(rows, count)
    area, wins = np.zeros(live.shape, np.int32), []
    for t in range(live.shape[0]):
        ws = []
        for k in np.flatnonzero(live[t]):
            win = MK.inside_row_host(rows[t, k], H, W)
            if win is not None and win[2].any():
                area[t, k] = int(win[2].sum())
                ws.append((int(k),) + win)
        wins.append(ws)
    return live, area, wins


def _overlap_host(wins, t0, n_pairs, d, K):
    """inter int32 [n_pairs,K,K] of the pairs (t, t + d), t = t0 .. t0 + n_pairs - 1."""
    inter = np.zeros((n_pairs, K, K), np.int32)
    for p in range(n_pairs):
        _inter_frames_host(wins[t0 + p], wins[t0 + p + d], inter[p])
    return inter


def _inter_frames_host(wins_a, wins_b, out):
    """out [Ka,Kb] (zeros) receives |S(a, i) & S(b, j)| of two frames' window lists."""
    for i, ax, ay, A in wins_a:
        for j, bx, by, B in wins_b:
            x0, y0 = max(ax, bx), max(ay, by)
            x1, y1 = min(ax + A.shape[1], bx + B.shape[1]), min(ay + A.shape[0], by + B.shape[0])
            if x1 > x0 and y1 > y0:
                out[i, j] = np.count_nonzero(A[y0 - ay:y1 - ay, x0 - ax:x1 - ax] & B[y0 - by:y1 - by, x0 - bx:x1 - bx])


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


def _mutual_host(I, area_a, area_b, open_a, open_b, iou_q):
    """The mutual best of two sides: per row of I [Ka,Kb] its partner j -- the best eligible open column, whose best
    eligible open row it is -- or -1."""
    I, area_a, area_b = (np.asarray(v).astype(np.int64) for v in (I, area_a, area_b))
    fwd = _best_host(I, area_a, area_b, open_a, open_b, iou_q)
    bwd = _best_host(I.T, area_b, area_a, open_b, open_a, iou_q)
    hit = np.flatnonzero(fwd >= 0)                          # (an empty side B leaves none: bwd is never indexed)
    out = np.full(fwd.size, -1, np.int64)
    out[hit] = np.where(bwd[fwd[hit]] == hit, fwd[hit], -1)
    return out


def _link_host(inter, area, live, t0, d, iou_q, nxt, prv):
    K = area.shape[1]
    for p in range(inter.shape[0]):
        ta, tb = t0 + p, t0 + p + d
        if not inter[p].any():
            continue
        j = _mutual_host(inter[p], area[ta], area[tb], live[ta] & (nxt[ta] == -1), live[tb] & (prv[tb] == -1), iou_q)
        i = np.flatnonzero(j >= 0)
        nxt[ta, i], prv[tb, j[i]] = tb * K + j[i], ta * K + i


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
    rows, count = MK.host_rows(rows, count)
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
    rows, count, N, K = MK.device_rows(rows, count, device, MK.ROWS_TEXT % ("link_tracks_device", "N", "N"), every_row=True)
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
        Y = _host(Y_denorm)
        MK.check_grids(Y, "tracks_from_predictions")
        rows = np.ascontiguousarray(MK.prediction_rows(Y))
        return (rows,) + link_tracks_host(rows, None, H, W, iou, max_gap, ws_bytes)
    import torch
    rows = MK.prediction_rows(MK.device_grids(Y_denorm, device, "tracks_from_predictions"), torch).contiguous()
    return (rows,) + link_tracks_device(rows, None, H, W, iou, max_gap, ws_bytes)


# ----------------------------------------------------------------------------- tables (numpy on N * K integers)
_host = MK.host_array


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


def _suffixed(path, suffix):
    root, ext = os.path.splitext(path)
    return root + suffix + ext


def summary_path(path):
    return _suffixed(path, "_summary")


def _write_csv(path, fields, records):
    """A header line and one line per record: None as an empty field, a float by repr (it reads back exactly)."""
    with open(path, "w") as f:
        f.write(",".join(fields) + "\n")
        for rec in records:
            f.write(",".join("" if v is None else repr(v) if isinstance(v, float) else str(v) for v in rec) + "\n")


def write_tracks(path, rows, track, age, names=None, min_len=1):
    """The table as CSV at `path` and the summary at `path` with _summary before the extension (header lines: TABLE_FIELDS,
    SUMMARY_FIELDS; floats by repr, so they read back exactly).  Returns (table, summary)."""
    table, summary = track_table(rows, track, age, names, min_len), track_summary(rows, track, age, min_len)
    _write_csv(path, TABLE_FIELDS, table)
    _write_csv(summary_path(path), SUMMARY_FIELDS, summary)
    return table, summary


# ----------------------------------------------------------------------------- the tracking score (csrc/track_score.hip)
MAX_M = 65536               # csrc/track_score_core.h
STAT_FIELDS = ("ident", "present", "matched", "switches", "fragments", "first_matched_frame")
SCORE_FIELDS = ("gt", "tp", "fn", "fp", "switches", "fragments", "mota", "precision", "recall", "identities", "mostly_tracked",
                "mostly_lost", "ring_mae", "onset_error")


def score_path(path):
    return _suffixed(path, "_score")


def _check_score(N, Kt, Kp, H, W, M):
    MK.check_size(H, W, max(Kt, 1))
    MK.check_size(H, W, max(Kp, 1))
    if N * Kt > MAX_FLAT or N * Kp > MAX_FLAT:
        raise ValueError("tracks: N * K = %d exceeds %d" % (N * max(Kt, Kp), MAX_FLAT))
    if not (isinstance(M, (int, np.integer)) and 1 <= M <= MAX_M):
        raise ValueError("tracks: the number of identities M is an integer 1 .. %d, got %r" % (MAX_M, M))


def frame_chunks(N, Kt, Kp, ws_bytes):
    """[(n0, n), ...] covering the frames so that a chunk's inter int32 [n][Kt][Kp] fits ws_bytes (one frame at least) and
    the limit n * Kt * Kp <= 2^31 - 2."""
    per = max(1, min(int(ws_bytes) // (4 * Kt * Kp), MAX_FLAT // (Kt * Kp)))
    return [(n0, min(per, N - n0)) for n0 in range(0, N, per)]


def effective_ident_host(live, ident, M):
    """eff int32 [N,Kt]: ident where the row is live, 1 <= ident <= M and no live row of a lower index in the frame has the
    same ident; 0 otherwise (the rule's "Identity")."""
    ident = np.asarray(ident).astype(np.int64)
    ok = live & (ident >= 1) & (ident <= M)
    eff = np.where(ok, ident, 0)
    for n, k in zip(*np.nonzero(ok)):
        if k and (eff[n, :k] == ident[n, k]).any():
            eff[n, k] = 0
    return eff.astype(np.int32)


def match_tracks_host(rows_t, count_t, ident, rows_p, count_p, track, H=384, W=512, iou=DEFAULT_IOU, M=None):
    """The match rule in numpy (include/spnet_hip.h "Tracking score"): (match int32 [N,Kt], frame_counts int32 [N,3] =
    (tp, fn, fp), eff int32 [N,Kt] the effective identities).  M None: the largest ident."""
    rows_t, count_t = MK.host_rows(np.asarray(rows_t, np.float64), np.asarray(count_t))
    rows_p, count_p = MK.host_rows(np.asarray(rows_p, np.float64), np.asarray(count_p))
    ident, track = np.asarray(ident).astype(np.int64), np.asarray(track).astype(np.int64)
    N, Kt, Kp = rows_t.shape[0], rows_t.shape[1], rows_p.shape[1]
    if rows_p.shape[0] != N or ident.shape != (N, Kt) or track.shape != (N, Kp):
        raise ValueError("tracks: truth [N,Kt] and prediction [N,Kp] of the same N frames, got %s, %s, %s, %s"
                         % (rows_t.shape, ident.shape, rows_p.shape, track.shape))
    M = _default_M(ident) if M is None else M
    _check_score(N, Kt, Kp, int(H), int(W), M)
    iou_q = iou_to_q(iou)
    live_t, area_t, wins_t = _windows_host(rows_t, count_t, int(H), int(W))
    live_p, area_p, wins_p = _windows_host(rows_p, count_p, int(H), int(W))
    eff = effective_ident_host(live_t, ident, M)
    open_t, open_p = eff > 0, live_p & (track > 0)
    match, counts = np.full((N, Kt), -1, np.int32), np.zeros((N, 3), np.int32)
    for n in range(N):
        I = np.zeros((Kt, Kp), np.int64)
        _inter_frames_host(wins_t[n], wins_p[n], I)
        match[n] = _mutual_host(I, area_t[n], area_p[n], open_t[n], open_p[n], iou_q)
        tp = int((match[n] >= 0).sum())
        counts[n] = (tp, int(open_t[n].sum()) - tp, int(open_p[n].sum()) - tp)
    return match, counts, eff


def ident_stats_host(eff, match, track, M):
    """The identity statistics in numpy: int32 [M + 1, 5] = (present, matched, switches, fragments, first_matched_frame),
    row 0 zeroed.  eff: effective_ident_host's array; a match entry outside 0 .. Kp-1 counts as unmatched."""
    eff, match, track = np.asarray(eff), np.asarray(match).astype(np.int64), np.asarray(track)
    Kp = track.shape[1] if track.ndim == 2 else 0
    stats = np.zeros((M + 1, 5), np.int32)
    stats[1:, 4] = -1
    last_track, gap = {}, {}
    for n, k in zip(*np.nonzero(eff > 0)):                         # row-major: time order
        g, m = int(eff[n, k]), int(match[n, k])
        s = stats[g]
        s[0] += 1
        if not 0 <= m < Kp:
            gap[g] = s[1] > 0
            continue
        tr = int(track[n, m])
        if s[1] > 0 and tr != last_track[g]:
            s[2] += 1
        if gap.get(g):
            s[3] += 1
        if s[1] == 0:
            s[4] = n
        s[1] += 1
        last_track[g], gap[g] = tr, False
    return stats


def _default_M(ident):
    size = ident.numel() if hasattr(ident, "numel") else ident.size
    m = int(ident.max()) if size else 0
    if m > MAX_M:
        raise ValueError("tracks: the largest identity %d exceeds %d; renumber the identities" % (m, MAX_M))
    return max(m, 1)


def score_tracks_host(rows_t, count_t, ident, rows_p, count_p, track, H=384, W=512, iou=DEFAULT_IOU, M=None):
    """(match int32 [N,Kt], frame_counts int32 [N,3], ident_stats int32 [M+1,5]) by the numpy rule."""
    ident = np.asarray(ident)
    M = _default_M(ident) if M is None else M
    match, counts, eff = match_tracks_host(rows_t, count_t, ident, rows_p, count_p, track, H, W, iou, M)
    return match, counts, ident_stats_host(eff, match, track, M)


def score_tracks_device(rows_t, count_t, ident, rows_p, count_p, track, H=384, W=512, iou=DEFAULT_IOU, M=None,
                        ws_bytes=256 << 20):
    """(match int32 [N,Kt], frame_counts int32 [N,3], ident_stats int32 [M+1,5]) device tensors on the current stream
    (spnet_track_match a range of frames at a time, ws_bytes of inter each, then spnet_track_ident over the whole movie; the
    result is identical for any chunking).  Truth rows_t float64 [N,Kt,6], count_t int32 [N], ident int32 [N,Kt]; prediction
    rows_p [N,Kp,6], count_p [N] (None: every row counts), track int32 [N,Kp] as link_tracks_device returns it: all device
    tensors.  M None: the largest ident (one scalar read back)."""
    import torch
    from . import _lib as L
    text = ("score_tracks_device expects device tensors: rows float64 [N,K,6], count int32 [N], ident int32 [N,Kt], "
            "track int32 [N,Kp]")
    rows_t, count_t, N, Kt = MK.device_rows(rows_t, count_t, None, text, upload=False)
    rows_p, count_p, Np, Kp = MK.device_rows(rows_p, count_p, None, text, every_row=True, upload=False)
    dev = rows_t.device
    if not (Np == N and all(isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.int32 for a in (ident, track))
            and tuple(ident.shape) == (N, Kt) and tuple(track.shape) == (N, Kp)):
        raise TypeError(text)
    ident, track = ident.contiguous(), track.contiguous()
    M = _default_M(ident) if M is None else M
    _check_score(N, Kt, Kp, int(H), int(W), M)
    iou_q = iou_to_q(iou)
    match = torch.empty((N, Kt), dtype=torch.int32, device=dev)
    counts = torch.empty((N, 3), dtype=torch.int32, device=dev)
    stats = torch.empty((M + 1, 5), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        st = L.current_stream()
        chunks = frame_chunks(N, Kt, Kp, ws_bytes)
        if chunks:
            ws = torch.empty((int(L.spnet_track_match_ws(max(n for _, n in chunks), Kt, Kp)),), dtype=torch.uint8, device=dev)
        for n0, n in chunks:                                # stream order: a chunk is done with ws before the next one
            L.spnet_track_match(rows_t[n0:].data_ptr(), count_t[n0:].data_ptr(), ident[n0:].data_ptr(), Kt,
                                rows_p[n0:].data_ptr(), count_p[n0:].data_ptr(), track[n0:].data_ptr(), Kp, n, int(H), int(W),
                                iou_q, M, ws.data_ptr(), match[n0:].data_ptr(), counts[n0:].data_ptr(), st)
        ws2 = torch.empty((int(L.spnet_track_ident_ws(N, Kt, M)),), dtype=torch.uint8, device=dev)
        L.spnet_track_ident(L.ptr(rows_t) if N else ws2.data_ptr(), L.ptr(count_t) if N else ws2.data_ptr(),
                            L.ptr(ident) if N else ws2.data_ptr(), L.ptr(match) if N else ws2.data_ptr(),
                            L.ptr(track) if N else ws2.data_ptr(), N, Kt, Kp, M, ws2.data_ptr(), stats.data_ptr(), st)
    return match, counts, stats


def live_rows_host(rows, count=None):
    """live bool [N,K]: k < count (clamped to 0 .. K; None: every row) and masks.quantise_row accepts the row."""
    rows = np.asarray(rows, np.float64)
    N, K = rows.shape[:2]
    live = np.zeros((N, K), bool)
    for n in range(N):
        for k in range(K if count is None else min(max(int(count[n]), 0), K)):
            live[n, k] = MK.quantise_row(rows[n, k]) is not None
    return live


def track_score(match, frame_counts, ident_stats, rows_t, rows_p, ident=None, count_t=None):
    """The score as a dictionary (SCORE_FIELDS), in float64 on the host from the integer arrays of either path -- ONE
    function for both, so the device and the host scores agree bit for bit.  gt = tp + fn; mota = 1 - (fn + fp + switches) /
    gt; precision = tp / (tp + fp); recall = tp / (tp + fn); identities = those present in some frame, mostly_tracked /
    mostly_lost = those with matched / present >= 0.8 / <= 0.2 (compared as integers); ring_mae = the mean |rings_t -
    rings_p| over the matched pairs; onset_error = the mean over the identities that are ever matched of first_matched_frame
    minus the identity's first PRESENT frame, which ident_stats does not hold: it is found from `ident` (the truth
    identities [N,Kt]) and count_t ([N]; None: every row counts) by the rule's own effective identity -- live rows, 1 ..
    M, the lower index of a duplicate -- so it is the first of the frames that `present` counts; None without ident.  A
    ratio with a zero denominator is None."""
    match, fc, st = _host(match).astype(np.int64), _host(frame_counts).astype(np.int64), _host(ident_stats).astype(np.int64)
    rows_t, rows_p = np.asarray(_host(rows_t), np.float64), np.asarray(_host(rows_p), np.float64)
    tp, fn, fp = (int(v) for v in fc.sum(0)) if fc.size else (0, 0, 0)
    switches, fragments = int(st[1:, 2].sum()), int(st[1:, 3].sum())
    gt = tp + fn

    def ratio(a, b):
        return float(a) / float(b) if b else None

    present, matched = st[1:, 0], st[1:, 1]
    nn, ii = np.nonzero(match >= 0)
    err = np.abs(rows_t[nn, ii, 5] - rows_p[nn, match[nn, ii], 5])
    onset = None
    if ident is not None:
        eff = effective_ident_host(live_rows_host(rows_t, None if count_t is None else _host(count_t)), _host(ident),
                                   st.shape[0] - 1).astype(np.int64)
        first = np.full(st.shape[0], eff.shape[0], np.int64)
        np.minimum.at(first, eff[eff > 0], np.nonzero(eff > 0)[0])
        sel = np.flatnonzero(st[:, 4] >= 0)
        sel = sel[sel >= 1]
        onset = float((st[sel, 4] - first[sel]).sum()) / len(sel) if len(sel) else None
    return {"gt": gt, "tp": tp, "fn": fn, "fp": fp, "switches": switches, "fragments": fragments,
            "mota": None if not gt else 1.0 - float(fn + fp + switches) / float(gt),
            "precision": ratio(tp, tp + fp), "recall": ratio(tp, tp + fn), "identities": int((present > 0).sum()),
            "mostly_tracked": int(((present > 0) & (5 * matched >= 4 * present)).sum()),
            "mostly_lost": int(((present > 0) & (5 * matched <= present)).sum()),
            "ring_mae": float(err.sum()) / len(err) if len(err) else None, "onset_error": onset}


def truth_table(rows, ident, names=None):
    """Ground-truth identities as track_table records: `track` is the identity, `age` the number of frames since its first
    frame.  rows [N,K,6], ident [N,K] (0: no identity)."""
    ident = _host(ident).astype(np.int64)
    first = {}
    age = np.zeros_like(ident)
    for n, k in zip(*np.nonzero(ident > 0)):
        age[n, k] = n - first.setdefault(int(ident[n, k]), n)
    return track_table(rows, ident, age, names, 1)


def write_truth_tracks(path, rows, ident, names=None):
    """truth_table as a CSV with the header TABLE_FIELDS (floats by repr: they read back exactly).  Returns the table."""
    table = truth_table(rows, ident, names)
    _write_csv(path, TABLE_FIELDS, table)
    return table


def read_truth_tracks(path):
    """The records of a truth_tracks.csv (or of any table write_tracks wrote), typed as track_table gives them."""
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or tuple(lines[0].split(",")) != TABLE_FIELDS:
        raise ValueError("read_truth_tracks: %s does not start with the header %s" % (path, ",".join(TABLE_FIELDS)))
    out = []
    for line in lines[1:]:
        v = line.split(",")
        if len(v) != len(TABLE_FIELDS):
            raise ValueError("read_truth_tracks: %s: %d fields in %r" % (path, len(v), line))
        out.append((int(v[0]), v[1], int(v[2]), int(v[3])) + tuple(float(x) for x in v[4:]))
    return out


def truth_arrays(records, names=None, n_frames=None, skip_unknown=False):
    """Truth records -> (rows float64 [N,K,6], count int32 [N], ident int32 [N,K]), a frame's rows in record order.  names (a
    list of file names, one per frame of the prediction): records are joined BY NAME and a record of an unknown name is an
    error, or left out with skip_unknown (a loader that rounds the frames down to whole batches); otherwise by frame index, with n_frames frames (default: the largest index + 1)."""
    if names is not None:
        index = {os.path.basename(str(nm)): n for n, nm in enumerate(names)}
        if skip_unknown:
            records = [r for r in records if os.path.basename(r[1]) in index]
        frames = []
        for r in records:
            if os.path.basename(r[1]) not in index:
                raise ValueError("tracks: truth frame %r is not among the predicted frames" % (r[1],))
            frames.append(index[os.path.basename(r[1])])
        N = len(names)
    else:
        frames = [r[0] for r in records]
        N = int(n_frames) if n_frames is not None else (max(frames) + 1 if frames else 0)
        if frames and (min(frames) < 0 or max(frames) >= N):
            raise ValueError("tracks: truth frames %d .. %d outside the movie's %d frames" % (min(frames), max(frames), N))
    per = [[] for _ in range(N)]
    for f, r in sorted(zip(frames, records), key=lambda fr: (fr[0], fr[1][2])):
        per[f].append(r)
    K = max(max((len(p) for p in per), default=0), 1)
    if K > MAX_K:
        raise ValueError("tracks: %d truth rows in one frame exceed %d" % (K, MAX_K))
    rows, count, ident = np.zeros((N, K, 6), np.float64), np.zeros(N, np.int32), np.zeros((N, K), np.int32)
    for n, p in enumerate(per):
        count[n] = len(p)
        for k, r in enumerate(p):
            rows[n, k], ident[n, k] = r[4:], r[2]
    return rows, count, ident


def write_track_score(path, score, ident_stats):
    """The score dictionary at `path` (a header line of SCORE_FIELDS and one line of values; None as an empty field) and the
    per-identity statistics of the identities that are present at `path` with _idents before the extension (STAT_FIELDS)."""
    st = _host(ident_stats).astype(np.int64)
    _write_csv(path, SCORE_FIELDS, [[score[k] for k in SCORE_FIELDS]])
    _write_csv(_suffixed(path, "_idents"), STAT_FIELDS,
               [(g,) + tuple(int(v) for v in st[g]) for g in range(1, st.shape[0]) if st[g, 0] > 0])
