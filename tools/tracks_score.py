#!/usr/bin/env python3
"""Dev tool (GPU box): how well the linker's three flags follow antinodes, measured on strike movies with known tracks.

`--sequences` strike sequences (default 64) of `--frames` frames (default 64) at 384 x 512, jitter `--jitter` (default 2),
seed `--seed` (fake_espi.strike_params_device).  The sequences are laid end to end as one movie with 4 empty frames between
two of them, which no gap of the sweep bridges.  The linker (tracks.link_tracks_device) runs on
  perfect    the truth rows themselves (a perfect detector)
  low / mid / high   the truth rows perturbed as a detector perturbs them, seeded: centre noise N(0, sigma_c) px, axis
             noise N(0, sigma_a) relative, and detections dropped with probability p_drop (LEVELS below), positions and
             axes rounded to sixteenths
over track_iou in {0.1, 0.25, 0.5} x track_gap in {1, 2, 4}; tracks with fewer than track_min_len in {1, 3} detections are
then taken out (their rows count as undetected), and the rest is scored against the truth by tracks.score_tracks_device at a
FIXED matching IoU of `--score_iou` (default 0.25).  Per cell: MOTA, switches, fragments, onset_error and the counts.  The
leg on real predictor output (tracks_from_predictions) needs trained weights; none were at hand, so it is left out and the
file says so.  No threshold is set beforehand: the file records what came out.

Timing: the two new entry points through score_tracks_device on the whole movie against score_tracks_host on the first
`--host_sequences` sequences (default 2; the numpy rule is slow), alternating in this one process, median / min / max of
`--repeats` rounds after a warm-up round; and spnet_track_match and spnet_track_ident alone (events around back-to-back
launches over rotating outputs).

usage: tracks_score.py [--sequences 64] [--frames 64] [--out profiles/tracks_score.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resize_time import gpu_time

H, W, PAD = 384, 512, 4
IOUS, GAPS, MIN_LENS = (0.1, 0.25, 0.5), (1, 2, 4), (1, 3)
LEVELS = (("perfect", 0.0, 0.0, 0.0), ("low", 1.0, 0.03, 0.05), ("mid", 2.0, 0.06, 0.15), ("high", 4.0, 0.10, 0.30))


def movie(S, T, seed, jitter):
    """(rows float64 [S (T + PAD), 7, 6], count, ident) on the device: the sequences end to end, PAD empty frames after each."""
    import torch
    from spnet_amd import fake_espi as F
    rows, count, ident = F.strike_rows(*F.strike_params_device(S, T, seed, jitter)[1:])

    def padded(a):
        out = torch.zeros((S, T + PAD) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
        out[:, :T] = a.reshape((S, T) + tuple(a.shape[1:]))
        return out.reshape((S * (T + PAD),) + tuple(a.shape[1:])).contiguous()
    return padded(rows), padded(count), padded(ident)


def perturb(rows, count, sigma_c, sigma_a, p_drop, seed):
    """The rows as a detector of that quality would report them (a dropped detection: axes 0, a dead row)."""
    import torch
    if sigma_c == 0 and sigma_a == 0 and p_drop == 0:
        return rows
    g = torch.Generator(device="cpu").manual_seed(seed)
    n, k = rows.shape[:2]
    dc = (torch.randn((n, k, 2), generator=g, dtype=torch.float64) * sigma_c).to(rows.device)
    da = (1.0 + torch.randn((n, k, 2), generator=g, dtype=torch.float64) * sigma_a).clamp(0.5, 1.5).to(rows.device)
    keep = (torch.rand((n, k), generator=g, dtype=torch.float64) >= p_drop).to(rows.device)
    out = rows.clone()
    out[..., :2] = torch.round((rows[..., :2] + dc) * 16.0) / 16.0
    out[..., 2:4] = torch.round(rows[..., 2:4] * da * 16.0) / 16.0 * keep[..., None]
    return out.contiguous()


def drop_short(track, min_len):
    import torch
    if min_len <= 1:
        return track
    flat = track.reshape(-1)
    _, inv, cnt = torch.unique(flat, return_inverse=True, return_counts=True)
    return torch.where((cnt[inv] >= min_len) & (flat > 0), flat, torch.zeros_like(flat)).reshape(track.shape).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=64)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--jitter", type=int, default=2)
    ap.add_argument("--seed", type=int, default=11)
    ap.add_argument("--noise_seed", type=int, default=12)
    ap.add_argument("--score_iou", type=float, default=0.25)
    ap.add_argument("--host_sequences", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/tracks_score.json")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "tracks_score.py measures on the GPU"
    from spnet_amd import _lib as L
    from spnet_amd import tracks as TK

    S, T = args.sequences, args.frames
    rows_t, count_t, ident = movie(S, T, args.seed, args.jitter)
    N, K = int(rows_t.shape[0]), int(rows_t.shape[1])
    M = int(ident.max())
    ident_h, count_h = ident.cpu().numpy(), count_t.cpu().numpy()
    res = {"device": torch.cuda.get_device_name(0), "sequences": S, "frames_per_sequence": T, "pad_frames": PAD, "movie_frames": N,
           "H": H, "W": W, "K": K, "identities": int(np.unique(ident_h[ident_h > 0]).size), "truth_detections": int((ident_h > 0).sum()),
           "seed": args.seed, "jitter": args.jitter, "noise_seed": args.noise_seed, "score_iou": args.score_iou,
           "levels": {n: {"sigma_centre_px": c, "sigma_axis_rel": a, "p_drop": p} for n, c, a, p in LEVELS},
           "defaults": {"track_iou": TK.DEFAULT_IOU, "track_gap": TK.DEFAULT_GAP, "track_min_len": TK.DEFAULT_MIN_LEN},
           "cpus_usable": len(os.sched_getaffinity(0)), "cells": [], "best": {},
           "real_predictor_leg": "left out: no trained weight file was at hand"}

    for li, (level, sc, sa, pd) in enumerate(LEVELS):
        rows_p = perturb(rows_t, count_t, sc, sa, pd, args.noise_seed + li)
        for iou in IOUS:
            for gap in GAPS:
                track = TK.link_tracks_device(rows_p, count_t, H, W, iou=iou, max_gap=gap)[0]
                for ml in MIN_LENS:
                    got = TK.score_tracks_device(rows_t, count_t, ident, rows_p, count_t, drop_short(track, ml), H, W,
                                                 iou=args.score_iou, M=M)
                    s = TK.track_score(*got, rows_t, rows_p, ident=ident_h, count_t=count_h)
                    cell = {"level": level, "track_iou": iou, "track_gap": gap, "track_min_len": ml}
                    cell.update({k: s[k] for k in ("mota", "switches", "fragments", "onset_error", "gt", "tp", "fn", "fp",
                                                   "mostly_tracked", "mostly_lost", "ring_mae")})
                    res["cells"].append(cell)
        cells = [c for c in res["cells"] if c["level"] == level]
        order = sorted(cells, key=lambda c: (-c["mota"], c["switches"], c["fragments"]))
        default = next(c for c in cells if (c["track_iou"], c["track_gap"], c["track_min_len"]) ==
                       (TK.DEFAULT_IOU, TK.DEFAULT_GAP, TK.DEFAULT_MIN_LEN))
        res["best"][level] = {"best": order[0], "default": default, "default_rank_of_%d" % len(order): 1 + order.index(default),
                              "default_is_best": order[0]["mota"] == default["mota"] and order[0]["switches"] == default["switches"]}
        print(level, "best", json.dumps(order[0]), "\n   default", json.dumps(default), "rank", 1 + order.index(default), flush=True)

    # ---- time: the device path on the whole movie, the host rule on the first sequences; mid-level rows, default flags
    rows_p = perturb(rows_t, count_t, *LEVELS[2][1:], args.noise_seed + 2)
    track = TK.link_tracks_device(rows_p, count_t, H, W)[0]
    nh = min(args.host_sequences, S) * (T + PAD)
    host_args = [a[:nh].cpu().numpy() for a in (rows_t, count_t, ident, rows_p, count_t, track)]
    got = {}

    def host():
        got["score_tracks_host"] = TK.score_tracks_host(*host_args, H, W, iou=args.score_iou, M=M)

    def device():
        got["score_tracks_device"] = TK.score_tracks_device(rows_t, count_t, ident, rows_p, count_t, track, H, W, iou=args.score_iou, M=M)

    ways = (("score_tracks_host", host, nh), ("score_tracks_device", device, N))
    times = {k: [] for k, _, _ in ways}
    for rnd in range(args.repeats + 1):              # round 0 warms up
        for name, fn, _ in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
        if rnd == 0:                                 # match and the frame counts of the first frames: the same integers
            for k in (0, 1):
                assert np.array_equal(got["score_tracks_device"][k][:nh].cpu().numpy(), got["score_tracks_host"][k]), k
    for name, _, frames in ways:
        t = sorted(times[name])
        res[name] = {"frames_per_s": frames / t[len(t) // 2], "min_frames_per_s": frames / t[-1],
                     "max_frames_per_s": frames / t[0], "ms_per_frame": 1e3 * t[len(t) // 2] / frames, "rounds": len(t),
                     "frames": frames}
        print(name, json.dumps(res[name]), flush=True)
    res["device_over_host"] = res["score_tracks_device"]["frames_per_s"] / res["score_tracks_host"]["frames_per_s"]

    nrot = 4
    st = L.current_stream()
    i32 = lambda *shape: [torch.empty(shape, dtype=torch.int32, device="cuda") for _ in range(nrot)]
    matches, counts, stats = i32(N, K), i32(N, 3), i32(M + 1, 5)
    ws = torch.empty((int(L.spnet_track_match_ws(N, K, K)),), dtype=torch.uint8, device="cuda")
    ws2 = torch.empty((int(L.spnet_track_ident_ws(N, K, M)),), dtype=torch.uint8, device="cuda")
    q = TK.iou_to_q(args.score_iou)
    p = [a.data_ptr() for a in (rows_t, count_t, ident, rows_p, count_t, track)]
    m0 = got["score_tracks_device"][0]
    steps = (("spnet_track_match", lambda i: L.spnet_track_match(p[0], p[1], p[2], K, p[3], p[4], p[5], K, N, H, W, q, M,
                                                                 ws.data_ptr(), matches[i].data_ptr(), counts[i].data_ptr(), st)),
             ("spnet_track_ident", lambda i: L.spnet_track_ident(p[0], p[1], p[2], m0.data_ptr(), p[5], N, K, K, M, ws2.data_ptr(),
                                                                 stats[i].data_ptr(), st)))
    for name, fn in steps:
        k = gpu_time(fn, nrot, window_ms=100.0)
        k["us_per_frame"] = k["us"] / N
        res[name] = k
        print(name, json.dumps(k), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
