#!/usr/bin/env python3
"""Dev tool (GPU box): what linking antinodes through a movie costs on the host and on the device.

A seeded sequence of `--frames` frames (default 4,096) at 384 x 512: the streamed parameter sampler's label sets
(fake_espi.draw_params_device), one per segment of 32 frames, every ellipse drifting up to 3 px a frame in a direction of its
own within its segment (a new label set starts a new segment, so tracks end and start there).  Two ways, IoU 0.25, gap 1:
  host     tracks.link_tracks_host on the FIRST `--host_frames` frames only (default 128; the numpy rule is slow), rows on
           the host
  device   tracks.link_tracks_device on ALL frames, rows in HBM, results left there
One warm-up round, then `--repeats` rounds in which the two alternate in this one process; median / min / max frames per
second each.  The device's track and age of the first host_frames frames are checked against the host's (a track depends on
earlier frames only).  Also the four entry points alone on the whole sequence (events around back-to-back launches over
rotating output buffers): area, overlap, link, rank.

usage: tracks_time.py [--frames 4096] [--host_frames 128] [--repeats 5] [--out profiles/tracks_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resize_time import gpu_time

H, W, SEGMENT = 384, 512, 32


def sequence(n, seed=1):
    """(rows float64 [n,K,6], count int32 [n]) on the device."""
    import torch
    from spnet_amd import fake_espi as F
    segs = (n + SEGMENT - 1) // SEGMENT
    _, nodes, nnode = F.draw_params_device(segs, seed=seed)
    base, cnt = F.rows_from_params(nodes, nnode)
    g = torch.Generator(device="cpu").manual_seed(seed)
    vel = (torch.rand((segs, base.shape[1], 2), generator=g, dtype=torch.float64) * 6.0 - 3.0).to(base.device)
    t = torch.arange(n, device=base.device)
    rows = base[t // SEGMENT].clone()
    rows[..., :2] += vel[t // SEGMENT] * (t % SEGMENT).to(torch.float64)[:, None, None]
    rows[..., :2] = torch.round(rows[..., :2] * 16.0) / 16.0
    return rows.contiguous(), cnt[t // SEGMENT].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--host_frames", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/tracks_time.json")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "tracks_time.py measures on the GPU"
    from spnet_amd import _lib as L
    from spnet_amd import tracks as TK

    n, nh = args.frames, min(args.host_frames, args.frames)
    rows_d, count_d = sequence(n)
    rows_h, count_h = rows_d[:nh].cpu().numpy(), count_d[:nh].cpu().numpy()
    K = int(rows_d.shape[1])
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "host_frames": nh, "H": H, "W": W, "K": K, "iou": 0.25,
           "max_gap": 1, "cpus_usable": len(os.sched_getaffinity(0)), "ellipses_per_frame": float(count_d.sum()) / n,
           "note": "the host way runs on the first host_frames frames only; its rate is frames of that run per second"}

    got = {}

    def host():
        got["host"] = TK.link_tracks_host(rows_h, count_h, H, W)

    def device():
        got["device"] = TK.link_tracks_device(rows_d, count_d, H, W)

    ways = (("host", host, nh), ("device", device, n))
    times = {k: [] for k, _, _ in ways}
    for rnd in range(args.repeats + 1):              # round 0 warms up: code objects, allocator
        for name, fn, _ in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
        if rnd == 0:
            for k in (0, 1):                         # track, age: the same integers
                assert np.array_equal(got["device"][k][:nh].cpu().numpy(), got["host"][k]), k
            track = got["device"][0].cpu().numpy()
            res["tracks"] = int(np.unique(track[track > 0]).size)
            res["longest_track"] = int(got["device"][1].max()) + 1
    for name, _, frames in ways:
        t = sorted(times[name])
        res[name] = {"frames_per_s": frames / t[len(t) // 2], "min_frames_per_s": frames / t[-1],
                     "max_frames_per_s": frames / t[0], "ms_per_frame": 1e3 * t[len(t) // 2] / frames, "rounds": len(t),
                     "frames": frames}
        print(name, json.dumps(res[name]), flush=True)
    res["device_over_host"] = res["device"]["frames_per_s"] / res["host"]["frames_per_s"]

    # the entry points alone, on the whole sequence
    nrot = 4
    st = L.current_stream()
    rp, cp = rows_d.data_ptr(), count_d.data_ptr()
    i32 = lambda *shape: [torch.empty(shape, dtype=torch.int32, device="cuda") for _ in range(nrot)]
    areas, inters, tracks_, ages = i32(n, K), i32(max(n - 1, 1), K, K), i32(n, K), i32(n, K)
    nexts = [torch.full((n, K), -1, dtype=torch.int32, device="cuda") for _ in range(nrot)]
    prevs = [torch.full((n, K), -1, dtype=torch.int32, device="cuda") for _ in range(nrot)]
    ws = torch.empty((int(L.spnet_track_rank_ws(n, K)),), dtype=torch.uint8, device="cuda")
    area, prev = got["device"][4], got["device"][3]
    steps = (("spnet_track_area", lambda i: L.spnet_track_area(rp, cp, n, K, H, W, areas[i].data_ptr(), st)),
             ("spnet_track_overlap", lambda i: L.spnet_track_overlap(rp, cp, n, K, H, W, 0, n - 1, 1, inters[i].data_ptr(), st)),
             # next / prev are refilled with -1 before every launch (a linked slot would leave nothing open to link): the
             # figure holds the two fills of n x K int32
             ("spnet_track_link", lambda i: (nexts[i].fill_(-1), prevs[i].fill_(-1),
                                             L.spnet_track_link(inters[0].data_ptr(), area.data_ptr(), rp, cp, n, K, 0, n - 1, 1,
                                                                256, nexts[i].data_ptr(), prevs[i].data_ptr(), st))),
             ("spnet_track_rank", lambda i: L.spnet_track_rank(prev.data_ptr(), rp, cp, n, K, tracks_[i].data_ptr(),
                                                               ages[i].data_ptr(), ws.data_ptr(), st)))
    for name, fn in steps:
        if n < 2 and name in ("spnet_track_overlap", "spnet_track_link"):
            continue
        k = gpu_time(fn, nrot, window_ms=100.0)
        k["us_per_frame"] = k["us"] / n
        res[name] = k
        print(name, json.dumps(k), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
