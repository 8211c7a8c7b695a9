#!/usr/bin/env python3
"""Dev tool (GPU box): what the prediction overlays cost drawn by Pillow and drawn by csrc/overlay.hip.

512 fake-ESPI frames 384 x 512 (fake_espi.generate_device) written to files, their labels as the "true" grid and a shifted
copy as the "predicted" one, through utils.show_pred_ellipses three ways, each ending in PNG files and the CSV written:
  host_draw            draw="host",   png="device"  -- the loop before this tool existed: Pillow opens, draws, uploads
  device_draw          draw="device", png="device"  -- Pillow opens, one upload and one launch per chunk
  device_draw_decode   draw="device", png="device", device_decode=True -- the files are decoded on the GPU too
One warm-up round, then `--repeats` rounds in which the ways alternate; median / min / max frames per second.  Also: the
kernel alone per launch of 64 frames (events, back-to-back launches) for these overlays and for frames with no commands,
draw_overlays_device alone (plan given, upload of the command buffers included) and plan_overlays alone on the host.

usage: overlay_time.py [--frames 512] [--repeats 5] [--tmp DIR] [--out profiles/overlay_time.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from tools.resize_time import gpu_time

CHUNK = 64


def grids(labels):
    from spnet_amd import config as cf
    v = cf.vars_per_pred
    n_pred = max(max(len(rows) for rows in labels), 1)
    Yt = np.zeros((len(labels), n_pred * v), np.float64)
    Yt[:, 6::v] = 1.0
    Yp = Yt.copy()
    for j, rows in enumerate(labels):
        for k, (cx, cy, a, b, angle, rings) in enumerate(rows):
            t = 2 * np.deg2rad(float(angle))
            Yt[j, k * v:(k + 1) * v] = (cx, cy, a, b, np.cos(t), np.sin(t), 0, rings)
            Yp[j, k * v:(k + 1) * v] = (cx + 2.6, cy - 1.7, a * 0.95, b * 1.04, np.cos(t + 0.05), np.sin(t + 0.05), 0.1, rings + 0.2)
    return Yt, Yp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a fresh temporary directory)")
    ap.add_argument("--out", default="profiles/overlay_time.json")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "overlay_time.py measures on the GPU"
    from PIL import Image
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    from spnet_amd import overlay as O
    from spnet_amd import png as P
    from spnet_amd import utils as U

    n = args.frames
    root = args.tmp or tempfile.mkdtemp(prefix="overlay_time_")
    src, out = os.path.join(root, "src"), os.path.join(root, "out")
    os.makedirs(src, exist_ok=True)
    _, labels, frames = F.generate_device(n, seed=1, want_u8=True)
    files = [os.path.join(src, "steelpan_%07d.png" % j) for j in range(n)]
    for lo in range(0, n, 256):
        P.write_png_device(frames[lo:lo + 256], files[lo:lo + 256])
    Yt, Yp = grids(labels)
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "chunk": CHUNK, "pillow": Image.__version__,
           "cpus_usable": len(os.sched_getaffinity(0)),
           "ellipses_per_frame": 2 * sum(len(r) for r in labels) / n}

    ways = (("host_draw", dict(draw="host")), ("device_draw", dict(draw="device")),
            ("device_draw_decode", dict(draw="device", device_decode=True)))
    times = {k: [] for k, _ in ways}
    for rnd in range(args.repeats + 1):              # round 0 warms up: code objects, allocator, fonts, page cache
        for name, kw in ways:
            os.makedirs(out, exist_ok=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            U.show_pred_ellipses(Yt, Yp, files, num_draw=n, log_dir=out, out_csv=os.path.join(out, "pred.csv"), png="device",
                                 png_chunk=CHUNK, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(os.listdir(out)) == n + 1
            shutil.rmtree(out)
            if rnd:
                times[name].append(dt)
    for name, _ in ways:
        t = sorted(times[name])
        res[name] = {"frames_per_s": n / t[len(t) // 2], "min_frames_per_s": n / t[-1], "max_frames_per_s": n / t[0],
                     "ms_per_frame": 1e3 * t[len(t) // 2] / n, "rounds": len(t)}
        print(name, json.dumps(res[name]), flush=True)
    res["device_over_host_draw"] = res["device_draw"]["frames_per_s"] / res["host_draw"]["frames_per_s"]
    res["device_decode_over_host_draw"] = res["device_draw_decode"]["frames_per_s"] / res["host_draw"]["frames_per_s"]

    # the parts: plan on the host, the wrapper, the kernel
    m = min(CHUNK, n)
    t0 = time.perf_counter()
    plan = O.plan_overlays(Yt[:m], Yp[:m], files[:m], size=(384, 512))
    res["plan_overlays_host_ms_per_frame"] = 1e3 * (time.perf_counter() - t0) / m
    dev = frames[:m].contiguous()
    torch.cuda.synchronize()
    t = []
    for _ in range(args.repeats + 1):
        t0 = time.perf_counter()
        O.draw_overlays_device(dev, plan)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    t = sorted(t[1:])
    res["draw_overlays_device"] = {"frames_per_s": m / t[len(t) // 2], "min_frames_per_s": m / t[-1], "max_frames_per_s": m / t[0]}
    host = np.concatenate([plan.frame_start.view(np.uint8), plan.cmd.reshape(-1).view(np.uint8),
                           plan.verts.reshape(-1).view(np.uint8), plan.masks])
    blob = torch.from_numpy(host).cuda()
    p = blob.data_ptr()
    o0 = 4 * plan.frame_start.size
    o1 = o0 + 4 * plan.cmd.size
    o2 = o1 + 4 * plan.verts.size
    nrot = 8                                          # 8 x (12.6 + 37.7) MB: launches read and write cold lines
    srcs = [dev.clone() for _ in range(nrot)]
    outs = [torch.empty((m, 384, 512, 3), dtype=torch.uint8, device="cuda") for _ in range(nrot)]
    st = L.current_stream()
    k = gpu_time(lambda i: L.spnet_draw_overlays(srcs[i].data_ptr(), m, 384, 512, 1, p, p + o0, int(plan.cmd.shape[0]), p + o1,
                                                 int(plan.verts.shape[0]), p + o2, int(plan.masks.size), outs[i].data_ptr(), st),
                 nrot, window_ms=100.0)
    k["us_per_frame"] = k["us"] / m
    k["commands"] = int(plan.cmd.shape[0])
    res["spnet_draw_overlays"] = k
    zero = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    k0 = gpu_time(lambda i: L.spnet_draw_overlays(srcs[i].data_ptr(), m, 384, 512, 1, zero.data_ptr(), p + o0, 0, p + o1, 0,
                                                  p + o2, 0, outs[i].data_ptr(), st), nrot, window_ms=100.0)
    k0["us_per_frame"] = k0["us"] / m
    k0["GB_per_s"] = m * 384 * 512 * 4 / (k0["us"] * 1e-6) / 1e9
    res["spnet_draw_overlays_no_commands"] = k0
    print("kernel:", json.dumps(k), json.dumps(k0), flush=True)

    if args.tmp is None:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
