#!/usr/bin/env python3
"""Dev tool (GPU box): what fitting ellipses to ring-count masks costs on the host and on the device.

512 fake-ESPI label sets at 384 x 512 from the streamed parameter sampler (fake_espi.draw_params_device), painted by
masks.ring_masks_device; the masks are then fitted to ellipse rows three ways:
  host     masks.ellipses_from_masks_host on the masks in host memory (the product's rule without a GPU)
  scipy    scipy.ndimage.label per value + numpy moments, where scipy imports (what one would write without this project)
  device   masks.ellipses_from_masks_device on the masks in HBM (five launches, the sums to the host, the rows back)
One warm-up round, then `--repeats` rounds in which the ways alternate in this one process; median / min / max frames per
second.  The device rows are checked against the host rows bit for bit in the warm-up round.  Also the two entry points alone
(events around back-to-back launches over rotating buffers): spnet_mask_label (its three launches) and spnet_mask_moments
(its two).  The five kernels are not exported one by one, so their split inside an entry point is not measured here.

usage: mask_fit_time.py [--frames 512] [--repeats 5] [--host_frames N] [--out profiles/mask_fit_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resize_time import gpu_time

H, W = 384, 512


def scipy_fit(masks_h):
    """Per frame and value: ndimage.label with the 3 x 3 structure, then the same sums by np.bincount (float64 weights:
    exact at this size).  Returns the number of components found."""
    import numpy as np
    from scipy import ndimage
    total = 0
    yy, xx = np.mgrid[0:H, 0:W]
    for frame in masks_h:
        for v in np.unique(frame[frame > 0]):
            lab, n = ndimage.label(frame == v, np.ones((3, 3)))
            sel = lab > 0
            l, x, y = lab[sel], xx[sel].astype(np.float64), yy[sel].astype(np.float64)
            for w in (None, x, y, x * x, y * y, x * y):
                np.bincount(l, weights=w, minlength=n + 1)
            total += n
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host_frames", type=int, default=None,
                    help="the host and scipy ways fit only the first N frames (default: all); rates are per frame either way")
    ap.add_argument("--out", default="profiles/mask_fit_time.json")
    args = ap.parse_args()
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "mask_fit_time.py measures on the GPU"
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    from spnet_amd import masks as MK

    n = args.frames
    _, nodes, nnode = F.draw_params_device(n, seed=1)
    rows_d, count_d = F.rows_from_params(nodes, nnode)
    masks_d = MK.ring_masks_device(rows_d, count_d, H=H, W=W)
    nh = n if args.host_frames is None else min(n, args.host_frames)
    masks_h = masks_d[:nh].cpu().numpy()
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "H": H, "W": W, "numpy": np.__version__,
           "cpus_usable": len(os.sched_getaffinity(0)), "host_frames": nh, "ellipses_per_frame": float(count_d.sum()) / n}

    ways = [("host", lambda: MK.ellipses_from_masks_host(masks_h, overflow="truncate")),
            ("device", lambda: MK.ellipses_from_masks_device(masks_d, overflow="truncate"))]
    try:
        import scipy
        res["scipy"] = scipy.__version__
        ways.insert(1, ("scipy", lambda: scipy_fit(masks_h)))
    except ImportError:
        res["scipy"] = None
    frames_of = {"host": nh, "scipy": nh, "device": n}
    times, got = {k: [] for k, _ in ways}, {}
    for rnd in range(args.repeats + 1):              # round 0 warms up: code objects, allocator
        for name, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got[name] = fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
        if rnd == 0:
            assert np.array_equal(got["device"][0][:nh].cpu().numpy().view(np.uint64), got["host"][0].view(np.uint64))
            assert np.array_equal(got["device"][1][:nh].cpu().numpy(), got["host"][1])
            res["components_per_frame"] = float(got["device"][1].sum()) / n
    for name, _ in ways:
        t, nf = sorted(times[name]), frames_of[name]
        res[name + "_fit"] = {"frames_per_s": nf / t[len(t) // 2], "min_frames_per_s": nf / t[-1],
                              "max_frames_per_s": nf / t[0], "ms_per_frame": 1e3 * t[len(t) // 2] / nf, "rounds": len(t),
                              "frames": nf}
        print(name, json.dumps(res[name + "_fit"]), flush=True)
    res["device_over_host"] = res["device_fit"]["frames_per_s"] / res["host_fit"]["frames_per_s"]

    # the entry points alone
    nrot = 4
    st = L.current_stream()
    src = [masks_d.clone() for _ in range(nrot)]
    labels = [torch.empty((n, H, W), dtype=torch.int32, device="cuda") for _ in range(nrot)]
    ncomp = torch.empty((n,), dtype=torch.int32, device="cuda")
    sums = torch.empty((n, MK.MAX_K, 8), dtype=torch.int64, device="cuda")
    k = gpu_time(lambda i: L.spnet_mask_label(src[i].data_ptr(), n, H, W, 0, labels[i].data_ptr(), st), nrot, window_ms=100.0)
    k["us_per_frame"] = k["us"] / n
    k["launches"] = 3
    k["GB_per_s_mask_read_label_written"] = 5 * n * H * W / (k["us"] * 1e-6) / 1e9
    res["spnet_mask_label"] = k
    m = gpu_time(lambda i: L.spnet_mask_moments(src[i].data_ptr(), labels[i].data_ptr(), n, H, W, MK.MAX_K, ncomp.data_ptr(),
                                                sums.data_ptr(), st), nrot, window_ms=100.0)
    m["us_per_frame"] = m["us"] / n
    m["launches"] = 2
    res["spnet_mask_moments"] = m
    print("entry points:", json.dumps(k), json.dumps(m), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
