#!/usr/bin/env python3
"""Dev tool (GPU box): what ring-count masks cost painted and written on the host and on the device.

512 fake-ESPI label sets at 384 x 512 from the streamed parameter sampler (fake_espi.draw_params_device), two ways, each
ending in one PNG file per mask:
  host     masks.ring_masks_host on the label rows, written by Pillow (write_masks' default)
  device   masks.ring_masks_device on the rows in HBM, written by write_masks(png="device-lz")
One warm-up round, then `--repeats` rounds in which the two alternate in this one process; median / min / max masks per
second and the bytes of the files each wrote.  Also the two kernels alone (events around back-to-back launches over
rotating buffers): spnet_ring_masks on these rows, spnet_mask_compare on these masks against a shifted copy.

usage: masks_time.py [--frames 512] [--repeats 5] [--tmp DIR] [--out profiles/masks_time.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resize_time import gpu_time

H, W = 384, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a fresh temporary directory)")
    ap.add_argument("--out", default="profiles/masks_time.json")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "masks_time.py measures on the GPU"
    from PIL import Image
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    from spnet_amd import masks as MK

    n = args.frames
    root = args.tmp or tempfile.mkdtemp(prefix="masks_time_")
    _, nodes, nnode = F.draw_params_device(n, seed=1)
    labels = F.labels_from_params(nodes, nnode)
    rows_d, count_d = F.rows_from_params(nodes, nnode)
    res = {"device": torch.cuda.get_device_name(0), "frames": n, "H": H, "W": W, "pillow": Image.__version__,
           "cpus_usable": len(os.sched_getaffinity(0)), "ellipses_per_frame": sum(len(r) for r in labels) / n}

    def host(paths):
        MK.write_masks(MK.ring_masks_host(labels, H=H, W=W), paths)

    def device(paths):
        MK.write_masks(MK.ring_masks_device(rows_d, count_d, H=H, W=W), paths, png="device-lz")

    ways = (("host", host), ("device", device))
    times, sizes = {k: [] for k, _ in ways}, {}
    for rnd in range(args.repeats + 1):              # round 0 warms up: code objects, allocator, page cache
        for name, fn in ways:
            out = os.path.join(root, name)
            os.makedirs(out, exist_ok=True)
            paths = [os.path.join(out, "steelpan_%07d.png" % j) for j in range(n)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(paths)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            sizes[name] = sum(os.path.getsize(p) for p in paths)
            if rnd == 0 and name == "device":        # the two ways wrote the same pixels
                import numpy as np
                for j in (0, n // 2, n - 1):
                    a = np.asarray(Image.open(paths[j]))
                    b = np.asarray(Image.open(os.path.join(root, "host", os.path.basename(paths[j]))))
                    assert np.array_equal(a, b), j
            if rnd:
                times[name].append(dt)
            if name == "device" or rnd == args.repeats:
                shutil.rmtree(out)
    for name, _ in ways:
        t = sorted(times[name])
        res[name] = {"masks_per_s": n / t[len(t) // 2], "min_masks_per_s": n / t[-1], "max_masks_per_s": n / t[0],
                     "ms_per_mask": 1e3 * t[len(t) // 2] / n, "rounds": len(t), "file_bytes": sizes[name],
                     "bytes_per_mask": sizes[name] / n}
        print(name, json.dumps(res[name]), flush=True)
    res["device_over_host"] = res["device"]["masks_per_s"] / res["host"]["masks_per_s"]

    # the kernels alone
    nrot = 8
    st = L.current_stream()
    outs = [torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(nrot)]
    K = int(rows_d.shape[1])
    k = gpu_time(lambda i: L.spnet_ring_masks(rows_d.data_ptr(), count_d.data_ptr(), n, K, H, W, outs[i].data_ptr(), st),
                 nrot, window_ms=100.0)
    k["us_per_mask"] = k["us"] / n
    k["GB_per_s_written"] = n * H * W / (k["us"] * 1e-6) / 1e9
    res["spnet_ring_masks"] = k
    shifted = [torch.roll(o, shifts=(3, 5), dims=(1, 2)).contiguous() for o in outs]
    counts = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    c = gpu_time(lambda i: L.spnet_mask_compare(outs[i].data_ptr(), shifted[i].data_ptr(), n, H * W, 5, counts.data_ptr(), st),
                 nrot, window_ms=100.0)
    c["us_per_mask"] = c["us"] / n
    c["GB_per_s_read"] = 2 * n * H * W / (c["us"] * 1e-6) / 1e9
    res["spnet_mask_compare"] = c
    res["compare_of_last_launch"] = MK.metrics_from_counts(*counts.sum(0).tolist())
    print("kernels:", json.dumps(k), json.dumps(c), flush=True)

    if args.tmp is None:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
