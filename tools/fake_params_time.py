#!/usr/bin/env python3
"""Dev tool (GPU box): what drawing the fake-ESPI parameters costs on the host and on the device.

  generate   fake_espi.generate_device(n) with params="host" (draw_params per frame, Python `random` + numpy) against
             params="device" (spnet_fake_espi_params), same process, wall time of the second call of each
  kernel     spnet_fake_espi_params alone over n frames, timed with events (median / min / max of 5 windows)
  epoch      FakeStream.epoch(n, size=331): generate + one label copy per chunk + targets_from_labels, and the host share
             spent in labels_from_params and in the target codec

usage: fake_params_time.py [--frames 4096] [--out profiles/fake_params_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.resize_time import gpu_time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--out", default="profiles/fake_params_time.json")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "fake_params_time.py measures on the GPU"
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    n = args.frames
    res = {"device": torch.cuda.get_device_name(0), "frames": n}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.time()
        out = fn()
        torch.cuda.synchronize()
        return time.time() - t0, out

    gen = {}
    for params in ("host", "device"):
        wall(lambda: F.generate_device(min(n, 64), seed=1, params=params))          # warm-up: allocator, tables
        t, _ = wall(lambda: F.generate_device(n, seed=1, params=params))
        gen[params] = {"seconds": t, "ms_per_frame": 1e3 * t / n}
    t, _ = wall(lambda: [F.draw_params(s) for s in F.frame_seeds(n, 1)])
    gen["draw_params_alone"] = {"seconds": t, "ms_per_frame": 1e3 * t / n}
    res["generate_device"] = gen
    print("generate_device(%d): params='host' %.3f s (%.3f ms/frame; draw_params alone %.3f ms/frame), params='device' "
          "%.3f s (%.4f ms/frame)" % (n, gen["host"]["seconds"], gen["host"]["ms_per_frame"],
                                      gen["draw_params_alone"]["ms_per_frame"], gen["device"]["seconds"],
                                      gen["device"]["ms_per_frame"]), flush=True)

    waves, nodes, nnode, tries = F.draw_params_device(n, seed=1, want_tries=True)
    t2 = F.trig2_table("cuda")
    st = L.current_stream()
    kern = {}
    for name, cr in (("count_1_7", (1, 7)), ("count_7_7", (7, 7))):
        k = gpu_time(lambda i: L.spnet_fake_espi_params(0, n, F.IM_H, F.IM_W, 1, cr[0], cr[1], t2.data_ptr(), waves.data_ptr(),
                                                        nodes.data_ptr(), nnode.data_ptr(), tries.data_ptr(), st), 1,
                     window_ms=100.0)
        k["us_per_frame"] = k["us"] / n
        kern[name] = k
        print("kernel alone, %d frames, count range %s: %.1f us per launch (%.1f-%.1f) = %.4f us per frame"
              % (n, cr, k["us"], k["min_us"], k["max_us"], k["us_per_frame"]), flush=True)
    res["kernel"] = kern

    # where the time of a streamed epoch goes
    stream = F.FakeStream(n, seed=1, size=331)
    stream.epoch(0, verbose=False)
    t_epoch, _ = wall(lambda: stream.epoch(1, verbose=False))
    t_frames, (X, labels) = wall(lambda: stream.frames(n, n))
    wv, nd, nn = F.draw_params_device(n, seed=1, first_frame=n)
    t_labels, labels2 = wall(lambda: F.labels_from_params(nd, nn))
    t0 = time.time()
    F.targets_from_labels(labels)
    t_targets = time.time() - t0
    res["epoch"] = {"seconds": t_epoch, "generate_device_seconds": t_frames, "labels_from_params_seconds": t_labels,
                    "targets_from_labels_seconds": t_targets, "size": 331}
    print("FakeStream.epoch(%d frames, 331 layout): %.3f s; of it generate_device %.3f s (labels_from_params %.3f s), "
          "targets_from_labels %.3f s" % (n, t_epoch, t_frames, t_labels, t_targets), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
