#!/usr/bin/env python3
"""Dev tool (GPU box): what the label path costs on the host and on the device (csrc/targets.hip).

  stream   FakeStream.epoch over --stream-frames frames (331 layout) with targets="host" (labels read back, encoded in
           numpy, Y uploaded) and targets="device" (spnet_encode_targets): whole epochs, and the label path alone on
           parameters that are already drawn
  warp     one AugmentOnTheFly warp epoch over --frames frames: the file-backed callback (warp_targets="host": numpy
           targets per chunk ahead of each warp launch) against warp_source= / warp_targets="device" on the SAME frames,
           labels and draws; the two epochs' targets are compared while at it

usage: targets_time.py [--stream-frames 40000] [--frames 4096] [--out profiles/targets_time.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def timed(fn, repeat=3):
    """Wall seconds of fn() between device synchronisations: (median, min, max) of `repeat` calls after one warm-up."""
    import torch
    fn()
    t = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        t.append(time.time() - t0)
    t.sort()
    return {"seconds": t[len(t) // 2], "min": t[0], "max": t[-1]}


def stream_part(res, n):
    import torch
    from spnet_amd import augmentation as A
    from spnet_amd import fake_espi as F
    out = {"frames": n}
    X = torch.empty((n, 331, 331, 1), dtype=torch.float32, device="cuda")
    Y = torch.empty((n, 576), dtype=torch.float32, device="cuda")
    for mode in ("host", "device"):
        s = F.FakeStream(n, seed=1, size=331, targets=mode)
        epochs = iter(range(100))
        out["epoch_" + mode] = timed(lambda: s.epoch(next(epochs), X, Y, verbose=False))
    _, nodes, nnode = F.draw_params_device(n, seed=1)

    def host():
        Yh, _ = F.targets_from_labels(F.labels_from_params(nodes, nnode))
        Y.copy_(torch.from_numpy(Yh).cuda())

    def device():
        Yd, flags = A.encode_targets_device(*F.rows_from_params(nodes, nnode))
        return int((flags != 0).sum())
    out["labels_host"], out["labels_device"] = timed(host), timed(device)
    res["stream"] = out
    print("FakeStream.epoch, %d frames: host targets %.3f s, device targets %.3f s; the label path alone %.4f s -> %.4f s"
          % (n, out["epoch_host"]["seconds"], out["epoch_device"]["seconds"], out["labels_host"]["seconds"],
             out["labels_device"]["seconds"]), flush=True)


def warp_part(res, n):
    import random
    import torch
    from PIL import Image
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    from spnet_amd import fake_espi as F
    from spnet_amd import utils
    out = {"frames": n}
    _, labels, U = F.generate_device(n, seed=3, params="device", want_u8=True)
    rows, count = (torch.from_numpy(a).cuda() for a in A.pad_metadata(labels, 7))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "Train")
        os.makedirs(path)
        Uh = U.cpu().numpy()
        for i in range(n):
            stem = os.path.join(path, "steelpan_%07d" % i)
            Image.fromarray(Uh[i]).save(stem + ".png", compress_level=1)
            with open(stem + ".csv", "w") as f:
                f.write(F.rows_to_csv(labels[i]))
        X, Y, files, _ = utils.build_dataset(path=path + "/", shuffle=False)
        Xd = torch.from_numpy(X).cuda()
        cbs = {"host": C.AugmentOnTheFly(Xd, Y, warp=True, warp_files=list(files)),
               "device": C.AugmentOnTheFly(Xd, Y, warp_source=A.DeviceWarper(U, (rows, count)), warp_targets="device")}
    for mode, cb in cbs.items():
        def epoch():
            np.random.seed(7)
            random.seed(7)
            cb.on_epoch_begin(0)
        out[mode] = timed(epoch)
        out[mode]["rejected"] = cb.rejected
        out[mode]["label_seconds_on_host"] = cb.label_seconds
    diff = (cbs["host"].Y_aug - cbs["device"].Y_aug).abs()
    out["targets_max_abs_diff"] = float(diff.max())
    out["targets_entries_differing"] = int((diff != 0).sum())
    out["frames_equal"] = bool(torch.equal(cbs["host"].X_aug, cbs["device"].X_aug))
    res["warp_epoch"] = out
    print("AugmentOnTheFly warp epoch, %d frames: host targets %.3f s (%.3f s of it in warp_targets), device targets %.3f s; "
          "rejected %d / %d, frames equal %s, targets differ in %d entries by at most %.1e"
          % (n, out["host"]["seconds"], out["host"]["label_seconds_on_host"], out["device"]["seconds"], out["host"]["rejected"],
             out["device"]["rejected"], out["frames_equal"], out["targets_entries_differing"], out["targets_max_abs_diff"]),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stream-frames", type=int, default=40000)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--out", default="profiles/targets_time.json")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "targets_time.py measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0)}
    stream_part(res, args.stream_frames)
    warp_part(res, args.frames)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
