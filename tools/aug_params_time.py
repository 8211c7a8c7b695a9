#!/usr/bin/env python3
"""Dev tool (GPU box): what drawing the on-the-fly augmentation's random parameters costs on the host and on the device.

One augmentation pass (AugmentOnTheFly.on_epoch_begin) over --frames streamed fake-ESPI frames in chunks of --chunk, with
params="host" (per-frame numpy / Python draws in the reference's order, packed and uploaded per chunk) against
params="device" (one spnet_augment_params launch per chunk, nothing uploaded), both callbacks alive in the SAME process on
the same frames and timed alternately, --rounds times each after one warm-up pass of each:

  plain    cutout + salt and pepper (+ the blur gate)
  warp     the same behind the warp of a warp_source (FreshFakeESPI(warper=True), targets on the device)
  kernel   spnet_augment_params alone over one chunk, both halves and the augmentation half only (events)

Per pass: `seconds` = wall time to the end of the device work (synchronised), `host_seconds` = until on_epoch_begin returns.
Each step runs in a fresh child process under its own time limit; a step that fails or runs out of time ends the tool (no
further step is started).

usage: aug_params_time.py [--frames 8192] [--chunk 256] [--size native|331] [--rounds 5] [--out profiles/aug_params_time.json]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("plain", 300), ("warp", 300), ("kernel", 120))       # (name, time limit in seconds)


def _stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def pass_step(warp, args):
    import contextlib
    import io
    import torch
    from spnet_amd import callbacks as C
    from spnet_amd import fake_espi as F
    n = args.frames
    stream = F.FakeStream(n, seed=1, size=None if args.size == "native" else 331)
    fresh = C.FreshFakeESPI(None, None, stream, verbose=False, warper=bool(warp))
    kw = dict(warp_source=fresh.warper, warp_targets="device") if warp else {}
    cbs = {m: C.AugmentOnTheFly(fresh.X, fresh.Y, chunk=args.chunk, seed=1, params=m, **kw) for m in ("host", "device")}
    times = {m: {"seconds": [], "host_seconds": []} for m in cbs}

    def one(mode, epoch):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            cbs[mode].on_epoch_begin(epoch)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0

    for m in cbs:                               # warm-up: code objects, allocator, pinned rings, tables
        one(m, 0)
    for r in range(args.rounds):                # alternating, so that what else runs on the host hits both alike
        for m in ("host", "device"):
            total, host = one(m, 1 + r)
            times[m]["seconds"].append(total)
            times[m]["host_seconds"].append(host)
    res = {"frames": n, "chunk": args.chunk, "frame_size": list(fresh.X.shape[1:3]), "rounds": args.rounds,
           "gpu": torch.cuda.get_device_name(0)}
    for m in cbs:
        res[m] = {k: _stats(v) for k, v in times[m].items()}
        res[m]["us_per_frame"] = 1e6 * res[m]["seconds"]["median"] / n
    if warp:
        res["rejected_last_pass"] = {m: cbs[m].rejected for m in cbs}
    res["host_over_device"] = res["host"]["seconds"]["median"] / res["device"]["seconds"]["median"]
    return res


def kernel_step(args):
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import augmentation as A
    from tools.resize_time import gpu_time
    B = args.chunk
    H, W = (384, 512) if args.size == "native" else (331, 331)
    X = torch.rand((B, H, W, 1), device="cuda") * 2 - 1
    aug = A.DeviceAugmenter(X)
    wr = A.DeviceWarper(torch.zeros((B, 384, 512), dtype=torch.uint8, device="cuda"),
                        (torch.zeros((B, 7, 6), dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")))
    idx = torch.arange(B, dtype=torch.int32, device="cuda")
    ap, wp = A.draw_params_device(idx, 1, 0, augmenter=aug, warper=wr)
    st = L.current_stream()
    a = [H, W, aug.n_salt, aug.n_pepper, aug.mm.data_ptr(), B] + [ap[k].data_ptr() for k in ("rects", "vals", "nrect", "coords", "flag", "ksize")]
    w = [384, 512, A.aug_trig_table("cuda").data_ptr(), wp["records"].data_ptr(), wp["fwd"].data_ptr()]
    res = {"samples": B, "frame_size": [H, W], "gpu": torch.cuda.get_device_name(0)}
    for name, tail in (("both_halves", w), ("augmentation_only", [0, 0, None, None, None])):
        res[name] = gpu_time(lambda i: L.spnet_augment_params(1, i, idx.data_ptr(), B, *a, *tail, st), 1 << 30, window_ms=100.0)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=256)
    ap.add_argument("--size", choices=("native", "331"), default="native")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="profiles/aug_params_time.json")
    ap.add_argument("--step", choices=[s for s, _ in STEPS], help="(internal) run one step in this process")
    ap.add_argument("--part-out", help="(internal) where the step writes its result")
    args = ap.parse_args()
    if args.step:
        import torch
        assert torch.cuda.is_available(), "aug_params_time.py measures on the GPU"
        res = kernel_step(args) if args.step == "kernel" else pass_step(args.step == "warp", args)
        with open(args.part_out, "w") as f:
            json.dump(res, f)
        return 0
    out = {"frames": args.frames, "chunk": args.chunk, "size": args.size}
    for name, limit in STEPS:
        with tempfile.TemporaryDirectory() as d:
            part = os.path.join(d, "part.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--part-out", part, "--frames", str(args.frames),
                   "--chunk", str(args.chunk), "--size", args.size, "--rounds", str(args.rounds)]
            try:
                r = subprocess.run(cmd, timeout=limit, cwd=ROOT)
            except subprocess.TimeoutExpired:
                print("step %s did not finish within %d s: stopping here" % (name, limit), flush=True)
                return 1
            if r.returncode != 0:
                print("step %s failed with exit status %d: stopping here" % (name, r.returncode), flush=True)
                return 1
            with open(part) as f:
                out[name] = json.load(f)
        s = out[name]
        if name == "kernel":
            print("kernel alone, %d samples: both halves %.1f us, augmentation only %.1f us per launch"
                  % (s["samples"], s["both_halves"]["us"], s["augmentation_only"]["us"]), flush=True)
        else:
            print("%-5s pass over %d frames of %dx%d: params='host' %.3f s (%.3f-%.3f; host side %.3f s), params='device' %.3f s "
                  "(%.3f-%.3f; host side %.3f s): x%.2f"
                  % (name, s["frames"], s["frame_size"][0], s["frame_size"][1], s["host"]["seconds"]["median"],
                     s["host"]["seconds"]["min"], s["host"]["seconds"]["max"], s["host"]["host_seconds"]["median"],
                     s["device"]["seconds"]["median"], s["device"]["seconds"]["min"], s["device"]["seconds"]["max"],
                     s["device"]["host_seconds"]["median"], s["host_over_device"]), flush=True)
    out["gpu"] = out["plain"]["gpu"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
