#! /usr/bin/env python3
"""Times the device JPEG decoder against the default path (Pillow decode + upload), in ONE process, alternating over
rounds, on 512 grey 384 x 512 fake-ESPI-like frames in two forms: files written by this project's encoder (one restart
interval per MCU row) and Pillow-written files without restart markers (one interval per file).  Writes
profiles/jpeg_decode_time.json: files/s of read_jpeg_device (files on disk), decode_jpeg_device (bytes in memory),
MjpegReader.read_device (our files only: Pillow's go into the same container) and the default path over 16 worker threads,
and the kernels' own times (HIP events around each launch of a second, instrumented pass).  For the files without restart
markers every entry point also runs with entropy="interval" (one serial lane per file: the path before
spnet_jpeg_entropy_sync existed) and entropy="sync", alternating with the default in the same rounds; the sync kernel is
timed alone at every candidate segment size; a sweep over restart-interval lengths (Pillow's restart_marker_rows) times
both entropy kernels on the same intervals, which is where SYNC_MIN_BYTES comes from; colour files (4:4:4, 4:2:0) are
timed separately, since a speculative lane can lock onto the right bits in the wrong block of the MCU.

  python tools/jpeg_decode_time.py [--frames 512] [--rounds 5] [--out profiles/jpeg_decode_time.json]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_like_espi(n, H=384, W=512, seed=0):
    """Smooth fringes plus sensor noise: the statistics of the frames this project reads, without the rasteriser."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = np.empty((n, H, W), np.uint8)
    for k in range(n):
        cx, cy, f = rng.uniform(100, 400), rng.uniform(80, 300), rng.uniform(0.02, 0.08)
        r = np.hypot(xx - cx, yy - cy)
        img = 110 + 70 * np.cos(f * r * r / 20) * np.exp(-r / 300) + rng.normal(0, 12, (H, W))
        out[k] = np.clip(img, 0, 255).astype(np.uint8)
    return out


SEG_CANDIDATES = (16, 32, 64, 128, 256, 512)


def sync_kernel_times(J, L, torch, datas, segs=SEG_CANDIDATES):
    """{"spnet_jpeg_entropy": ms, "spnet_jpeg_entropy_sync": {seg_bytes: ms}, "mean_interval_bytes": ...} of one batch: both
    entropy kernels on the SAME intervals (the sync kernel takes them unpadded), best of 5; the sync kernel's workspace
    and status must be the serial kernel's."""
    infos = [J.parse_jpeg(d) for d in datas]
    plan = J.plan_decode(infos)
    real = np.ascontiguousarray(plan["intervals"][plan["intervals"][:, 4] > 0])
    dev = {k: torch.from_numpy(plan[k].view(np.uint8).reshape(-1).copy()).cuda() for k in ("intervals", "files", "tables",
                                                                                           "blob")}
    dev_real = torch.from_numpy(real.view(np.uint8).reshape(-1).copy()).cuda()
    n = len(infos)

    def run(seg):
        coef = torch.zeros((plan["blocks"], 64), dtype=torch.int16, device="cuda")
        status = torch.zeros((n,), dtype=torch.int32, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        if seg is None:
            L.spnet_jpeg_entropy(dev["blob"].data_ptr(), int(plan["blob"].size), dev["intervals"].data_ptr(),
                                 int(plan["intervals"].shape[0]), dev["files"].data_ptr(), n, dev["tables"].data_ptr(),
                                 int(plan["tables"].shape[0]), coef.data_ptr(), int(plan["blocks"]), status.data_ptr(),
                                 L.current_stream())
        else:
            L.spnet_jpeg_entropy_sync(dev["blob"].data_ptr(), int(plan["blob"].size), dev_real.data_ptr(),
                                      int(real.shape[0]), dev["files"].data_ptr(), n, dev["tables"].data_ptr(),
                                      int(plan["tables"].shape[0]), seg, coef.data_ptr(), int(plan["blocks"]),
                                      status.data_ptr(), L.current_stream())
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), coef, status

    _, want, want_status = run(None)
    assert not want_status.cpu().numpy().any()
    out = dict(intervals=int(real.shape[0]), mean_interval_bytes=int((real[:, 1] - real[:, 0]).mean()),
               spnet_jpeg_entropy=round(min(run(None)[0] for _ in range(5)), 3), spnet_jpeg_entropy_sync={})
    for seg in segs:
        _, coef, status = run(seg)
        assert torch.equal(coef, want) and torch.equal(status, want_status), seg
        out["spnet_jpeg_entropy_sync"][str(seg)] = round(min(run(seg)[0] for _ in range(5)), 3)
    return out


def kernel_times(J, L, torch, datas):
    """(entropy ms, pixels ms) of one batch, by events around the two launches."""
    infos = [J.parse_jpeg(d) for d in datas]
    plan = J.plan_decode(infos)
    H, W = infos[0].height, infos[0].width
    dev = {k: torch.from_numpy(plan[k].view(np.uint8).reshape(-1).copy()).cuda() for k in ("intervals", "files", "tables",
                                                                                           "quant", "blob")}
    n = len(infos)
    status = torch.empty((n,), dtype=torch.int32, device="cuda")
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    best = [1e30, 1e30]
    for _ in range(5):
        coef = torch.zeros((plan["blocks"], 64), dtype=torch.int16, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        L.spnet_jpeg_entropy(dev["blob"].data_ptr(), int(plan["blob"].size), dev["intervals"].data_ptr(),
                             int(plan["intervals"].shape[0]), dev["files"].data_ptr(), n, dev["tables"].data_ptr(),
                             int(plan["tables"].shape[0]), coef.data_ptr(), int(plan["blocks"]), status.data_ptr(),
                             L.current_stream())
        ev[1].record()
        L.spnet_jpeg_pixels(coef.data_ptr(), int(plan["blocks"]), dev["files"].data_ptr(), n, dev["quant"].data_ptr(),
                            int(plan["quant"].shape[0]), H, W, 1, out.data_ptr(), 0, status.data_ptr(), L.current_stream())
        ev[2].record()
        torch.cuda.synchronize()
        best = [min(best[0], ev[0].elapsed_time(ev[1])), min(best[1], ev[1].elapsed_time(ev[2]))]
    assert not status.cpu().numpy().any()
    return best


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_decode_time.json"))
    args = ap.parse_args()
    import torch
    from PIL import Image
    from spnet_amd import _lib as L
    from spnet_amd import jpeg as J
    if not torch.cuda.is_available():
        sys.exit("jpeg_decode_time: needs a GPU")
    frames = frames_like_espi(args.frames)
    N = args.frames
    ours = []
    for lo in range(0, N, 64):
        ours += J.encode_jpeg_device(torch.from_numpy(frames[lo:lo + 64]).cuda(), args.quality)
    pillow = []
    for f in frames:
        b = io.BytesIO()
        Image.fromarray(f).save(b, "JPEG", quality=args.quality)
        pillow.append(b.getvalue())

    def default_path(paths):
        def one(p):
            return np.asarray(Image.open(p).convert("RGB"), dtype=np.uint8)[:, :, 0]
        with ThreadPoolExecutor(max_workers=J.MAX_THREADS) as pool:
            host = np.stack(list(pool.map(one, paths)))
        return torch.from_numpy(host).cuda()

    result = dict(frames=N, size=[384, 512], quality=args.quality, rounds=args.rounds, host_workers=J.MAX_THREADS,
                  device=torch.cuda.get_device_name(0), default_entropy=J.DEFAULT_ENTROPY, sync_min_bytes=J.SYNC_MIN_BYTES,
                  sync_seg_bytes=J.SYNC_SEG_BYTES, sync_workgroup_lanes=256, sources={})
    with tempfile.TemporaryDirectory() as tmp:
        for name, files in (("ours_restart_per_mcu_row", ours), ("pillow_no_restart_markers", pillow)):
            paths = []
            for k, data in enumerate(files):
                paths.append(os.path.join(tmp, "%s_%05d.jpg" % (name, k)))
                with open(paths[-1], "wb") as f:
                    f.write(data)
            movie = os.path.join(tmp, name + ".avi")
            it = iter(files)
            with J.MjpegWriter(movie, 512, 384, channels=1, encoder=lambda fr: [next(it) for _ in range(len(fr))]) as w:
                for lo in range(0, N, 64):
                    w.add(frames[lo:lo + 64])
            reader = J.MjpegReader(movie)
            want = default_path(paths)
            ways = dict(read_jpeg_device=lambda: J.read_jpeg_device(paths),
                        decode_jpeg_device=lambda: J.decode_jpeg_device(files),
                        mjpeg_read_device=lambda: reader.read_device(),
                        default_pillow_16_threads=lambda: default_path(paths))
            if name == "pillow_no_restart_markers":
                for mode in ("interval", "sync"):
                    ways["read_jpeg_device[%s]" % mode] = lambda m=mode: J.read_jpeg_device(paths, entropy=m)
                    ways["decode_jpeg_device[%s]" % mode] = lambda m=mode: J.decode_jpeg_device(files, entropy=m)
                    ways["mjpeg_read_device[%s]" % mode] = lambda m=mode: reader.read_device(entropy=m)
            for fn in ways.values():                              # warm-up, and the pixels are the default path's
                assert torch.equal(fn(), want)
            times = {k: [] for k in ways}
            for _ in range(args.rounds):
                for k, fn in ways.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append(time.perf_counter() - t0)
            entropy_ms, pixels_ms = kernel_times(J, L, torch, files)
            result["sources"][name] = dict(
                bytes_per_file=int(np.mean([len(f) for f in files])),
                intervals_per_file=int(J.parse_jpeg(files[0]).bounds.shape[0]),
                files_per_s={k: round(N / float(np.median(v)), 1) for k, v in times.items()},
                seconds={k: [round(t, 4) for t in v] for k, v in times.items()},
                kernel_ms=dict(spnet_jpeg_entropy=round(entropy_ms, 3), spnet_jpeg_pixels=round(pixels_ms, 3)))
            if name == "pillow_no_restart_markers":
                result["sources"][name]["entropy_kernels_ms"] = sync_kernel_times(J, L, torch, files)

    def pillow_files(some, **options):
        out = []
        for f in some:
            b = io.BytesIO()
            Image.fromarray(f).save(b, "JPEG", quality=args.quality, **options)
            out.append(b.getvalue())
        return out

    # where the sync kernel overtakes the lane kernel: the same frames with a restart marker every r MCU rows
    result["crossover"] = {}
    for rows in (1, 2, 4, 8, 16, 24):
        result["crossover"]["restart_marker_rows_%d" % rows] = sync_kernel_times(
            J, L, torch, pillow_files(frames, restart_marker_rows=rows), segs=(32, 64, 128, 256))
    # colour: the first 128 frames as three different channels
    M = min(N, 128)
    rgb = np.stack([frames[:M], np.roll(frames[:M], 1, axis=0), frames[:M, ::-1]], axis=-1)
    result["colour_%d_files" % M] = {
        "444": sync_kernel_times(J, L, torch, pillow_files(rgb, subsampling=0)),
        "420": sync_kernel_times(J, L, torch, pillow_files(rgb, subsampling=2))}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
