#!/usr/bin/env python3
"""Dev tool (GPU box): what writing the frames as JPEG on the GPU costs (spnet_amd/jpeg.py) beside Pillow's JPEG writer and the
device PNG writer, in the manner of tools/png_time.py.

The same frames four ways -- 512 fake-ESPI frames 384 x 512 from fake_espi.generate_device, and 256 RGB overlays of them:
  pillow_jpeg_16_threads   the frames copied to the host, Image.save(path, "JPEG", qtables=the same tables, subsampling=0) on
                           16 threads
  write_png_device         spnet_amd.png.write_png_device (--device_png), 256 frames per call
  write_jpeg_device        spnet_amd.jpeg.write_jpeg_device (--device_jpeg), 256 frames per call
  movie                    MjpegWriter.add, 256 frames per call, one AVI
One warm-up round, then `--repeats` rounds in which the four alternate in this one process; wall time around work that ends
in files written; median / min / max frames per second and the bytes written.  Also the two kernels alone (events,
back-to-back launches).

usage: jpeg_time.py [--frames 512] [--overlays 256] [--repeats 5] [--quality 90] [--tmp DIR] [--out profiles/jpeg_time.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from PIL import Image

from tools.png_time import draw_overlays
from tools.resize_time import gpu_time

CHUNK = 256
from spnet_amd.codec_host import MAX_THREADS as THREADS


def four_ways(dev, tmp, repeats, quality):
    import torch
    from spnet_amd import jpeg as J
    from spnet_amd import png as P
    n, H, W = (int(v) for v in dev.shape[:3])
    channels = 1 if dev.dim() == 3 else int(dev.shape[3])
    qt = J.quant_tables(quality)
    tables = [[int(v) for v in qt[t]] for t in range(1 if channels == 1 else 2)]
    jpg = [os.path.join(tmp, "f%05d.jpg" % i) for i in range(n)]
    png = [os.path.join(tmp, "f%05d.png" % i) for i in range(n)]

    def pillow():
        host = dev.cpu().numpy()
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            list(pool.map(lambda i: Image.fromarray(host[i]).save(jpg[i], "JPEG", qtables=tables, subsampling=0), range(n)))
        return sum(os.path.getsize(p) for p in jpg)

    def device_png():
        return sum(sum(P.write_png_device(dev[lo:lo + CHUNK], png[lo:lo + CHUNK], threads=THREADS)) for lo in range(0, n, CHUNK))

    def device_jpeg():
        return sum(sum(J.write_jpeg_device(dev[lo:lo + CHUNK], jpg[lo:lo + CHUNK], quality=quality, threads=THREADS))
                   for lo in range(0, n, CHUNK))

    def movie():
        path = os.path.join(tmp, "movie.avi")
        with J.MjpegWriter(path, W, H, channels=channels, quality=quality) as w:
            for lo in range(0, n, CHUNK):
                w.add(dev[lo:lo + CHUNK])
        return os.path.getsize(path)

    ways = (("pillow_jpeg_16_threads", pillow), ("write_png_device", device_png), ("write_jpeg_device", device_jpeg),
            ("movie", movie))
    times = {k: [] for k, _ in ways}
    size = {}
    for rnd in range(repeats + 1):                   # round 0 warms up: code objects, allocator, page cache of tmp
        for name, fn in ways:
            os.makedirs(tmp, exist_ok=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            size[name] = fn()
            dt = time.perf_counter() - t0
            shutil.rmtree(tmp)
            if rnd:
                times[name].append(dt)
    res = {"frames": n}
    for name, _ in ways:
        t = sorted(times[name])
        res[name] = {"frames_per_s": n / t[len(t) // 2], "min_frames_per_s": n / t[-1], "max_frames_per_s": n / t[0],
                     "ms_per_frame": 1e3 * t[len(t) // 2] / n, "bytes": size[name], "rounds": len(t)}
    res["device_jpeg_over_pillow_jpeg_files_per_s"] = (res["write_jpeg_device"]["frames_per_s"]
                                                       / res["pillow_jpeg_16_threads"]["frames_per_s"])
    res["device_jpeg_over_pillow_jpeg_bytes"] = size["write_jpeg_device"] / size["pillow_jpeg_16_threads"]
    res["device_jpeg_over_device_png_bytes"] = size["write_jpeg_device"] / size["write_png_device"]
    return res


def kernels_alone(dev, quality):
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import jpeg as J
    n, H, W = (int(v) for v in dev.shape[:3])
    ch = 1 if dev.dim() == 3 else int(dev.shape[3])
    sizes, sizes_dev = J.interval_sizes(dev, quality)
    offsets = J.scan_offsets(sizes)
    out = J.pack_frames(dev, sizes_dev, offsets, quality)
    off = torch.from_numpy(offsets).cuda()
    qt = J._device_tables(quality, dev.device)
    st = L.current_stream()
    k_scan = gpu_time(lambda i: L.spnet_jpeg_scan(dev.data_ptr(), n, H, W, ch, qt.data_ptr(), sizes_dev.data_ptr(), st), 1,
                      window_ms=100.0)
    k_pack = gpu_time(lambda i: L.spnet_jpeg_pack(dev.data_ptr(), n, H, W, ch, qt.data_ptr(), sizes_dev.data_ptr(),
                                                  off.data_ptr(), out.data_ptr(), int(out.numel()), st), 1, window_ms=100.0)
    for k in (k_scan, k_pack):
        k["us_per_frame"] = k["us"] / n
    return {"frames": n, "spnet_jpeg_scan": k_scan, "spnet_jpeg_pack": k_pack, "scan_bytes": int(offsets[-1]),
            "pixel_bytes": int(dev.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--overlays", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a fresh temporary directory)")
    ap.add_argument("--out", default="profiles/jpeg_time.json")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "jpeg_time.py measures on the GPU"
    from spnet_amd import fake_espi as F
    root = args.tmp or tempfile.mkdtemp(prefix="jpeg_time_")
    tmp = os.path.join(root, "files")
    res = {"device": torch.cuda.get_device_name(0), "threads": THREADS, "chunk": CHUNK, "quality": args.quality,
           "pillow": Image.__version__, "cpus_usable": len(os.sched_getaffinity(0))}

    _, labels, U = F.generate_device(args.frames, seed=1, want_u8=True)
    res["grey_384x512"] = four_ways(U, tmp, args.repeats, args.quality)
    res["grey_384x512"]["kernels"] = kernels_alone(U[:CHUNK], args.quality)
    print("grey:", json.dumps(res["grey_384x512"]), flush=True)

    m = min(args.overlays, args.frames)
    O = torch.from_numpy(draw_overlays(U[:m].cpu().numpy(), labels[:m])).cuda()
    res["rgb_overlay_384x512"] = four_ways(O, tmp, args.repeats, args.quality)
    res["rgb_overlay_384x512"]["kernels"] = kernels_alone(O[:CHUNK], args.quality)
    print("rgb overlays:", json.dumps(res["rgb_overlay_384x512"]), flush=True)

    if args.tmp is None:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
