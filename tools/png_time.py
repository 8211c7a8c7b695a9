#!/usr/bin/env python3
"""Dev tool (GPU box): what writing PNG files costs through Pillow and through the device encoder (spnet_amd/png.py).

The same frames three ways -- 512 fake-ESPI frames 384 x 512 from fake_espi.generate_device, and 256 RGB overlays of them
drawn as utils.show_pred_ellipses draws them:
  pillow_16_threads   the frames copied to the host, Image.fromarray(frame).save(path) on 16 threads: the default writers
  write_png_device    spnet_amd.png.write_png_device, 256 frames per call (files on disk)
  encode_png_device   spnet_amd.png.encode_png_device, 256 frames per call (bytes in memory, no files)
One warm-up round, then `--repeats` rounds in which the three alternate; wall time around work that ends in files written or
bytes on the host; median / min / max frames per second.  Also: the two kernels alone (events, back-to-back launches), the
ratio of the device files' size to Pillow's on the same frames, and that ratio on noise-free canvases (no LZ77 stage: the
known limit).

--lz77 adds the encoder's LZ77 stage as two more ways in the same rounds (write_png_device_lz77, encode_png_device_lz77:
the same calls with lz77=True), its two kernels alone, the host plan and how many frames took the LZ stream, and writes
profiles/png_lz_time.json: Pillow, the literal-only encoder and the LZ stage side by side, one run.

usage: png_time.py [--frames 512] [--overlays 256] [--repeats 5] [--tmp DIR] [--lz77] [--out profiles/png_time.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
from PIL import Image

from tools.resize_time import gpu_time

CHUNK = 256
from spnet_amd.codec_host import MAX_THREADS as THREADS


def draw_overlays(frames, labels):
    """uint8 [n,H,W,3]: every frame as RGB with its labelled ellipses and ring counts drawn on it."""
    from PIL import ImageDraw
    from spnet_amd import config as cf
    from spnet_amd import utils
    out = []
    for frame, rows in zip(frames, labels):
        img = Image.fromarray(frame).convert("RGB")
        d = ImageDraw.Draw(img)
        for cx, cy, a, b, angle, rings in rows:
            utils.draw_ellipse(img, [cx, cy], [a, b], angle, color=cf.predcolor, thickness=3)
            d.text((cx - 10, cy + 6), "{: >3.1f}".format(float(rings)), fill=tuple(cf.predcolor[::-1]))
        d.text((5, frame.shape[0] - 14), "steelpan_0000000.png", fill=(255, 255, 255))
        out.append(np.asarray(img, dtype=np.uint8))
    return np.stack(out)


def three_ways(dev, tmp, repeats, lz77=False):
    """dev: uint8 device frames.  Frames per second of the three writers and the bytes they wrote."""
    import torch
    from spnet_amd import png as P
    n = int(dev.shape[0])
    paths = [os.path.join(tmp, "f%05d.png" % i) for i in range(n)]

    def pillow():
        host = dev.cpu().numpy()
        with ThreadPoolExecutor(max_workers=THREADS) as pool:
            list(pool.map(lambda i: Image.fromarray(host[i]).save(paths[i]), range(n)))
        return sum(os.path.getsize(p) for p in paths)

    def write_device():
        return sum(sum(P.write_png_device(dev[lo:lo + CHUNK], paths[lo:lo + CHUNK], threads=THREADS)) for lo in range(0, n, CHUNK))

    def encode_device():
        return sum(sum(len(b) for b in P.encode_png_device(dev[lo:lo + CHUNK], threads=THREADS)) for lo in range(0, n, CHUNK))

    def write_device_lz():
        return sum(sum(P.write_png_device(dev[lo:lo + CHUNK], paths[lo:lo + CHUNK], threads=THREADS, lz77=True))
                   for lo in range(0, n, CHUNK))

    def encode_device_lz():
        return sum(sum(len(b) for b in P.encode_png_device(dev[lo:lo + CHUNK], threads=THREADS, lz77=True))
                   for lo in range(0, n, CHUNK))

    ways = (("pillow_16_threads", pillow), ("write_png_device", write_device), ("encode_png_device", encode_device))
    if lz77:
        ways += (("write_png_device_lz77", write_device_lz), ("encode_png_device_lz77", encode_device_lz))
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
    res = {}
    for name, _ in ways:
        t = sorted(times[name])
        res[name] = {"frames_per_s": n / t[len(t) // 2], "min_frames_per_s": n / t[-1], "max_frames_per_s": n / t[0],
                     "ms_per_frame": 1e3 * t[len(t) // 2] / n, "bytes": size[name], "rounds": len(t)}
    res["frames"] = n
    res["device_over_pillow_bytes"] = size["write_png_device"] / size["pillow_16_threads"]
    if lz77:
        res["lz77_over_pillow_bytes"] = size["write_png_device_lz77"] / size["pillow_16_threads"]
        res["lz77_over_device_bytes"] = size["write_png_device_lz77"] / size["write_png_device"]
        res["lz77_over_pillow_files_per_s"] = res["write_png_device_lz77"]["frames_per_s"] / res["pillow_16_threads"]["frames_per_s"]
        res["lz77_over_device_files_per_s"] = res["write_png_device_lz77"]["frames_per_s"] / res["write_png_device"]["frames_per_s"]
    return res


def kernels_alone(dev):
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import png as P
    n, H, W = (int(v) for v in dev.shape[:3])
    ch = 1 if dev.dim() == 3 else int(dev.shape[3])
    hist, adler = P.frame_statistics(dev)
    plan = P.plan_frames(hist)
    hist_d = torch.empty((n, 256), dtype=torch.int32, device=dev.device)
    st = L.current_stream()
    k_hist = gpu_time(lambda i: L.spnet_png_hist(dev.data_ptr(), n, H, W, ch, hist_d.data_ptr(), adler.data_ptr(), st), 1,
                      window_ms=100.0)
    out = P.pack_frames(dev, plan, adler)
    # the same call again and again into the same buffer: OR-ing identical bits, the same traffic
    blob = torch.from_numpy(np.concatenate([plan["offsets"].view(np.uint8), plan["codes"].reshape(-1).view(np.uint8),
                                            plan["header"].reshape(-1).view(np.uint8), plan["header_bits"].view(np.uint8)])).cuda()
    p = blob.data_ptr()
    pc = p + 8 * (n + 1)
    ph = pc + 4 * P.NSYM * n
    pb = ph + 4 * P.HEADER_WORDS * n
    k_pack = gpu_time(lambda i: L.spnet_png_pack(dev.data_ptr(), n, H, W, ch, pc, ph, pb, p, adler.data_ptr(), out.data_ptr(),
                                                 int(out.numel()), st), 1, window_ms=100.0)
    t0 = time.perf_counter()
    P.plan_frames(hist)
    t_plan = time.perf_counter() - t0
    for k in (k_hist, k_pack):
        k["us_per_frame"] = k["us"] / n
    return {"frames": n, "spnet_png_hist": k_hist, "spnet_png_pack": k_pack, "plan_frames_host_ms_per_frame": 1e3 * t_plan / n,
            "compressed_bytes": int(plan["offsets"][-1]), "pixel_bytes": int(dev.numel())}


def kernels_alone_lz(dev):
    """The LZ stage's two kernels (events, back-to-back launches), its host plan and the choice it made."""
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import png as P
    n, H, W = (int(v) for v in dev.shape[:3])
    ch = 1 if dev.dim() == 3 else int(dev.shape[3])
    hist, adler = P.frame_statistics(dev)
    lhist, dhist = P.lz_statistics(dev)
    t0 = time.perf_counter()
    plan = P.plan_frames_lz(hist, lhist, dhist)
    t_plan = time.perf_counter() - t0
    both = torch.empty((n * (P.NLL + P.NDIST),), dtype=torch.int32, device=dev.device)
    st = L.current_stream()
    k_scan = gpu_time(lambda i: L.spnet_png_lz_scan(dev.data_ptr(), n, H, W, ch, both.data_ptr(), both.data_ptr() + 4 * P.NLL * n,
                                                    st), 1, window_ms=100.0)
    out = P.pack_frames_lz(dev, plan, adler)
    parts = [plan["offsets"].astype(np.int64), plan["lcodes"], plan["dcodes"], plan["lz_header"], plan["lz_header_bits"]]
    blob = torch.from_numpy(np.concatenate([np.ascontiguousarray(v).reshape(-1).view(np.uint8) for v in parts])).cuda()
    at = [int(v) for v in np.cumsum([0] + [v.nbytes for v in parts[:-1]]) + blob.data_ptr()]
    # the same call again and again into the same buffer (OR-ing identical bits); frames that stayed literal-only are skipped
    k_pack = gpu_time(lambda i: L.spnet_png_lz_pack(dev.data_ptr(), n, H, W, ch, at[1], at[2], at[3], at[4], at[0], adler.data_ptr(),
                                                    out.data_ptr(), int(out.numel()), st), 1, window_ms=100.0)
    for k in (k_scan, k_pack):
        k["us_per_frame"] = k["us"] / n
    return {"frames": n, "frames_that_took_lz": int(plan["use_lz"].sum()), "spnet_png_lz_scan": k_scan,
            "spnet_png_lz_pack": k_pack, "plan_frames_lz_host_ms_per_frame": 1e3 * t_plan / n,
            "compressed_bytes": int(plan["offsets"][-1]), "lz_bytes_if_always": int(plan["lz_sizes"].sum()),
            "literal_bytes_if_always": int(plan["literal_sizes"].sum()), "pixel_bytes": int(dev.numel())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--overlays", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: a fresh temporary directory)")
    ap.add_argument("--lz77", action="store_true", help="also time the encoder's LZ77 stage (default --out: png_lz_time.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = "profiles/png_lz_time.json" if args.lz77 else "profiles/png_time.json"
    import torch
    assert torch.cuda.is_available(), "png_time.py measures on the GPU"
    from spnet_amd import fake_espi as F
    root = args.tmp or tempfile.mkdtemp(prefix="png_time_")
    tmp = os.path.join(root, "files")
    res = {"device": torch.cuda.get_device_name(0), "threads": THREADS, "chunk": CHUNK, "pillow": Image.__version__,
           "cpus_usable": len(os.sched_getaffinity(0))}

    _, labels, U = F.generate_device(args.frames, seed=1, want_u8=True)
    res["grey_384x512"] = three_ways(U, tmp, args.repeats, args.lz77)
    res["grey_384x512"]["kernels"] = kernels_alone(U[:CHUNK])
    if args.lz77:
        res["grey_384x512"]["kernels_lz77"] = kernels_alone_lz(U[:CHUNK])
    print("grey:", json.dumps(res["grey_384x512"]), flush=True)

    m = min(args.overlays, args.frames)
    O = torch.from_numpy(draw_overlays(U[:m].cpu().numpy(), labels[:m])).cuda()
    res["rgb_overlay_384x512"] = three_ways(O, tmp, args.repeats, args.lz77)
    res["rgb_overlay_384x512"]["kernels"] = kernels_alone(O[:CHUNK])
    if args.lz77:
        res["rgb_overlay_384x512"]["kernels_lz77"] = kernels_alone_lz(O[:CHUNK])
    print("rgb overlays:", json.dumps(res["rgb_overlay_384x512"]), flush=True)

    _, _, C = F.generate_device(64, seed=1, noise=False, want_u8=True)
    res["noise_free_canvas_384x512"] = three_ways(C, tmp, 1, args.lz77)
    if args.lz77:
        res["noise_free_canvas_384x512"]["kernels_lz77"] = kernels_alone_lz(C)
    print("noise-free canvases:", json.dumps(res["noise_free_canvas_384x512"]), flush=True)

    if args.tmp is None:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
