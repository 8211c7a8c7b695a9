#!/usr/bin/env python3
"""Dev tool (GPU box): what reading PNG files costs through the default path and through the device decoder
(spnet_amd/png.py: read_png_device / decode_png_device).

The corpus is 512 fake-ESPI frames 384 x 512 (fake_espi.generate_device) in three forms:
  pillow    as Pillow writes them (gen_fake_espi.py's default writer)
  device    as the project's device encoder writes them (one literal-only dynamic block, filter 0)
  level1    zlib level 1 with the Sub filter on every row (what cv2.imwrite produces)
and three rates per form, files per second:
  build_X_upload     utils.build_X(..., as_uint8=True, device_resize=True) -- Pillow in build_X's own pool of forked
                     workers, 8 of them for 512 files -- followed by the upload of the frames.  Measured in a process
                     that has not touched the GPU while the files are decoded (as predict_spnet.py runs build_X); the
                     upload is timed after the rounds and its median is added to every round.
  pool16_upload      the same, with build_X's body run over 16 forked workers: the baseline of equal host parallelism
  read_png_device    files on disk -> uint8 device frames
  decode_png_device  bytes in memory -> uint8 device frames
One warm-up round, then `--repeats` rounds; wall time around work that ends with the frames in HBM and a synchronise;
median / min / max.  The decoded frames are compared with the default path's once.  Every step (writing the corpus, the
host baselines, each form on the device) is a process of its own under its own time limit.

usage: png_decode_time.py [--frames 512] [--repeats 5] [--tmp DIR] [--out profiles/png_decode_time.json]"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
from PIL import Image

from spnet_amd.codec_host import MAX_THREADS as THREADS
FORMS = ("pillow", "device", "level1")


def rates(n, times):
    t = sorted(times)
    return {"files_per_s": n / t[len(t) // 2], "min_files_per_s": n / t[-1], "max_files_per_s": n / t[0],
            "ms_per_file": 1e3 * t[len(t) // 2] / n, "rounds": len(t)}


def pool16_load(files):
    """build_X's own body (utils.build_X: _load_one over a forked pool, imap in chunks of 32) with 16 workers: build_X
    itself takes min(cpu_count, N // 64) = 8 for 512 files."""
    import multiprocessing
    from functools import partial
    from spnet_amd import utils as U
    worker = partial(U._load_one, None, True, as_uint8=True)
    X = np.zeros((len(files),) + U._load_one(None, True, files[0], True).shape, np.uint8)
    pool = multiprocessing.get_context("fork").Pool(THREADS)
    try:
        for i, arr in enumerate(pool.imap(worker, files, chunksize=32)):
            X[i] = arr
    finally:
        pool.close()
        pool.join()
    return X


def step_host(root, repeats):
    """(a), in a process that does not touch the GPU while the files are decoded (as predict_spnet.py runs build_X):
    prints one JSON line {form: {...}}."""
    from spnet_amd import utils as U
    res, frames = {}, {}
    for form in FORMS:
        files = sorted(glob.glob(os.path.join(root, form, "*.png")))
        ways = (("build_X_s", lambda: U.build_X(len(files), files, force_dim=331, grayscale=True, as_uint8=True,
                                                device_resize=True)[0]),
                ("pool16_s", lambda: pool16_load(files)))
        times = {k: [] for k, _ in ways}
        for rnd in range(repeats + 1):
            for name, fn in ways:
                t0 = time.perf_counter()
                X = fn()
                dt = time.perf_counter() - t0
                if rnd:
                    times[name].append(dt)
        frames[form] = X
        res[form] = {k: sorted(v) for k, v in times.items()}
        res[form]["build_X_workers"] = min(os.cpu_count() or 1, max(1, len(files) // 64))
    import torch
    for form in FORMS:
        up = []
        for rnd in range(repeats + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            d = torch.from_numpy(frames[form]).cuda()
            torch.cuda.synchronize()
            if rnd:
                up.append(time.perf_counter() - t0)
            del d
        res[form]["upload_s"] = sorted(up)
    print("STEP_RESULT " + json.dumps(res), flush=True)


def write_corpus(root, U):
    from spnet_amd import png as P
    host = U.cpu().numpy()
    n = len(host)
    paths = {form: [os.path.join(root, form, "f%05d.png" % i) for i in range(n)] for form in FORMS}
    for form in FORMS:
        os.makedirs(os.path.join(root, form))

    def level1(i):
        a = host[i]
        sub = a.copy()
        sub[:, 1:] = a[:, 1:] - a[:, :-1]
        stream = np.concatenate([np.ones((a.shape[0], 1), np.uint8), sub], axis=1).tobytes()
        with open(paths["level1"][i], "wb") as f:
            f.write(P.png_container(zlib.compress(stream, 1), a.shape[1], a.shape[0], 1))

    with ThreadPoolExecutor(max_workers=THREADS) as pool:
        list(pool.map(lambda i: Image.fromarray(host[i]).save(paths["pillow"][i]), range(n)))
        list(pool.map(level1, range(n)))
    for lo in range(0, n, 256):
        P.write_png_device(U[lo:lo + 256], paths["device"][lo:lo + 256], threads=THREADS)


def step_corpus(root, n):
    import torch
    from spnet_amd import fake_espi as F
    _, _, U = F.generate_device(n, seed=1, want_u8=True)
    write_corpus(root, U)
    np.save(os.path.join(root, "frames.npy"), U.cpu().numpy())
    print("STEP_RESULT " + json.dumps({"device": torch.cuda.get_device_name(0)}), flush=True)


def step_device(root, form, repeats):
    import torch
    from spnet_amd import png as P
    paths = sorted(glob.glob(os.path.join(root, form, "*.png")))
    host = np.load(os.path.join(root, "frames.npy"))
    n = len(paths)
    datas = [open(p, "rb").read() for p in paths]
    out, status, fallback = P.read_png_device(paths, threads=THREADS, return_info=True)
    assert fallback == [] and np.array_equal(out.cpu().numpy(), host), form          # the same frames, no fallback
    ways = (("read_png_device", lambda: P.read_png_device(paths, threads=THREADS)),
            ("decode_png_device", lambda: P.decode_png_device(datas, threads=THREADS)))
    times = {k: [] for k, _ in ways}
    for rnd in range(repeats + 1):
        for name, fn in ways:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    r = {"file_bytes": sum(len(d) for d in datas), "pixel_bytes": int(host.nbytes)}
    for name, _ in ways:
        r[name] = rates(n, times[name])
    print("STEP_RESULT " + json.dumps(r), flush=True)


def run_step(args, limit):
    """One step as a process of its own, under its own time limit; a step that fails ends the tool."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=limit,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, "step %s failed (%d)\n%s\n%s" % (args, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("STEP_RESULT ")][0][len("STEP_RESULT "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default="profiles/png_decode_time.json")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--form", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step == "corpus":
        return step_corpus(args.tmp, args.frames)
    if args.step == "host":
        return step_host(args.tmp, args.repeats)
    if args.step == "device":
        return step_device(args.tmp, args.form, args.repeats)
    root = args.tmp or tempfile.mkdtemp(prefix="png_decode_time_")
    common = ["--tmp", root, "--frames", str(args.frames), "--repeats", str(args.repeats)]
    n = args.frames
    res = {"threads": THREADS, "pillow_version": Image.__version__, "cpus_usable": len(os.sched_getaffinity(0)),
           "frames": n, "forms": {}}
    res["gpu"] = run_step(["--step", "corpus"] + common, 300)["device"]
    a = run_step(["--step", "host"] + common, 900)
    for form in FORMS:
        r = run_step(["--step", "device", "--form", form] + common, 300)
        up = a[form]["upload_s"][len(a[form]["upload_s"]) // 2]
        r["build_X_upload"] = dict(rates(n, [t + up for t in a[form]["build_X_s"]]), workers=a[form]["build_X_workers"],
                                   upload_ms=1e3 * up)
        r["pool16_upload"] = dict(rates(n, [t + up for t in a[form]["pool16_s"]]), workers=THREADS, upload_ms=1e3 * up)
        r["read_over_pool16"] = r["read_png_device"]["files_per_s"] / r["pool16_upload"]["files_per_s"]
        res["forms"][form] = r
        print(form + ":", json.dumps(r), flush=True)
    if args.tmp is None:
        shutil.rmtree(root, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
