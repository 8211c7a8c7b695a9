#! /usr/bin/env python3
"""Band-pass mix-up throughput (csrc/bandpass.hip): N frames of H x W, uint8 in -> uint8 out, timed with HIP events.

Prints one JSON line: frames/s, ms per batch (median of --reps), and the fraction of the computed compute bound.  The
bound counts the algorithmic work of the windowed transform, 64 FLOP per pixel for the projection and 128 for the
reconstruction (192 FLOP per pixel), at the fp32 vector peak; the kernels execute more than that (the reconstruction
runs twice, once for the frame's min / max and once for the output, and the projection's column pass adds 32 FLOP per
pixel: 352 FLOP per pixel), reported as `executed_fraction`."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_VECTOR_PEAK = 157.3e12      # MI355X fp32 vector FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--H", type=int, default=384)
    ap.add_argument("--W", type=int, default=512)
    ap.add_argument("--reals", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    from spnet_amd.augmentation import BandpassPool
    rng = np.random.RandomState(0)
    real = torch.from_numpy(rng.randint(0, 256, (a.reals, a.H, a.W)).astype(np.uint8)).cuda()
    mixer = BandpassPool(real, a.H, a.W).mixer
    x = torch.from_numpy(rng.randint(0, 256, (a.n, a.H, a.W)).astype(np.uint8)).cuda()
    out = torch.empty_like(x)
    p = mixer.draw(a.n, seeds=list(range(a.n)))
    for _ in range(3):
        mixer.apply(p, x, out_u8=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        mixer.apply(p, x, out_u8=out)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    fps = a.n / (ms * 1e-3)
    px = a.H * a.W
    bound_fps = FP32_VECTOR_PEAK / (192.0 * px)
    print(json.dumps(dict(metric="bandpass_mixup_u8", n=a.n, H=a.H, W=a.W, ms=round(ms, 4), ms_min=round(min(times), 4),
                          frames_per_s=round(fps), bound_frames_per_s=round(bound_fps),
                          fraction_of_bound=round(fps / bound_fps, 4),
                          executed_fraction=round(fps * 352.0 * px / FP32_VECTOR_PEAK, 4))))


if __name__ == "__main__":
    main()
