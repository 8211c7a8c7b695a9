#! /usr/bin/env python3
"""Generate a synthetic 'fake-ESPI' data set -- entry point and flags of the reference's gen_fake_espi.py, running on the
MI355X: the frames are drawn and rasterised in HBM (spnet_amd.fake_espi.generate_device) and written as
steelpan_NNNNNNN.png + steelpan_NNNNNNN.csv pairs, the layout utils.build_dataset reads.

  -d / --datapath   directory under which Train/ (and with -a, Val/) are written
  -n / --numframes  number of frames
  -a / --all        the first 80 % of the frame numbers go to Train/, the rest to Val/ (the reference deals its ten tasks
                    the same way: tasks 0-7 Train, 8-9 Val); default: Train/ only

Additive flags: --seed; --count_range LO HI (antinodes per frame; 0 6 is the published Dataset A, see fake_espi.draw_params);
--bp_real DIR --bp_path DIR (also the band-pass mixed copies, steelpan_NNNNNNN_bp.png + .csv, as a data set of their own
under bp_path, as fake_espi.write_dataset writes them); --host_params (the parameters of the reference-ordered host stream,
fake_espi.draw_params, instead of the device sampler's own stream: the same distributions, other frames); --device_png (the
PNGs are encoded from HBM by spnet_amd.png instead of copied out for Pillow: the same pixels, other file bytes).

The PNGs are encoded (by default) and written by at most 16 threads of this process; nothing is forked once the GPU is
initialised."""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

TRAIN_FRACTION = 0.8


def _write_csv(stem, rows):
    from spnet_amd.fake_espi import rows_to_csv
    with open(stem + ".csv", "w") as f:
        f.write(rows_to_csv(rows))


def _write_pair(stem, frame, rows):
    Image.fromarray(frame).save(stem + ".png")
    _write_csv(stem, rows)


def split_dirs(n, everything):
    """Subdirectory of every frame number 0 .. n-1."""
    n_train = int(n * TRAIN_FRACTION) if everything else n
    return ["Train" if i < n_train else "Val" for i in range(n)]


def gen_dataset(datapath=".", numframes=500, everything=False, seed=0, count_range=(1, 7), bp_real=None, bp_path=None,
                host_params=False, chunk=256, device="cuda:0", threads=None, device_png=False, device_png_lz=False):
    """Writes the data set; returns the label rows of every frame, in frame order.  device_png: the frames are encoded where
    they are (spnet_amd.png.write_png_device) and only the compressed bytes cross to the host.  device_png_lz: the same (it
    implies device_png), with the encoder's LZ77 stage on."""
    import torch
    from spnet_amd import fake_espi as F
    if (bp_real is None) != (bp_path is None):
        raise ValueError("gen_fake_espi: --bp_real and --bp_path go together")
    if not torch.cuda.is_available():
        raise RuntimeError("gen_fake_espi: the frames are generated on the GPU (no CPU fallback)")
    device_png = device_png or device_png_lz
    n = int(numframes)
    sub = split_dirs(n, everything)
    for root in (datapath,) + ((bp_path,) if bp_path else ()):
        for d in sorted(set(sub)):
            os.makedirs(os.path.join(root, d), exist_ok=True)
    threads = threads or min(16, os.cpu_count() or 1)
    mixer = None
    if bp_real is not None:
        from spnet_amd.augmentation import BandpassPool
        mixer = BandpassPool.get(bp_real, F.IM_H, F.IM_W, torch.device(device)).mixer
    U_host = labels_host = None
    if host_params:         # that stream is keyed by (n, seed): one call for the whole set
        _, labels_host, U_host = F.generate_device(n, seed, device, want_u8=True, chunk=chunk, count_range=count_range)
    labels = []

    def submit(pool, root, suffix, frames_dev, rows, lo, hi):
        stems = [os.path.join(root, sub[i], "steelpan_" + str(i).zfill(7) + suffix) for i in range(lo, hi)]
        if device_png:
            from spnet_amd.png import write_png_device
            write_png_device(frames_dev, [st + ".png" for st in stems], pool=pool, lz77=device_png_lz)
            return [pool.submit(_write_csv, st, r) for st, r in zip(stems, rows)]
        frames = frames_dev.cpu().numpy()
        return [pool.submit(_write_pair, st, frames[k], rows[k]) for k, st in enumerate(stems)]

    with ThreadPoolExecutor(max_workers=threads) as pool:
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            if host_params:
                U, rows = U_host[lo:hi], labels_host[lo:hi]
            else:
                _, rows, U = F.generate_device(hi - lo, seed, device, want_u8=True, chunk=chunk, count_range=count_range,
                                               params="device", first_frame=lo)
            jobs = submit(pool, datapath, "", U, rows, lo, hi)
            if mixer is not None:
                bp = mixer.draw(hi - lo, seeds=F.bandpass_seeds(hi - lo, seed, lo))
                mixed = U.clone()
                mixer.apply(bp, mixed, out_u8=mixed)
                jobs += submit(pool, bp_path, "_bp", mixed, rows, lo, hi)
            for j in jobs:
                j.result()
            labels += rows
            print("   wrote frames %d .. %d of %d" % (lo, hi - 1, n), flush=True)
    return labels


if __name__ == "__main__":
    p = argparse.ArgumentParser(description="generates fake-ESPI frames and their annotations",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-d', '--datapath', default=".", help='Directory to write images to (in Train/ and maybe Val/ subdirs)')
    p.add_argument('-n', '--numframes', type=int, default=500, help='Number of images to generate')
    p.add_argument('-a', '--all', action='store_true', help='generate Train and Val data; default is Train only')
    p.add_argument('--seed', type=int, default=0, help='seed of the parameter stream and the sensor noise')
    p.add_argument('--count_range', type=int, nargs=2, default=(1, 7), metavar=('LO', 'HI'),
                   help='antinodes drawn per frame, inclusive (0 6: the published Dataset A)')
    p.add_argument('--bp_real', default=None, help='directory of real 512x384 *.png frames: also write band-pass mixed copies')
    p.add_argument('--bp_path', default=None, help='directory for the band-pass mixed copies (a data set of its own)')
    p.add_argument('--host_params', action='store_true',
                   help="draw the parameters on the host in the reference's RNG order instead of on the device")
    p.add_argument('--device_png', action='store_true',
                   help="(additive) encode the PNG files on the GPU (Huffman-only deflate): the same pixels, other file bytes")
    p.add_argument('--device_png_lz', action='store_true',
                   help="(additive) --device_png with the encoder's LZ77 stage: smaller files where pixels repeat")
    args = p.parse_args()
    gen_dataset(datapath=args.datapath, numframes=args.numframes, everything=args.all, seed=args.seed,
                count_range=tuple(args.count_range), bp_real=args.bp_real, bp_path=args.bp_path, host_params=args.host_params,
                device_png=args.device_png, device_png_lz=args.device_png_lz)
