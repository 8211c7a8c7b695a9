#! /usr/bin/env python3
"""Offline geometric augmentation of a directory of PNG + CSV pairs -- the surface of the reference's augment_preproc.py:
every image is flipped at random, rotated by up to +-20 degrees about its centre and (nine times out of ten) shifted by
up to +-40 px, n_augs times, and each result is written beside it as a new PNG + CSV with the reference's file-name
suffixes (_v | _h | _vh, _r{angle:.2f}, _t{xt},{yt}).  The pixels are warped in batches on the GPU (spnet_amd.augmentation.
DeviceWarper: the whole chain in one launch, bit-identical to flip_image -> rotate_image -> translate_image), the metadata
with the reference's arithmetic.

Differences from the reference, on purpose: the file lists are sorted; every (file, augmentation) pair draws from its own
RNG stream seeded by (seed, file index, augmentation index) -- the reference's forked workers all inherit ONE generator
state and so repeat each other's draws -- which makes a run reproducible whatever the batch size; band-pass mix-up
(bp_too) is not part of this tool.  train_spnet.py --warp does the same warps afresh every epoch without writing files.
"""
import glob
import os

import numpy as np
from PIL import Image

meta_extension = ".csv"


def caption_from_metadata(metadata):
    """metadata list-of-lists -> CSV text, one antinode per line (augment_preproc.py:41-53)."""
    return "\n".join("{0},{1},{2},{3},{4},{5}".format(*row) for row in metadata)


def _read_planes(filename):
    """PNG -> uint8 planes [C,H,W] (1 for L, 3 for RGB, 4 for RGBA); other modes are read as RGB."""
    with Image.open(filename) as im:
        if im.mode not in ("L", "RGB", "RGBA"):
            im = im.convert("RGB")
        a = np.asarray(im, dtype=np.uint8)
    return a[None] if a.ndim == 2 else np.ascontiguousarray(np.moveaxis(a, 2, 0))


class _DevicePlanes:
    """A file whose planes the GPU decodes when its batch is warped (--device_decode): what _read_planes would return for
    it has shape (channels, height, width)."""

    def __init__(self, filename, info):
        self.filename = filename
        self.shape = (info.channels, info.height, info.width)


def _planes_or_promise(filename):
    """_read_planes, or for a file the device decodes to the same planes (8 bits, L / RGB / RGBA) a _DevicePlanes."""
    from spnet_amd import png as P
    info = P.parse_png_file(filename)
    if info.device and info.channels in (1, 3, 4):
        return _DevicePlanes(filename, info)
    return _read_planes(filename)


def _planes_on_device(planes):
    """The batch's planes as one uint8 device tensor [P,H,W]: promised files are decoded on the GPU, one call per channel
    count (a file the kernels reject is decoded by Pillow there), the others uploaded."""
    import torch
    from spnet_amd import png as P
    total = sum(p.shape[0] for p in planes)
    X = torch.empty((total,) + tuple(planes[0].shape[1:]), dtype=torch.uint8, device="cuda")
    groups, p0 = {}, 0
    for p in planes:
        if isinstance(p, _DevicePlanes):
            groups.setdefault(p.shape[0], []).append((p0, p.filename))
        else:
            X[p0:p0 + p.shape[0]] = torch.from_numpy(p).cuda()
        p0 += p.shape[0]
    for c, members in groups.items():
        frames = P.read_png_device([f for _, f in members], channels="all", device=X.device)        # [n,H,W,c]
        idx = torch.tensor([q for q, _ in members], device=X.device)[:, None] + torch.arange(c, device=X.device)[None, :]
        X[idx] = frames.permute(0, 3, 1, 2)
    return X


def augment_data(path='Train', n_augs=39, seed=0, chunk=256, device_png=False, device_decode=False, device_png_lz=False):
    """Writes n_augs warped copies of every PNG + CSV pair of `path`; returns [(prefix, params)] of the files written,
    params = dict(flip, angle, xt, yt) with xt = yt = None where no shift was drawn.  chunk: planes warped per launch.
    device_png: the warped batch is encoded where DeviceWarper leaves it (spnet_amd.png) instead of copied out for Pillow:
    the same pixels and modes, other file bytes.  device_png_lz: the same (it implies device_png), with the encoder's LZ77
    stage on.
    device_decode: the originals are decoded on the GPU from the files' bytes (spnet_amd.png.read_png_device) into the
    tensor DeviceWarper warps, instead of by Pillow and uploaded: the same planes, the same files written."""
    import torch
    device_png = device_png or device_png_lz
    if device_png:
        from spnet_amd.png import write_png_device
    from spnet_amd import augmentation as A
    from spnet_amd import parallel, utils
    print("augment_data: Augmenting data in", path, 'by a factor of', n_augs + 1)
    path += '/'
    img_file_list = sorted(glob.glob(path + '*.png'))
    meta_file_list = sorted(glob.glob(path + '*' + meta_extension))
    assert len(img_file_list) == len(meta_file_list), \
        f"{len(img_file_list)} images, {len(meta_file_list)} CSV files. Should be the same number"
    numfiles = len(img_file_list)
    print("Found", numfiles, "files in", path)
    if not torch.cuda.is_available():
        raise RuntimeError("augment_preproc warps on the GPU (no CPU fallback)")
    written = []
    jobs, planes = [], []          # pending (file index, aug index, first plane, plane count), their source planes

    def flush():
        if not jobs:
            return
        X = _planes_on_device(planes) if device_decode else np.concatenate(planes)
        warper = A.DeviceWarper(X)
        index, draws = [], []
        for i, k, p0, c in jobs:
            np.random.seed(parallel.sample_seed(seed, k, i))
            d = A.draw_warp_gated()
            draws.append(d)
            index += list(range(p0, p0 + c))
        params = warper.new_params(index)
        j = 0
        for (i, k, p0, c), (flip, angle, xt, yt) in zip(jobs, draws):
            for _ in range(c):              # the planes of one image share its parameter set
                A.set_warp(params, j, flip, angle, xt or 0, yt or 0)
                j += 1
        out = torch.empty((len(index), warper.H, warper.W), dtype=torch.uint8, device=warper.X.device)
        warper.apply(params, out_u8=out)
        if not device_png:
            out = out.cpu().numpy()
        j = 0
        held = {}                  # device_png: plane count -> ([first plane of an image], [its file]), encoded in one batch
        for (i, k, p0, c), (flip, angle, xt, yt) in zip(jobs, draws):
            md, suffix = A.chain_metadata(utils.read_metadata(meta_file_list[i]), flip, angle, xt, yt, warper.W, warper.H)
            prefix = os.path.splitext(img_file_list[i])[0] + suffix
            with open(prefix + meta_extension, "w") as f:
                f.write(caption_from_metadata(md))
            if device_png:
                first, paths = held.setdefault(c, ([], []))
                first.append(j)
                paths.append(prefix + '.png')
            else:
                img = out[j] if c == 1 else np.moveaxis(out[j:j + c], 0, 2)
                Image.fromarray(np.ascontiguousarray(img)).save(prefix + '.png')     # 1 / 3 / 4 planes: L / RGB / RGBA, the input's mode
            j += c
            written.append((prefix, dict(flip=flip, angle=angle, xt=xt, yt=yt)))
        for c, (first, paths) in held.items():          # the warped planes stay in HBM; [n][c][H][W] -> [n][H][W][c]
            idx = torch.tensor(first, device=out.device)[:, None] + torch.arange(c, device=out.device)[None, :]
            frames = out[idx] if c > 1 else out[idx[:, 0]]
            write_png_device(frames.permute(0, 2, 3, 1).contiguous() if c > 1 else frames, paths, lz77=device_png_lz)
        jobs.clear()
        planes.clear()

    saved = np.random.get_state()
    try:
        shape, n_planes = None, 0
        for i in range(numfiles):
            if 0 == i % 10:
                print("     Progress: i =", i, "/", numfiles)
            pl = _planes_or_promise(img_file_list[i]) if device_decode else _read_planes(img_file_list[i])
            if shape is not None and tuple(pl.shape[1:]) != tuple(shape):
                flush()                      # a batch holds frames of one size
                n_planes = 0
            shape = pl.shape[1:]
            planes.append(pl)
            for k in range(n_augs):
                jobs.append((i, k, n_planes, pl.shape[0]))
            n_planes += pl.shape[0]
            if len(jobs) * pl.shape[0] >= chunk:
                flush()
                n_planes = 0
        flush()
    finally:
        np.random.set_state(saved)
    print("Augmented from", numfiles, "files up to", len(sorted(glob.glob(path + '*.png'))))
    return written


if __name__ == "__main__":
    import argparse
    parser = argparse.ArgumentParser(description="augments data in path",
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument('-d', '--datapath', help='dataset directory in which to augment', default="Train/")
    parser.add_argument('-n', '--naugs', type=int, help='number of augmentations per image to generate', default=42)
    parser.add_argument('--seed', type=int, help='seed of the per-(file, augmentation) random streams', default=0)
    parser.add_argument('--device_png', action='store_true',
                        help='(additive) encode the PNG files on the GPU (Huffman-only deflate): same pixels, other file bytes')
    parser.add_argument('--device_png_lz', action='store_true',
                        help="(additive) --device_png with the encoder's LZ77 stage: smaller files where pixels repeat")
    parser.add_argument('--device_decode', action='store_true',
                        help='(additive) decode the original PNG files on the GPU (inflate + unfilter): same planes, same output')
    args = parser.parse_args()
    augment_data(path=args.datapath, n_augs=args.naugs, seed=args.seed, device_png=args.device_png,
                 device_decode=args.device_decode, device_png_lz=args.device_png_lz)
