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
PNGs are encoded from HBM by spnet_amd.png instead of copied out for Pillow: the same pixels, other file bytes); --masks
(beside every X/steelpan_NNNNNNN.png a ring-count segmentation mask X/masks/steelpan_NNNNNNN.png, spnet_amd.masks: painted on
the device from the parameter arrays the frames were rasterised from, or from the label rows with --host_params; the
loaders glob X/*.png only and do not see the sub-directory).  Without a GPU the script stops, as before; only --masks
then still runs, on the host generator's frames (fake_espi.generate, the reference-ordered stream) and the host mask rule,
and says so.  --strike S --strike_frames T [--strike_jitter J] [--movie]: instead of a data set, S movies of T frames with
known tracks (gen_strike below), for predict_spnet.py --tracks --track_truth.  --audio [--audio_rate R] [--audio_fps F]
[--audio_lag FRAMES] [--audio_noise LSB] (with --strike): also the strike's SOUND with known onsets -- strike_NNNN.wav,
strike_NNNN/notes.csv and strike_NNNN/truth_audio.csv -- for predict_spnet.py --tracks --audio --notes.

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
                host_params=False, chunk=256, device="cuda:0", threads=None, device_png=False, device_png_lz=False,
                masks=False):
    """Writes the data set; returns the label rows of every frame, in frame order.  device_png: the frames are encoded where
    they are (spnet_amd.png.write_png_device) and only the compressed bytes cross to the host.  device_png_lz: the same (it
    implies device_png), with the encoder's LZ77 stage on.  masks: also X/masks/steelpan_NNNNNNN.png, the frame's ring-count
    mask (spnet_amd.masks), written by the same writer as the frames."""
    import torch
    from spnet_amd import fake_espi as F
    if (bp_real is None) != (bp_path is None):
        raise ValueError("gen_fake_espi: --bp_real and --bp_path go together")
    device_png = device_png or device_png_lz
    n = int(numframes)
    sub = split_dirs(n, everything)
    if not torch.cuda.is_available():
        if not masks:
            raise RuntimeError("gen_fake_espi: the frames are generated on the GPU (no CPU fallback)")
        return _gen_dataset_host(datapath, n, sub, seed, tuple(count_range), bp_real, device_png)
    for root in (datapath,) + ((bp_path,) if bp_path else ()):
        for d in sorted(set(sub)):
            os.makedirs(os.path.join(root, d), exist_ok=True)
            if masks and root == datapath:
                os.makedirs(os.path.join(root, d, "masks"), exist_ok=True)
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

    def submit_masks(pool, mask_dev, lo, hi):
        from spnet_amd.masks import write_masks
        paths = [os.path.join(datapath, sub[i], "masks", "steelpan_" + str(i).zfill(7) + ".png") for i in range(lo, hi)]
        if device_png:
            write_masks(mask_dev, paths, png="device-lz" if device_png_lz else "device", pool=pool)
            return []
        host = mask_dev.cpu().numpy()
        return [pool.submit(write_masks, host[k:k + 1], [p]) for k, p in enumerate(paths)]

    with ThreadPoolExecutor(max_workers=threads) as pool:
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            mask_dev = None
            if host_params:
                U, rows = U_host[lo:hi], labels_host[lo:hi]
                if masks:
                    from spnet_amd.masks import ring_masks_device
                    mask_dev = ring_masks_device(rows, H=F.IM_H, W=F.IM_W, device=device)
            elif masks:     # the label rows stay in HBM for the rasteriser; the CSV rows are read back from them
                from spnet_amd.masks import ring_masks_device
                _, (rows_d, count_d), U = F.generate_device(hi - lo, seed, device, want_u8=True, chunk=chunk,
                                                            count_range=count_range, params="device", first_frame=lo,
                                                            labels="device")
                mask_dev = ring_masks_device(rows_d, count_d, H=F.IM_H, W=F.IM_W)
                packed = torch.cat([rows_d.reshape(hi - lo, -1), count_d.double()[:, None]], 1).cpu().numpy()
                rows = [[tuple(r) for r in fr.reshape(-1, 6)[:int(k)].astype(np.int64).tolist()]
                        for fr, k in zip(packed[:, :-1], packed[:, -1])]
            else:
                _, rows, U = F.generate_device(hi - lo, seed, device, want_u8=True, chunk=chunk, count_range=count_range,
                                               params="device", first_frame=lo)
            jobs = submit(pool, datapath, "", U, rows, lo, hi)
            if mask_dev is not None:
                jobs += submit_masks(pool, mask_dev, lo, hi)
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


def gen_strike(datapath=".", sequences=1, frames=64, jitter=0, seed=0, count_range=(1, 7), device="cuda:0", threads=None,
               device_png=False, device_png_lz=False, movie=False, movie_fps=5.0, audio=False, audio_rate=48000, audio_fps=200.0,
               audio_lag=4, audio_noise=8):
    """Strike movies with known tracks (spnet_amd.fake_espi.generate_strike_device): for sequence s the directory
    datapath/strike_NNNN with steelpan_NNNNNNN.png + .csv per frame in time order -- the loaders' own format -- and
    truth_tracks.csv (spnet_amd.tracks.write_truth_tracks: `track` is the identity, `age` the frames since it first
    appeared); movie: also datapath/strike_NNNN.avi, the frames as a grey Motion-JPEG movie encoded on the GPU.  Returns per
    sequence the truth table.  audio: also the sequence's sound (fake_espi.strike_audio_host, host numpy: every antinode is a
    note that becomes audible audio_lag frames after its rings appear, the struck one at once) as datapath/strike_NNNN.wav,
    PCM16 at audio_rate with audio_fps movie frames a second; strike_NNNN/notes.csv (name, freq_hz and the antinode's frame-0
    centre cx, cy); strike_NNNN/truth_audio.csv (ident, name, freq_hz, video_onset, audio_onset at audio.DEFAULT_ONSET_FRAC)."""
    import torch
    from spnet_amd import fake_espi as F
    from spnet_amd import tracks as TK
    if not torch.cuda.is_available():
        raise RuntimeError("gen_fake_espi: the frames are generated on the GPU (no CPU fallback)")
    device_png = device_png or device_png_lz
    S, T = int(sequences), int(frames)
    threads = threads or min(16, os.cpu_count() or 1)
    tables = []
    with ThreadPoolExecutor(max_workers=threads) as pool:
        for s in range(S):
            root = os.path.join(datapath, "strike_" + str(s).zfill(4))
            os.makedirs(root, exist_ok=True)
            _, (rows_d, count_d), ident_d, U = F.generate_strike_device(1, T, seed, jitter, first_sequence=s,
                                                                        count_range=count_range, device=device, want_u8=True)
            rows, count, ident = rows_d.cpu().numpy(), count_d.cpu().numpy(), ident_d.cpu().numpy()
            labels = [[tuple(r) for r in rows[t, :count[t]].astype(np.int64).tolist()] for t in range(T)]
            stems = [os.path.join(root, "steelpan_" + str(t).zfill(7)) for t in range(T)]
            if device_png:
                from spnet_amd.png import write_png_device
                write_png_device(U, [st + ".png" for st in stems], pool=pool, lz77=device_png_lz)
                jobs = [pool.submit(_write_csv, st, r) for st, r in zip(stems, labels)]
            else:
                host = U.cpu().numpy()
                jobs = [pool.submit(_write_pair, st, host[t], labels[t]) for t, st in enumerate(stems)]
            for j in jobs:
                j.result()
            tables.append(TK.write_truth_tracks(os.path.join(root, "truth_tracks.csv"), rows, ident,
                                                [os.path.basename(st) + ".png" for st in stems]))
            if audio:
                from spnet_amd import audio as AU
                _, n0, c0 = (a.cpu().numpy() for a in F.draw_params_device(1, seed, device, count_range, first_frame=s))
                pcm, info = F.strike_audio_host(n0, c0, T, seed, first_sequence=s, rate=audio_rate, fps=audio_fps,
                                                lag=audio_lag, noise=audio_noise)
                AU.write_wav(root + ".wav", pcm[0], audio_rate)
                AU.write_notes(os.path.join(root, "notes.csv"),
                               [(info["name"][0][j], float(info["freq"][0, j]), float(n0[0, j, 0]), float(n0[0, j, 1]))
                                for j in np.flatnonzero(info["valid"][0])])
                TK._write_csv(os.path.join(root, "truth_audio.csv"), F.TRUTH_AUDIO_FIELDS,
                              F.strike_audio_truth(info, 0, T, first_sequence=s))
            if movie:
                from spnet_amd.jpeg import MjpegWriter
                with MjpegWriter(root + ".avi", F.IM_W, F.IM_H, fps=movie_fps, channels=1) as w:
                    w.add(U)
            print("   wrote sequence %d of %d: %d frames, %d identities -> %s" % (s, S, T, len({r[2] for r in tables[-1]}), root),
                  flush=True)
    return tables


def _gen_dataset_host(datapath, n, sub, seed, count_range, bp_real, device_png):
    """gen_dataset(masks=True) on a machine without a GPU: the host generator's frames (fake_espi.generate: the
    reference-ordered parameter stream, Pillow's rasteriser -- other pixels than the device's) and the host mask rule."""
    from spnet_amd import fake_espi as F
    from spnet_amd.masks import ring_masks_host, write_masks
    if bp_real is not None or device_png or count_range != (1, 7):
        raise RuntimeError("gen_fake_espi: no GPU -- the band-pass copies, the device PNG encoder and --count_range need one")
    print("gen_fake_espi: no GPU -- frames from the host generator (fake_espi.generate), masks by the host rule", flush=True)
    X, labels = F.generate(n, seed)
    for i in range(n):
        d = os.path.join(datapath, sub[i])
        os.makedirs(os.path.join(d, "masks"), exist_ok=True)
        name = "steelpan_" + str(i).zfill(7)
        _write_pair(os.path.join(d, name), X[i], labels[i])
        write_masks(ring_masks_host([labels[i]], H=F.IM_H, W=F.IM_W), [os.path.join(d, "masks", name + ".png")])
    return labels


def main(argv=None):
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
    p.add_argument('--masks', action='store_true',
                   help="(additive) also write X/masks/steelpan_NNNNNNN.png, the frame's ring-count segmentation mask: "
                        "trunc(10 * rings) inside every ellipse, 0 outside")
    p.add_argument('--strike', type=int, default=None, metavar='S',
                   help="(additive, instead of -n / -a) write S strike movies with known tracks: DIR/strike_NNNN/ with the "
                        "frames in time order and truth_tracks.csv -- the struck note rings at once, the sympathetic notes "
                        "ramp up after an onset of their own")
    p.add_argument('--strike_frames', type=int, default=64, metavar='T', help="frames of a strike movie, 1 .. 4096")
    p.add_argument('--strike_jitter', type=int, default=0, metavar='J',
                   help="the centres move by up to J whole pixels from frame to frame, 0 .. 8")
    p.add_argument('--movie', action='store_true', help="(with --strike) also DIR/strike_NNNN.avi, Motion-JPEG encoded on the GPU")
    p.add_argument('--audio', action='store_true',
                   help="(with --strike) also the strike's sound with known onsets: DIR/strike_NNNN.wav (PCM16, one channel), "
                        "DIR/strike_NNNN/notes.csv and DIR/strike_NNNN/truth_audio.csv; every antinode is a note that becomes "
                        "audible --audio_lag frames after its rings appear, the struck one at once")
    p.add_argument('--audio_rate', type=int, default=48000, help="samples per second of --audio, at least 16000")
    p.add_argument('--audio_fps', type=float, default=200.0, help="movie frames per second that --audio is synchronous with")
    p.add_argument('--audio_lag', type=int, default=4, metavar='FRAMES',
                   help="frames by which a sympathetic note's sound follows its rings, 0 .. 64 (put in by construction: it shows "
                        "what the lag analysis recovers, nothing about a drum)")
    p.add_argument('--audio_noise', type=int, default=8, metavar='LSB', help="uniform noise of +- this many LSB on --audio, 0 .. 1024")
    args = p.parse_args(argv)
    if args.audio and args.strike is None:
        p.error("--audio goes with --strike")
    if args.audio and not (args.audio_rate >= 16000 and args.audio_fps > 0 and 0 <= args.audio_lag <= 64
                           and 0 <= args.audio_noise <= 1024):
        p.error("--audio_rate is at least 16000, --audio_fps above 0, --audio_lag 0 .. 64 and --audio_noise 0 .. 1024")
    if args.strike is not None:
        if args.strike < 0 or not 1 <= args.strike_frames <= 4096 or not 0 <= args.strike_jitter <= 8:
            p.error("--strike is at least 0, --strike_frames 1 .. 4096 and --strike_jitter 0 .. 8")
        if args.bp_real or args.bp_path or args.host_params or args.masks or args.all:
            p.error("--strike combines with --seed, --count_range, --device_png, --device_png_lz, --movie and --audio only")
        return gen_strike(args.datapath, args.strike, args.strike_frames, args.strike_jitter, args.seed, tuple(args.count_range),
                          device_png=args.device_png, device_png_lz=args.device_png_lz, movie=args.movie, audio=args.audio,
                          audio_rate=args.audio_rate, audio_fps=args.audio_fps, audio_lag=args.audio_lag, audio_noise=args.audio_noise)
    if args.movie:
        p.error("--movie goes with --strike")
    gen_dataset(datapath=args.datapath, numframes=args.numframes, everything=args.all, seed=args.seed,
                count_range=tuple(args.count_range), bp_real=args.bp_real, bp_path=args.bp_path, host_params=args.host_params,
                device_png=args.device_png, device_png_lz=args.device_png_lz, masks=args.masks)


if __name__ == "__main__":
    main()
