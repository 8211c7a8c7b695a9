#! /usr/bin/env python3
"""Predict ellipses + ring counts for a directory of frames (no scoring) -- entry point and flags of the
reference's predict_spnet.py (:40-115), running on the MI355X engine."""
import argparse
import glob
import time

import numpy as np

from spnet.models import load_model, setup_model
from spnet.utils import (build_X, denorm_Y, make_sure_path_exists, nearest_multiple, setup_means_and_ranges,
                         show_pred_ellipses)
import spnet.config as cf

default_image_dir = '/home/shawley/datasets/zooniverse_steelpan/'


def predict_network(weights_file="spnet.model", datapath=default_image_dir, fraction=1.0, log_dir='logs/Predicting/',
                    batch_size=16, model=None, X_pred='', u8_frames=False, device_resize=False, device_png=False,
                    device_decode=False, device_overlay=False, device_png_lz=False, device_jpeg=False, jpeg_quality=90,
                    movie=None, movie_fps=5.0, movie_in=None, tracks=None, track_iou=0.25, track_gap=1, track_min_len=3,
                    track_truth=None, audio=None, notes=None, audio_fps=None, audio_offset=0, audio_window=2048, onset_frac=0.1,
                    note_radius=40):
    img_file_list = []
    resize = False
    frames = None
    if movie_in is not None:
        # (additive) the frames of a Motion-JPEG AVI, decoded on the GPU; they stay there up to the encoders
        import os
        from spnet_amd.jpeg import MjpegReader
        if cf.model_type == 'simple':
            raise ValueError("movie_in is for grayscale input (model_type 'big' / 'monolithic')")
        force_dim = None if cf.model_type == 'big' else 331
        reader = MjpegReader(movie_in)
        audio_fps = reader.fps if audio_fps is None else audio_fps      # (additive) the sound is read on the movie's own clock
        total_load = int(len(reader) * fraction)
        if batch_size is not None:
            total_load = nearest_multiple(total_load, batch_size)
        print(f"Getting data from {movie_in}: {len(reader)} frames of {reader.size[0]}x{reader.size[1]} at {reader.fps} "
              f"frames per second, going to load total_load = {total_load}")
        frames = reader.read_device(range(total_load), channels="all")
        frames = frames[..., 0] if int(frames.shape[3]) == 1 else frames        # [N,H,W] grey | [N,H,W,3]
        stem = os.path.splitext(os.path.basename(movie_in))[0]
        img_file_list = ["%s_%05d" % (stem, k) for k in range(total_load)]
        resize = force_dim is not None
        X_pred, _ = build_X(total_load, img_file_list, force_dim=force_dim, grayscale=True, as_uint8=True,
                            frames=frames if frames.dim() == 3 else frames[..., 0])
        device_decode = device_overlay = True
    elif isinstance(X_pred, str) and X_pred == '':
        print(f"Getting data from {datapath}, fraction = {fraction}.")
        if cf.model_type == 'simple':
            grayscale, force_dim = False, 224
        elif cf.model_type == 'big':
            grayscale, force_dim = True, None      # native 384x512 frames
        else:
            grayscale, force_dim = True, 331
        img_file_list = sorted(glob.glob(datapath + '/*.png')) or sorted(glob.glob(datapath + '/*.bmp'))
        if not img_file_list:       # (additive) a directory without PNG and BMP files: its JPEG files
            img_file_list = sorted(glob.glob(datapath + '/*.jpg') + glob.glob(datapath + '/*.jpeg'))
        total_files = len(img_file_list)
        total_load = int(total_files * fraction)
        if batch_size is not None:
            total_load = nearest_multiple(total_load, batch_size)
        print("      Total files = ", total_files, ", going to load total_load = ", total_load)
        # device_resize: the files' own grey levels travel, the GPU resizes them to force_dim (implies u8 frames; the
        # 'big' layout has nothing to resize)
        # device_decode: the files' bytes travel, the GPU decodes them -- PNG: inflate and unfilter, JPEG: Huffman, IDCT,
        # colour -- (implies device_resize)
        if device_decode and not grayscale:
            raise ValueError("device_decode is for grayscale input (model_type 'big' / 'monolithic')")
        resize = (bool(device_resize) or bool(device_decode)) and grayscale and force_dim is not None
        X_pred, _ = build_X(total_load, img_file_list, force_dim=force_dim, grayscale=grayscale,
                            as_uint8=(bool(u8_frames) or resize or bool(device_decode)) and grayscale, device_resize=resize,
                            device_decode=bool(device_decode))
        print("")

    if model is None:
        print("Loading model from", weights_file)
        if '.hdf5' in weights_file:
            print("   Defining model, then loading weights")
            X_shape = np.empty((1, force_dim, force_dim, 1), np.float32) if resize else X_pred
            model, _ = setup_model(X_shape, try_checkpoint=True, no_cp_fatal=True, weights_file=weights_file,
                                   parallel=False, freeze_fac=0.0, quick_setup=True)
        else:
            print("   Loading whole model")
            model = load_model(weights_file)

    m = X_pred.shape[0]
    print("    Predicting... (m = ", m, " frames in dataset)", sep="")
    start_time = time.time()
    Y_pred = model.predict(X_pred, batch_size=batch_size, resize=True) if resize else \
        model.predict(X_pred, batch_size=batch_size)
    elapsed = time.time() - start_time
    print("    ...elapsed time to predict = ", elapsed, "s.   FPS = ", m * 1.0 / elapsed)

    print("    Drawing ellipse images...")
    make_sure_path_exists(log_dir)
    setup_means_and_ranges([6, 6, 2, cf.vars_per_pred])
    if cf.loss_type != 'same':
        Y_pred[:, cf.ind_noobj::cf.vars_per_pred] = 1.0 / (1.0 + np.exp(-Y_pred[:, cf.ind_noobj::cf.vars_per_pred]))
    Yp = denorm_Y(Y_pred)
    if img_file_list:
        show_pred_ellipses(Yp, Yp, img_file_list, num_draw=m, log_dir=log_dir, out_csv=log_dir + 'hawley_spnet.csv',
                           show_true=False, png="device-jpeg" if device_jpeg else "device-lz" if device_png_lz else
                           "device" if device_png else "host", jpeg_quality=jpeg_quality, movie=movie, movie_fps=movie_fps,
                           draw="device" if device_overlay else "host", device_decode=bool(device_decode and device_overlay),
                           frames=frames)
    if tracks is not None and img_file_list:
        # (additive) link the predicted ellipses through time on the GPU: file order (-d, sorted) or frame order (movie_in)
        # is time order.  The grids go up once; the rows are formed, linked and ranked there (spnet_amd/tracks.py)
        import os
        from spnet_amd import tracks as TK
        from spnet.utils import orig_img_dims
        names = [os.path.basename(f) for f in img_file_list[:m]]
        rows, track, age = TK.tracks_from_predictions(Yp[:len(names)], orig_img_dims[1], orig_img_dims[0], iou=track_iou,
                                                      max_gap=track_gap)[:3]
        table, summary = TK.write_tracks(tracks, rows, track, age, names, min_len=track_min_len)
        print(f"    Tracks: {len(summary)} of at least {track_min_len} frames, {len(table)} detections -> {tracks}, "
              f"{TK.summary_path(tracks)}")
        if track_truth is not None:
            # (additive) score the tracks just linked against ground-truth identities (gen_fake_espi.py --strike writes
            # them): joined by file name, or by frame index for a movie; matched and counted on the GPU
            import torch
            truth = TK.read_truth_tracks(track_truth)
            if movie_in is not None:
                kept = [r for r in truth if r[0] < len(names)]
                rows_t, count_t, ident = TK.truth_arrays(kept, n_frames=len(names))
            else:       # the loader rounds the frames down to whole batches: truth of frames that were not loaded is left out
                known = set(names)
                kept = [r for r in truth if os.path.basename(r[1]) in known]
                rows_t, count_t, ident = TK.truth_arrays(truth, names=names, skip_unknown=True)
            if len(kept) < len(truth):
                print(f"    Track score: {len(truth) - len(kept)} truth rows belong to frames that were not predicted "
                      f"(the frames are rounded down to whole batches of {batch_size}) and are left out")
            dev = rows.device
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
            got = TK.score_tracks_device(up(rows_t), up(count_t), up(ident), rows, None, track, orig_img_dims[1],
                                         orig_img_dims[0], iou=track_iou)
            score = TK.track_score(*got, rows_t, rows, ident=ident, count_t=count_t)
            TK.write_track_score(TK.score_path(tracks), score, got[2])
            print(f"    Track score against {track_truth}: {score} -> {TK.score_path(tracks)}")
        if audio is not None:
            # (additive) the audio half: how loud every note of notes.csv is in the recording at the instant of each frame
            # (computed on the GPU: the recording goes up once, [frames][notes] integers come back), an onset per note by
            # the rule that gives a track's ring-count curve its onset, and the lag between the two per track
            from spnet_amd import audio as AU
            if notes is None or audio_fps is None:
                raise ValueError("predict_network: audio needs notes (a notes.csv) and audio_fps (frames per second)")
            pcm, rate = AU.read_wav(audio)
            note_rows = AU.read_notes(notes)
            env = AU.note_curves(pcm, rate, note_rows, len(names), audio_fps, offset=audio_offset, window=audio_window,
                                 device=rows.device)
            AU.write_envelopes(AU.envelopes_path(tracks), env, note_rows)
            lag = AU.audio_lag(table, note_rows, env, float(audio_fps), frac=onset_frac, radius=note_radius)
            AU.write_lag(AU.lag_path(tracks), lag)
            print(f"    Audio: {len(note_rows)} notes in {audio} ({pcm.size} samples at {rate} Hz, {audio_fps} frames per "
                  f"second), {sum(1 for r in lag if r[2] is not None)} with a track -> {AU.envelopes_path(tracks)}, "
                  f"{AU.lag_path(tracks)}")
    return model


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="predicts ellipses for a directory of images",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-w', '--weights', default="spnet.model", help='weights file (.hdf5) or whole-model file')
    p.add_argument('-d', '--datapath', default=default_image_dir, help='Dataset directory with list of images')
    p.add_argument('-f', '--fraction', type=float, default=1.0, help='Fraction of dataset to use')
    p.add_argument('-l', '--logdir', default='logs/Predicting/', help='Directory of log/output files')
    p.add_argument('-b', '--batch_size', type=int, default=16, help='Batch size to use')
    p.add_argument('--model_type', default=None, help="override spnet.config.model_type ('monolithic' | 'big')")
    p.add_argument('--loss_type', default=None, help="override spnet.config.loss_type")
    p.add_argument('--u8_frames', action='store_true',
                   help="(additive) keep the decoded frames as uint8 and scale them to [-1,1] on the GPU: same "
                        "predictions, a quarter of the host-to-device bytes")
    p.add_argument('--device_resize', action='store_true',
                   help="(additive, implies --u8_frames) load the frames at their own size and resize them to the "
                        "network's on the GPU, bit-identical to the PIL resize of the default path")
    p.add_argument('--device_decode', action='store_true',
                   help="(additive, implies --device_resize) upload the PNG / JPEG files as they are and decode them on the GPU "
                        "(formats the device does not take are decoded by Pillow): same predictions")
    p.add_argument('--movie_in', default=None, metavar='PATH.avi',
                   help="(additive, instead of -d; implies --device_decode and --device_overlay) predict on the frames of a "
                        "Motion-JPEG AVI, decoded on the GPU; they are named <stem>_NNNNN in the CSV and on the overlays")
    p.add_argument('--device_png', action='store_true',
                   help="(additive) encode the overlay PNG files on the GPU (Huffman-only deflate): the same pixels, "
                        "other file bytes")
    p.add_argument('--device_png_lz', action='store_true',
                   help="(additive) --device_png with the encoder's LZ77 stage: smaller overlay files")
    p.add_argument('--device_overlay', action='store_true',
                   help="(additive) draw the overlays (outlines, ring counts, file name) on the GPU: the same CSV and file "
                        "names, the same pixels away from outline edges; with --device_decode the frames are decoded there "
                        "too, with --device_png encoded there")
    p.add_argument('--device_jpeg', action='store_true',
                   help="(additive) write the overlays as steelpan_pred_NNNNN.jpg, baseline JPEG encoded on the GPU (lossy; "
                        "not with --device_png / --device_png_lz)")
    p.add_argument('--jpeg_quality', type=int, default=90, help="quality 1 .. 100 of --device_jpeg and --movie")
    p.add_argument('--movie', default=None, metavar='PATH',
                   help="(additive) also append every overlay, in order, to a Motion-JPEG AVI at PATH (encoded on the GPU)")
    p.add_argument('--movie_fps', type=float, default=5.0, help="frames per second of --movie")
    p.add_argument('--tracks', default=None, metavar='PATH.csv',
                   help="(additive) link the predicted ellipses from frame to frame on the GPU (sorted file order of -d, or "
                        "the frame order of --movie_in, is time order) and write one row per tracked detection to PATH.csv "
                        "and one row per track -- frames, length, mean and maximal ring count -- to PATH_summary.csv")
    p.add_argument('--track_iou', type=float, default=0.25,
                   help="least intersection over union of two ellipses' pixel sets for a link, applied in 1/1024 (a choice, "
                        "not a measurement)")
    p.add_argument('--track_gap', type=int, default=1,
                   help="link across up to this many frames, 1 .. 8: 2 bridges one missed detection (a choice, not a "
                        "measurement)")
    p.add_argument('--track_min_len', type=int, default=3,
                   help="leave tracks with fewer detections out of the two tables (a choice, not a measurement)")
    p.add_argument('--track_truth', default=None, metavar='TRUTH.csv',
                   help="(additive, with --tracks) score the linked tracks against the ground-truth identities of a "
                        "truth_tracks.csv (gen_fake_espi.py --strike): frames joined by file name, or by index with "
                        "--movie_in; prints the score and writes it to PATH_score.csv and PATH_score_idents.csv")
    p.add_argument('--audio', default=None, metavar='REC.wav',
                   help="(additive, with --tracks and --notes) a PCM16 sound recording of the same strike (first channel): the "
                        "envelope of every note at the instant of each frame, computed on the GPU, to PATH_envelopes.csv, and "
                        "per note its track, the onsets of its ring-count curve and of its envelope and their lag to PATH_lag.csv")
    p.add_argument('--notes', default=None, metavar='notes.csv',
                   help="(with --audio) the notes: name, freq_hz and the position cx, cy of the note on the pan in frame pixels")
    p.add_argument('--audio_fps', type=float, default=None,
                   help="video frames per second, the clock that places the frames in the recording; required with -d, the "
                        "movie's own rate with --movie_in")
    p.add_argument('--audio_offset', type=int, default=0, metavar='SAMPLES',
                   help="the sample of the recording at which frame 0 begins (may be negative)")
    p.add_argument('--audio_window', type=int, default=2048,
                   help="samples of the Hann window that starts at each frame's instant, 64 .. 8192: an onset is resolved no "
                        "finer than this (a choice, not a measurement)")
    p.add_argument('--onset_frac', type=float, default=0.1,
                   help="an onset is the first frame at which a curve reaches this fraction of its maximum, for the envelopes "
                        "and the ring counts alike (a choice, not a measurement)")
    p.add_argument('--note_radius', type=float, default=40,
                   help="a track belongs to the nearest note within this many pixels of its mean centre (a choice, not a "
                        "measurement)")
    args = p.parse_args(argv)
    if args.audio is not None and (args.tracks is None or args.notes is None):
        p.error("--audio compares a recording with the tracks of --tracks PATH.csv at the notes of --notes notes.csv: give all three")
    if args.audio is not None and args.movie_in is None and args.audio_fps is None:
        p.error("--audio with -d needs --audio_fps, the frames per second of the video")
    if args.audio is not None and not (64 <= args.audio_window <= 8192 and 0 <= args.onset_frac <= 1 and args.note_radius >= 0
                                       and (args.audio_fps is None or args.audio_fps > 0)):
        p.error("--audio_window is 64 .. 8192, --onset_frac 0 .. 1, --note_radius at least 0 and --audio_fps above 0")
    if args.track_truth is not None and args.tracks is None:
        p.error("--track_truth scores the tracks of --tracks PATH.csv: give both")
    if args.device_jpeg and (args.device_png or args.device_png_lz):
        p.error("--device_jpeg writes .jpg files: not with --device_png / --device_png_lz")
    if not 1 <= args.jpeg_quality <= 100:
        p.error("--jpeg_quality is 1 .. 100")
    if not 1 <= args.track_gap <= 8 or args.track_min_len < 1:
        p.error("--track_gap is 1 .. 8 and --track_min_len at least 1")
    return args


if __name__ == '__main__':
    np.random.seed(1)
    args = parse_args()
    for attr, val in (("model_type", args.model_type), ("loss_type", args.loss_type)):
        if val is not None:
            setattr(cf, attr, val)
    predict_network(weights_file=args.weights, datapath=args.datapath, fraction=args.fraction, log_dir=args.logdir,
                    batch_size=args.batch_size, u8_frames=args.u8_frames, device_resize=args.device_resize,
                    device_png=args.device_png, device_decode=args.device_decode, device_overlay=args.device_overlay,
                    device_png_lz=args.device_png_lz, device_jpeg=args.device_jpeg, jpeg_quality=args.jpeg_quality,
                    movie=args.movie, movie_fps=args.movie_fps, movie_in=args.movie_in, tracks=args.tracks,
                    track_iou=args.track_iou, track_gap=args.track_gap, track_min_len=args.track_min_len,
                    track_truth=args.track_truth, audio=args.audio, notes=args.notes, audio_fps=args.audio_fps,
                    audio_offset=args.audio_offset, audio_window=args.audio_window, onset_frac=args.onset_frac,
                    note_radius=args.note_radius)
