#! /usr/bin/env python3
"""Score a trained model on a labelled directory (mAP, count metrics, overlays) -- entry point and flags
of the reference's evaluate_spnet.py (:38-120), running on the MI355X engine."""
import argparse
import os
import time

import numpy as np

from spnet import diagnostics, models
from spnet.utils import build_dataset, denorm_Y, make_sure_path_exists, show_pred_ellipses
import spnet.config as cf


MASK_METRIC_LOG = "mask_metric.txt"


def mask_metric_report(Yp, Yt, log_dir, chunk=256, tol=5):
    """(additive, --mask_metric) The detector scored in pixels that carry a ring count: predicted and true grids are painted
    as ring-count masks on the device (spnet_amd.masks, one row per predictor, at the frames' own size), chunk by chunk, and
    compared pixel by pixel.  Prints the three ratios and the five counts and appends them to log_dir/mask_metric.txt."""
    from spnet.utils import orig_img_dims
    from spnet_amd import masks as MK
    W, H = int(orig_img_dims[0]), int(orig_img_dims[1])
    counts = np.zeros(5, np.int64)
    for lo in range(0, Yp.shape[0], chunk):
        pred = MK.masks_from_predictions(Yp[lo:lo + chunk], H, W)
        true = MK.masks_from_predictions(Yt[lo:lo + chunk], H, W)
        counts += MK.mask_counts_device(pred, true, tol).sum(0).cpu().numpy()
    res = MK.metrics_from_counts(*counts.tolist())
    lines = ["Mask metric (%d frames of %d x %d, ring tolerance %d/10):" % (Yp.shape[0], H, W, tol),
             "    pixel_acc = %s   object_iou = %s   ring_acc = %s" % (res["pixel_acc"], res["object_iou"], res["ring_acc"]),
             "    " + "   ".join("%s = %d" % (k, res[k]) for k in MK.COUNT_NAMES)]
    print("\n".join(lines))
    with open(log_dir + MASK_METRIC_LOG, "a") as f:
        f.write("\n".join(lines) + "\n")
    return res


def pred_mask_paths(file_list, pred_dir):
    """DIR/<same file name> for every frame of the data set."""
    return [os.path.join(pred_dir, os.path.basename(f)) for f in file_list]


def read_pred_masks(file_list, pred_dir, device_decode=False):
    """(additive, --pred_masks) The predicted ring-count masks of the data set's frames, uint8 [N,H,W].  A missing file is a
    FileNotFoundError that names it."""
    from spnet_amd import masks as MK
    return MK.read_masks(pred_mask_paths(file_list, pred_dir), device_decode=device_decode)


def predictions_from_masks(file_list, pred_dir, pred_grid, join_tol=0, min_pixels=1, device_decode=False, chunk=256):
    """(additive, --pred_masks) What model.predict returns, from mask files instead of a model: every mask is fitted to
    ellipse rows on the device (spnet_amd.masks.ellipses_from_masks_device) and the rows are encoded into the grid of Y_test
    by augmentation.encode_targets_device.  The grid holds target values (noobj 0 / 1), not logits."""
    import torch
    from spnet.augmentation import MAX_OBJECTS, encode_targets_device
    from spnet_amd import masks as MK
    out = []
    for lo in range(0, len(file_list), chunk):
        names = file_list[lo:lo + chunk]
        masks = read_pred_masks(names, pred_dir, device_decode)
        rows, count = MK.ellipses_from_masks_device(masks, join_tol=join_tol, min_pixels=min_pixels, overflow="truncate")
        many = torch.nonzero(count > MAX_OBJECTS).flatten().tolist()
        if many:
            raise ValueError("%s: %d objects of at least %d pixels, the grid codec takes %d (raise --mask_min_pixels?)"
                             % (pred_mask_paths(names, pred_dir)[many[0]], int(count[many[0]]), min_pixels, MAX_OBJECTS))
        Y, flags = encode_targets_device(rows[:, :MAX_OBJECTS].contiguous(), count, tuple(pred_grid))
        for j in torch.nonzero(flags).flatten().tolist():
            print("    %s: more objects in a grid cell than it has predictors; the first ones are kept"
                  % pred_mask_paths(names, pred_dir)[j])
        out.append(Y.cpu().numpy())
    return np.concatenate(out) if out else np.zeros((0, int(np.prod(pred_grid)) * cf.vars_per_pred), np.float32)


def evaluate_network(model=None, weights_file="", datapath="Test/", fraction=1.0, log_dir="", batch_size=32,
                     pred_grid=[6, 6, 2], set_means_ranges=True, device_png=False, device_decode=False,
                     device_overlay=False, device_png_lz=False, device_jpeg=False, jpeg_quality=90, movie=None,
                     movie_fps=5.0, mask_metric=False, pred_masks=None, mask_join_tol=0, mask_min_pixels=1):
    np.random.seed(1)
    print("Getting data..., fraction = ", fraction)
    X_test, Y_test, test_file_list, pred_shape = build_dataset(
        path=datapath, load_frac=fraction, set_means_ranges=set_means_ranges, batch_size=batch_size, shuffle=False,
        pred_grid=pred_grid, device_decode=device_decode)
    if model is None and pred_masks is None:
        print("Loading full model from full_model.h5")
        model = models.load_model("full_model.h5")

    m = X_test.shape[0]
    if pred_masks is not None:          # (additive) no model: the predictions are mask files, fitted to ellipses
        print("    Fitting ellipses to the masks in ", pred_masks, " (m = ", m, " frames)", sep="")
        start_time = time.time()
        Y_pred = predictions_from_masks(list(test_file_list[:m]), pred_masks, pred_grid, mask_join_tol, mask_min_pixels,
                                        device_decode)
        elapsed = time.time() - start_time
        print("    ...elapsed time to fit = ", elapsed, "s.   FPS = ", m * 1.0 / max(elapsed, 1e-9))
    else:
        print("    Predicting... (m = ", m, " frames in this (Test?) dataset)", sep="")
        start_time = time.time()
        # device_decode: uint8 device frames at the files' own size; every layout but 'big' resizes them on the device
        Y_pred = model.predict(X_test, batch_size=batch_size, resize=True) if device_decode and cf.model_type != 'big' else \
            model.predict(X_test, batch_size=batch_size)
        elapsed = time.time() - start_time
        print("    ...elapsed time to predict = ", elapsed, "s.   FPS = ", m * 1.0 / elapsed)

    if cf.loss_type != 'same' and pred_masks is None:
        Y_pred[:, cf.ind_noobj::cf.vars_per_pred] = 1.0 / (1.0 + np.exp(-Y_pred[:, cf.ind_noobj::cf.vars_per_pred]))
    Yt, Yp = denorm_Y(Y_test), denorm_Y(Y_pred)
    print("mAP = ", diagnostics.calc_map(Yp, Yt, device=True))      # 72 x N raster IoUs in one HIP launch

    (ring_miscounts, ring_truecounts, total_obj, false_obj_pos, false_obj_neg, true_obj_pos, true_obj_neg, pix_err,
     ipem) = diagnostics.calc_errors(Yp, Yt)
    mistakes = ring_miscounts + false_obj_pos + false_obj_neg
    tot = max(total_obj, 1)
    class_acc = (total_obj - mistakes) * 100.0 / tot
    print('Mean pixel error =', np.mean(pix_err))
    print("    Ring correct counts = ", ring_truecounts, ' / ', total_obj, '.   = ', 100 * ring_truecounts / tot,
          ' % ring-class accuracy', sep="")
    print("         Ring miscounts = ", ring_miscounts, ' / ', total_obj, '.   = ', 100 * ring_miscounts / tot, ' %', sep="")
    print("        False positives = ", false_obj_pos, ' / ', total_obj, '.   = ', 100 * false_obj_pos / tot, ' %', sep="")
    print("        False negatives = ", false_obj_neg, ' / ', total_obj, '.   = ', 100 * false_obj_neg / tot, ' %', sep="")
    print("         True positives = ", true_obj_pos, ' / ', total_obj, '.   = ', 100 * true_obj_pos / tot, ' %', sep="")
    print("         True negatives = ", true_obj_neg, sep="")
    print("    Total Mistakes = ", mistakes, ' / ', total_obj, '.   => ', class_acc,
          ' % class. accuracy rate (lack of mistakes)', sep="")

    make_sure_path_exists(log_dir)
    if mask_metric:
        mask_metric_report(Yp, Yt, log_dir)
    print("    Drawing sample ellipse images...")
    show_pred_ellipses(Yt, Yp, test_file_list, num_draw=m, log_dir=log_dir, out_csv=log_dir + 'hawley_spnet.csv',
                       png="device-jpeg" if device_jpeg else "device-lz" if device_png_lz else "device" if device_png
                       else "host",
                       jpeg_quality=jpeg_quality, movie=movie, movie_fps=movie_fps,
                       draw="device" if device_overlay else "host",
                       device_decode=bool(device_decode and device_overlay))
    return model


if __name__ == '__main__':
    p = argparse.ArgumentParser(description="tests network on test dataset",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-w', '--weights', default="weights.hdf5", help='weights file')
    p.add_argument('-d', '--datapath', default="Test/", help='Test dataset directory')
    p.add_argument('-f', '--fraction', type=float, default=1.0, help='Fraction of dataset to use')
    p.add_argument('-l', '--logdir', default='logs/Testing/', help='Directory to write log files into')
    p.add_argument('-b', '--batch_size', type=int, default=16, help='Batch size to use')
    p.add_argument('--model_type', default=None, help="override spnet.config.model_type ('monolithic' | 'big')")
    p.add_argument('--loss_type', default=None, help="override spnet.config.loss_type")
    p.add_argument('--device_decode', action='store_true',
                   help="(additive) upload the PNG files as they are and decode (and resize) them on the GPU; formats the "
                        "device does not take are decoded by Pillow: same predictions")
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
    p.add_argument('--mask_metric', action='store_true',
                   help="(additive) also score the predictions as ring-count segmentation masks, pixel by pixel on the GPU: "
                        "pixel_acc, object_iou, ring_acc and the five pixel counts, printed and appended to "
                        "<logdir>/" + MASK_METRIC_LOG)
    p.add_argument('--pred_masks', default=None, metavar='DIR',
                   help="(additive) score mask files instead of a model: DIR/<same file name> is read as the predicted "
                        "ring-count mask (value = 10 x rings) of every frame, fitted to ellipses on the GPU and scored by "
                        "the same mAP, count metrics, --mask_metric and overlays; no model is loaded")
    p.add_argument('--mask_join_tol', type=int, default=0,
                   help="--pred_masks: neighbouring pixels belong to one object if their values differ by at most this "
                        "(0: equal values only, what gen_fake_espi.py --masks paints; 255: anything above 0)")
    p.add_argument('--mask_min_pixels', type=int, default=1, help="--pred_masks: objects of fewer pixels are dropped")
    args = p.parse_args()
    if not 0 <= args.mask_join_tol <= 255:
        p.error("--mask_join_tol is 0 .. 255")
    if args.mask_min_pixels < 1:
        p.error("--mask_min_pixels is at least 1")
    if args.pred_masks is not None and not os.path.isdir(args.pred_masks):
        p.error("--pred_masks: no directory %s" % args.pred_masks)
    if args.device_jpeg and (args.device_png or args.device_png_lz):
        p.error("--device_jpeg writes .jpg files: not with --device_png / --device_png_lz")
    if not 1 <= args.jpeg_quality <= 100:
        p.error("--jpeg_quality is 1 .. 100")
    for attr, val in (("model_type", args.model_type), ("loss_type", args.loss_type)):
        if val is not None:
            setattr(cf, attr, val)
    model = evaluate_network(weights_file=args.weights, datapath=args.datapath + '/', fraction=args.fraction,
                             log_dir=args.logdir, batch_size=args.batch_size, device_png=args.device_png,
                             device_decode=args.device_decode, device_overlay=args.device_overlay,
                             device_png_lz=args.device_png_lz, device_jpeg=args.device_jpeg, jpeg_quality=args.jpeg_quality,
                             movie=args.movie, movie_fps=args.movie_fps, mask_metric=args.mask_metric,
                             pred_masks=args.pred_masks, mask_join_tol=args.mask_join_tol,
                             mask_min_pixels=args.mask_min_pixels)
    if model is not None:               # (--pred_masks: there is no model to save)
        weights2name = "eval_end_weights.hdf5"
        print("Saving model to", weights2name)
        model.save_weights(weights2name)
