#! /usr/bin/env python3
"""Train SPNet on a directory with Train/ and Val/ (PNG + same-stem CSV) -- entry point and flags of the
reference's train_spnet.py, running on the MI355X engine.

Additive flags (not in the reference): --model_type / --loss_type / --backbone override the
spnet.config globals; multi-GPU = launch with `python -m torch.distributed.run --nproc-per-node N`;
--fake_stream N trains on N fresh synthetic frames per epoch generated on the GPU (no Train/ or Val/ directory).
"""
import argparse
import os
import random
import shutil
import sys
import time

import numpy as np

from spnet import callbacks, models, multi_gpu, utils  # noqa: F401
import spnet.config as cf
from evaluate_spnet import evaluate_network
from predict_spnet import default_image_dir, predict_network


VAL_STREAM_TOP = 2 ** 40      # the validation frames of --fake_stream are the LAST M global frame indices below this


def fake_stream_data(n_train, n_val, global_batch, pred_grid, seed, warp=False):
    """--fake_stream: (X_train, Y_train, X_val, Y_val, FreshFakeESPI callback, pred_shape).  The training set is n_train
    (rounded down to a multiple of the global batch) fresh frames per epoch: epoch e = the global frames e*n .. e*n + n - 1
    of the device parameter stream.  The validation set, n_val frames (default n_train // 4), is generated once from the
    frame indices VAL_STREAM_TOP - n_val .. VAL_STREAM_TOP - 1: the top of the index space this script uses, which training
    would reach only after 2^40 / n frames' worth of epochs.  The layout follows cf.model_type: 331 x 331 frames, or the
    native 384 x 512 for 'big'.  X_train / Y_train are the callback's device tensors (fit() reads them in place).
    warp (--warp): the callback also keeps each epoch's full-size frames and label rows on the device in its .warper, the
    warp_source of AugmentOnTheFly."""
    from spnet_amd import fake_espi
    n = utils.nearest_multiple(int(n_train), global_batch)
    if n < 1:
        raise ValueError("--fake_stream %d is less than one global batch (%d)" % (n_train, global_batch))
    m = int(n_train) // 4 if n_val is None else int(n_val)
    if m < 1:
        raise ValueError("--fake_val: the validation set is empty")
    if cf.model_type == 'simple':
        raise ValueError("--fake_stream generates one-channel frames (model_type 'monolithic' | 'big' | 'compound')")
    size = None if cf.model_type == 'big' else 331
    device = str(multi_gpu.parallel.local_device())
    pred_shape = np.array([pred_grid[0], pred_grid[1], pred_grid[2], cf.vars_per_pred], dtype=int)
    print("Fresh fake-ESPI frames: %d per epoch, %d validation frames (global frames %d .. %d), frame size %s"
          % (n, m, VAL_STREAM_TOP - m, VAL_STREAM_TOP - 1, "384x512" if size is None else "331x331"))
    val = fake_espi.FakeStream(m, seed=seed, device=device, size=size, pred_grid=pred_grid)
    Xv, labels = val.frames(VAL_STREAM_TOP - m, m)
    Yv, _ = fake_espi.targets_from_labels(labels, pred_grid)
    fresh = callbacks.FreshFakeESPI(None, None, fake_espi.FakeStream(n, seed=seed, device=device, size=size,
                                                                     pred_grid=pred_grid), warper=bool(warp))
    return fresh.X, fresh.Y, Xv.cpu().numpy(), Yv, fresh, pred_shape


def train_network(weights_file="weights.hdf5", datapath=".", fraction=1.0, batch_size=32, epochs=30, pred_grid=[6, 6, 2],
                  noaugment=False, log_dir=".", lr_max=4e-5, freeze_fac=0.7, frozen_epochs=4, random_seed=1,
                  augment_blur=False, bp_real=None, bpmix_prob=0.3, warp=False, fake_stream=None, fake_val=None,
                  device_decode=False, device_aug_params=False):
    np.random.seed(random_seed)
    if device_decode and (noaugment or not ((warp and not fake_stream) or bp_real)):
        raise ValueError("--device_decode decodes the files of --warp (on a data set on disk) and of --bp_real on the GPU: "
                         "it needs one of them, and not --noaugment")
    # Data parallel (launched by torch.distributed.run): choose this rank's GPU and join the process group before
    # anything touches the device; rank 0 alone logs, validates and writes checkpoints.
    rank, _, world = multi_gpu.parallel.init_distributed()
    print("pred_grid = ", pred_grid)
    fresh = None
    if fake_stream:
        X_train, Y_train, X_val, Y_val, fresh, pred_shape = fake_stream_data(fake_stream, fake_val, batch_size * world,
                                                                             pred_grid, random_seed, warp and not noaugment)
        train_file_list, val_file_list = None, None          # no files: MyProgressCallback draws no overlays
    else:
        X_train, Y_train, train_file_list, pred_shape = utils.build_dataset(
            path=datapath + "/Train/", load_frac=fraction, set_means_ranges=True, batch_size=batch_size, pred_grid=pred_grid)
        X_val, Y_val, val_file_list, pred_shape = utils.build_dataset(
            path=datapath + "/Val/", load_frac=1.0, set_means_ranges=False, batch_size=batch_size, pred_grid=pred_grid)

    print("Seting up NN model.  model_type = ", cf.model_type)
    parallel = world > 1
    model, serial_model = models.setup_model(X_train, int(Y_train[0].size), no_cp_fatal=False, weights_file=weights_file,
                                             parallel=parallel, freeze_fac=freeze_fac)

    callback_list = []
    if rank == 0:           # logging / validation / checkpoints: one writer
        callback_list += [
            callbacks.MyProgressCallback(X_val=X_val, Y_val=Y_val, val_file_list=val_file_list, log_dir=log_dir,
                                         pred_shape=pred_shape),
            callbacks.ParallelCheckpointCallback(model, filepath=weights_file, save_every=5, dir=log_dir)]
    # one optimizer iteration consumes batch_size frames on EVERY rank
    callback_list.append(callbacks.OneCycleScheduler(lr_max=lr_max, n_data_points=X_train.shape[0], epochs=epochs,
                                                     batch_size=batch_size * world, verbose=int(rank == 0)))
    if fresh is not None:       # ahead of AugmentOnTheFly: the fresh frames are what it augments
        callback_list.append(fresh)
    if not noaugment:
        print("Adding callback for augment on the fly")
        if warp and fresh is not None:      # streamed frames: warped from the device tensors the stream keeps
            warp_args = dict(warp_source=fresh.warper, warp_targets="device", device_decode=bool(device_decode))
        else:
            warp_args = dict(warp=warp, warp_files=list(train_file_list[:X_train.shape[0]]) if warp else None,
                             device_decode=bool(device_decode))
        callback_list.append(callbacks.AugmentOnTheFly(X_train, Y_train, aug_every=1, seed=random_seed,
                                                       real_blur=augment_blur, bandpass_real=bp_real,
                                                       bpmix_prob=bpmix_prob, pred_grid=pred_grid,
                                                       params="device" if device_aug_params else "host", **warp_args))

    fit_args = dict(batch_size=batch_size, shuffle=True, verbose=1, validation_data=(X_val, Y_val), callbacks=callback_list)
    if frozen_epochs > 0 and freeze_fac > 0.0:        # warm-up phase with the first layers frozen
        model.fit(X_train, Y_train, epochs=frozen_epochs, **fit_args)
    if freeze_fac > 0.0:
        model = models.unfreeze_model(model, X_train, Y_train, parallel=parallel)
    model.fit(X_train, Y_train, epochs=epochs - frozen_epochs, **fit_args)
    if os.environ.get("SPNET_DUMP_WEIGHT_SUM"):       # test hook: one checksum of the trained weights per rank
        import hashlib
        h = hashlib.sha256()
        for k, v in model.state_dict().items():
            if "moving_" not in k:           # BatchNorm statistics are per replica (tower semantics), weights are not
                h.update(v.numpy().tobytes())
        with open("%s.%d" % (os.environ["SPNET_DUMP_WEIGHT_SUM"], rank), "w") as f:
            f.write(h.hexdigest())
    return model


if __name__ == '__main__':
    seed = 1
    np.random.seed(seed)
    random.seed(seed)
    p = argparse.ArgumentParser(description="trains network on training dataset",
                                formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument('-b', '--batch_size', type=int, default=16, help='Batch size to use')
    p.add_argument('-d', '--datapath', default="./", help='Directory with images in Train/ and Val/ subdirs')
    p.add_argument('-e', '--epochs', type=int, default=100, help='Number of epochs to run')
    p.add_argument('-f', '--fraction', type=float, default=1.0, help='Fraction of dataset to use')
    p.add_argument('--freeze_fac', type=float, default=0.0, help='Fraction of base model to freeze')
    p.add_argument('--frozen_epochs', type=int, default=0, help='Starting epochs to run while base model is frozen')
    p.add_argument('-g', '--grid', default="6x6x2", help='Shape of predictor grid')
    p.add_argument('-w', '--weights', default="weights.hdf5", help='Weights file')
    p.add_argument('-l', '--lrmax', type=float, default=4e-5, help='Maximum learning rate value')
    p.add_argument('-n', '--noaugment', action='store_true', help="don't augment on the fly")
    p.add_argument('--name', default='', help='Descriptive name of the run, prepended to the log directory name')
    p.add_argument('-r', '--random_seed', type=int, default=1, help="Random seed value")
    p.add_argument('--model_type', default=None, help="override spnet.config.model_type ('monolithic' | 'big')")
    p.add_argument('--loss_type', default=None, help="override spnet.config.loss_type ('same' | 'hybrid')")
    p.add_argument('--backbone', default=None, help="override spnet.config.basemodel")
    p.add_argument('--augment_blur', action='store_true',
                   help="apply the Gaussian blur of the on-the-fly augmentation (the reference computes and discards it)")
    p.add_argument('--bp_real', default=None,
                   help="directory of real ESPI *.png frames (the training frames' size): band-pass mix-up on the fly")
    p.add_argument('--bpmix_prob', type=float, default=0.3, help="probability of the band-pass mix-up per frame")
    p.add_argument('--warp', action='store_true',
                   help="warp every training frame afresh each epoch (random flip, rotation of +-20 degrees, shift of up to "
                        "+-40 px: what augment_preproc.py writes offline) and recompute its targets.  NEEDS the PNG + CSV "
                        "files of Train/ on disk: the frames are warped at their full size and the targets come from the "
                        "CSV rows -- or --fake_stream, whose full-size frames and label rows stay on the GPU.  Ignored "
                        "with --noaugment")
    p.add_argument('--device_decode', action='store_true',
                   help="(additive; needs --warp on a data set on disk, or --bp_real) decode the full-size frames of the warp "
                        "and the grey real frames of --bp_real on the GPU from the PNG files' bytes instead of with "
                        "Pillow: the same frames")
    p.add_argument('--device_aug_params', action='store_true',
                   help="(additive) draw the random parameters of the on-the-fly augmentation -- and, with --fake_stream "
                        "--warp, of the warp -- on the GPU, one launch per chunk, from a keyed stream of its own (the same "
                        "distributions, other values than the reference's RNG order; a sample's draws depend on the seed, "
                        "the epoch and the sample only).  Not with --warp on a data set on disk")
    p.add_argument('--fake_stream', type=int, default=None, metavar='N',
                   help="train on N fresh fake-ESPI frames per epoch, generated on the GPU (rounded down to a multiple of "
                        "the global batch); no Train/ or Val/ directory is read")
    p.add_argument('--fake_val', type=int, default=None, metavar='M',
                   help="with --fake_stream: size of the validation set, generated once (default N // 4)")
    args = p.parse_args()
    print("Command line ~= \n", ' '.join(sys.argv))
    print("args = ", args)
    for attr, val in (("model_type", args.model_type), ("loss_type", args.loss_type), ("basemodel", args.backbone)):
        if val is not None:
            setattr(cf, attr, val)

    pred_grid = [int(i) for i in args.grid.split('x')]
    now = time.strftime("%c").replace('  ', '_').replace(' ', '_')
    log_dir = './logs/' + (args.name + '_' + now if args.name else now)
    print("Logging will go to ", log_dir)

    print("\n----------------------------\nStarting training...")
    model = train_network(weights_file=args.weights, datapath=args.datapath, fraction=args.fraction,
                          batch_size=args.batch_size, epochs=args.epochs, pred_grid=pred_grid, noaugment=args.noaugment,
                          log_dir=log_dir, lr_max=args.lrmax, freeze_fac=args.freeze_fac,
                          frozen_epochs=args.frozen_epochs, random_seed=args.random_seed,
                          augment_blur=args.augment_blur, bp_real=args.bp_real, bpmix_prob=args.bpmix_prob, warp=args.warp,
                          fake_stream=args.fake_stream, fake_val=args.fake_val, device_decode=args.device_decode,
                          device_aug_params=args.device_aug_params)

    if int(os.environ.get("RANK", "0")) == 0:
        print("\n----------------------------\nStarting model evaluation...")
        testpath = args.datapath + '/Test/'
        if not os.path.isdir(testpath):
            testpath = args.datapath + '/Val/'
        if args.fake_stream and not os.path.isdir(testpath):
            print("(--fake_stream: no Test/ or Val/ directory under", args.datapath, "-- evaluation on files skipped)")
        else:
            evaluate_network(model=model, weights_file="", datapath=testpath, fraction=1.0, log_dir="logs/Evaluation/",
                             batch_size=args.batch_size, pred_grid=pred_grid, set_means_ranges=False)
        if os.path.isdir(default_image_dir):      # the reference predicts on the author's unlabeled set here
            print("\n----------------------------\nStarting Zooniverse predictions...")
            predict_network(weights_file="", fraction=args.fraction, log_dir='logs/Predicting/',
                            batch_size=args.batch_size, model=model, X_pred='')
        weights2name = "final_" + args.weights
        print("Just to be sure: Saving model to", weights2name)
        model.save_weights(weights2name)
        print("And saving full model too")
        model.save("full_model.h5")
        for f in (weights2name, "full_model.h5", "nohup.out"):
            if os.path.exists(f):
                shutil.copy(f, log_dir)
        print("SPNet execution completed.")
    import torch.distributed as dist
    if dist.is_initialized():
        dist.destroy_process_group()
