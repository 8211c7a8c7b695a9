"""Training-loop callbacks with the protocol and names of the reference's spnet/callbacks.py.

  Callback                    minimal Keras-style base (set_model / on_train_begin / on_epoch_begin /
                              on_batch_begin / on_epoch_end)
  AugmentOnTheFly             callbacks.py:272-341 -- per-epoch cutout + salt&pepper of the WHOLE training
                              set from pristine frames, frame order 0..N-1 (reference RNG order), but the
                              frames live in HBM and the pixel work runs in HIP kernels
  get_1cycle_schedule,
  OneCycleScheduler           callbacks.py:346-406 -- per-batch learning-rate table
  MyProgressCallback          callbacks.py:58-265 -- validation predict, per-term losses.dat, count
                              metrics, progress.png, overlay drawings
  FreshFakeESPI               (additive) a fresh synthetic training set every epoch, generated in HBM
  ParallelCheckpointCallback  callbacks.py:20-41 -- weights + full-model checkpoints every N epochs
"""
import os
import time

import numpy as np

from . import config as cf
from . import diagnostics, utils


class Callback:
    def __init__(self):
        self.model = None

    def set_model(self, model):
        self.model = model

    def on_train_begin(self, logs=None):
        pass

    def on_epoch_begin(self, epoch, logs=None):
        pass

    def on_batch_begin(self, batch, logs=None):
        pass

    def on_batch_end(self, batch, logs=None):
        pass

    def on_epoch_end(self, epoch, logs=None):
        pass

    def on_train_end(self, logs=None):
        pass


# ----------------------------------------------------------------------------- LR schedule
def get_1cycle_schedule(lr_max=1e-3, n_data_points=8000, epochs=200, batch_size=40, verbose=0):
    """Look-up table of per-iteration learning rates: linear warm-up over the first 30 % of the
    iterations from lr_max/25 to lr_max, then cosine annealing down to lr_max/25/1e4
    (callbacks.py:346-377)."""
    pct_start, div_factor = 0.3, 25.
    lr_start = lr_max / div_factor
    lr_end = lr_start / 1e4
    n_iter = n_data_points * epochs // batch_size
    a1 = int(n_iter * pct_start)
    a2 = n_iter - a1
    warm = np.linspace(lr_start, lr_max, a1)
    anneal = (lr_max - lr_end) * (1 + np.cos(np.linspace(0, np.pi, a2))) / 2 + lr_end
    return np.concatenate((warm, anneal))


class OneCycleScheduler(Callback):
    """Sets model.optimizer.lr from the table before every batch; the iteration counter is never reset
    between fit() calls (callbacks.py:380-406)."""

    def __init__(self, **kwargs):
        super().__init__()
        self.verbose = kwargs.get('verbose', 0)
        self.lrs = get_1cycle_schedule(**kwargs)
        self.iteration = 0

    def on_batch_begin(self, batch, logs=None):
        self.model.optimizer.lr = float(self.lrs[min(self.iteration, len(self.lrs) - 1)])
        self.iteration += 1

    def on_epoch_end(self, epoch, logs=None):
        if logs is not None:
            logs['lr'] = self.model.optimizer.lr
        if self.verbose > 0:
            print('\nLearning rate =', self.model.optimizer.lr)


# ----------------------------------------------------------------------------- augmentation
class AugmentOnTheFly(Callback):
    """Each epoch: X[i] = augment(X_orig[i]) for i = 0..N-1, Y unchanged (callbacks.py:319-338).

    X may be a numpy array (uploaded once; the reference's host-RAM copy X_orig becomes a device
    tensor) or already a device tensor.  The augmented set is a second device tensor that the model's
    fit() reads batches from (`model.set_train_frames`)."""

    def __init__(self, X, Y, orig_img_shape=(384, 512), aug_every=1, chunk=256, seed=1, real_blur=False,
                 bandpass_real=None, bpmix_prob=0.3, warp=False, warp_files=None, pred_grid=(6, 6, 2), warp_source=None,
                 warp_targets="host", device_decode=False, params="host"):
        """real_blur=False reproduces the reference, whose Gaussian blur is a no-op (the result of cv2.GaussianBlur is
        discarded, augmentation.py:66-70); True applies it (train_spnet.py --augment_blur).
        bandpass_real: directory of real *.png frames of the training frames' size -- after the blur, a frame is
        band-pass mixed with probability bpmix_prob (bp_mixup, callbacks.py:311-315, whose call the reference has
        commented out; train_spnet.py --bp_real / --bpmix_prob).  None (default): off.
        warp (train_spnet.py --warp; needs warp_files, the PNG of every row of X in X's order, each with its same-stem
        CSV): every epoch each frame is first flipped / rotated / shifted as augment_preproc.py does offline -- a fresh
        draw per frame and epoch, the frame's warp draws ahead of its cutout draws -- at the files' own size
        (spnet_warp_chain_u8), resized to X's frame size as the input codec resizes (spnet_resize_u8; 'big' frames need
        none) and then augmented as before; its targets are recomputed from the warped metadata (augmentation.
        warp_targets) into Y_aug, which fit() trains on (Model.set_train_targets).  A frame whose warp would put a third
        ellipse into a grid cell keeps its unwarped pixels and targets for that epoch (counted, printed once per epoch).
        The cutout fill range stays that of the unwarped frame.  warp=False (default): nothing of this exists, the RNG
        stream and the frames are what they were.
        warp_source (instead of warp_files; implies warp): an augmentation.DeviceWarper that holds the full-size frames
        of X's rows AND their metadata as device tensors -- frames that have no files (FreshFakeESPI(..., warper=...)
        refills it every epoch).  warp_targets: "host" (default) = the targets of a chunk are computed in numpy
        (warp_targets) before its warp is launched; "device" (needs device metadata, so a warp_source; and a warp_source
        needs it) = they come from spnet_encode_targets, which also rewrites the warp records of the rejected frames: a
        chunk is records upload -> targets -> warp -> resize -> cutout ... with no synchronisation between them, and the
        rejected count is summed on the device and read once per epoch.
        device_decode (with warp_files and / or a bandpass_real directory): the full-size frames of the warp, and the grey
        real frames of the mix-up, are decoded on the GPU from the files' bytes (spnet_amd.png) instead of by Pillow and
        uploaded: the same frames.
        params: "host" (default) = the random parameters are drawn per frame with numpy's / Python's RNGs in the
        reference's call order, as above.  "device" (train_spnet.py --device_aug_params) = one spnet_augment_params launch
        per chunk draws them in HBM -- cutout, salt and pepper, blur and, with a warp_source, the warp's flip / angle /
        shift with its matrices -- from a keyed stream of its own: the reference's distributions (the rotation angle
        quantised to 20/2048 degrees), other values, each a function of (seed, the model's epoch counter, sample index)
        only, so a sample's augmentation in an epoch is the same single-process and at any world size.  No per-frame host
        work and no parameter upload; the band-pass mix-up's gate / row / scale alone are computed on the host (vectorised,
        from the same keys) and uploaded, because its kernel takes a compacted list.  Not with warp_files: their metadata
        path computes the targets on the host from host-drawn parameters."""
        super().__init__()
        import torch
        from . import parallel
        from .augmentation import DeviceAugmenter
        self.X, self.Y = X, Y
        self.aug_every = aug_every
        self.orig_img_shape = orig_img_shape
        self.chunk = chunk
        self.seed = seed
        if params not in ("host", "device"):
            raise ValueError("AugmentOnTheFly: params must be 'host' or 'device', got %r" % (params,))
        if params == "device" and (warp_files is not None or (warp and warp_source is None)):
            raise ValueError("AugmentOnTheFly: params='device' draws the warp for a warp_source (device metadata, "
                             "warp_targets='device'); warp_files is the host-metadata path, whose targets are computed on "
                             "the host from host-drawn parameters -- use params='host' with warp_files")
        self.params = params
        parallel.init_distributed()          # this rank's GPU (no-op if the model already did it)
        dev = parallel.local_device()
        self.X_orig = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X)).to(dev)
        self.X_aug = self.X_orig.clone()      # rows no epoch has augmented yet hold the pristine frame, not garbage
        self.augmenter = DeviceAugmenter(self.X_orig, real_blur=real_blur, bandpass_real=bandpass_real,
                                         bpmix_prob=bpmix_prob, device_decode=device_decode)
        self.warper = None
        self.rejected = 0                     # frames of the last augmented epoch whose warp was rejected
        if warp_targets not in ("host", "device"):
            raise ValueError("AugmentOnTheFly: warp_targets must be 'host' or 'device', got %r" % (warp_targets,))
        if (warp_source is not None) != (warp_targets == "device"):
            raise ValueError("AugmentOnTheFly: warp_source and warp_targets='device' go together (the device codec reads "
                             "device metadata; files' metadata is on the host)")
        self.warp_targets = warp_targets
        if warp or warp_source is not None:
            self._setup_warp(warp_files, pred_grid, dev, warp_source, device_decode)

    def _setup_warp(self, warp_files, pred_grid, dev, warp_source=None, device_decode=False):
        import torch
        from .augmentation import DeviceWarper
        n = int(self.X_orig.shape[0])
        if self.X_orig.dim() != 4 or self.X_orig.shape[-1] != 1:
            raise ValueError("AugmentOnTheFly(warp=True) is for one-channel frames [N,H,W,1]")
        if warp_source is not None:
            if warp_files is not None:
                raise ValueError("AugmentOnTheFly: warp_files or warp_source, not both")
            if warp_source.N != n or warp_source.meta_dev is None or tuple(warp_source.pred_grid) != tuple(pred_grid):
                raise ValueError("AugmentOnTheFly: warp_source must hold the %d training frames with device metadata and "
                                 "pred_grid %s" % (n, tuple(pred_grid)))
            self.warper = warp_source
            self._counts = torch.zeros(2, dtype=torch.int64, device=dev)      # rejected warps, unwarped overflows
        else:
            if warp_files is None or len(warp_files) != n:
                raise ValueError("AugmentOnTheFly(warp=True) needs warp_files: the PNG file of each of the %d training frames" % n)
            files = list(warp_files)
            if device_decode:
                from .png import read_png_device
                X_dev = read_png_device(files, device=dev)
            else:
                X_full, _ = utils.build_X(n, files, grayscale=True, as_uint8=True, device_resize=True)
                X_dev = torch.from_numpy(X_full[..., 0]).to(dev)
            meta = [utils.read_metadata(os.path.splitext(f)[0] + cf.meta_extension) for f in files]
            self.warper = DeviceWarper(X_dev, meta, pred_grid=pred_grid)
        Yh = self.Y.detach().cpu().numpy() if isinstance(self.Y, torch.Tensor) else np.asarray(self.Y)
        self.Y_aug = torch.from_numpy(np.ascontiguousarray(Yh, dtype=np.float32)).to(dev)
        self._y_upload = None
        self.label_seconds = 0.0              # host time of the last epoch's draws' targets (tools/warp_time.py)

    def _augment_chunk(self, idx, seeds, out, epoch=None, idx_dev=None):
        """out[j] = augmented frame idx[j] (device [B,h,w,1]); with warp: warped first, and -> (Y [B,576] device, number
        of rejected frames -- 0 with warp_targets="device", which counts them in self._counts instead), else None.
        params="device": idx_dev holds idx as an int32 device tensor and the chunk's parameters are drawn there from
        (self.seed, epoch, sample index) in one launch; seeds is not used."""
        import torch
        from . import _lib as L
        aug, wr = self.augmenter, self.warper
        on_device = self.params == "device"
        if wr is None:
            p = aug.draw_device(idx_dev, self.seed, epoch, host_index=idx) if on_device else aug.draw(idx, seeds=seeds)
            aug.apply(p, out)
            return None
        if on_device:
            from .augmentation import draw_params_device
            p, wp = draw_params_device(idx_dev, self.seed, epoch, augmenter=aug, warper=wr)
            aug._add_bandpass_keyed(p, idx_dev, self.seed, epoch, idx)
        else:
            wp = wr.new_params(idx)
            p = aug.draw(idx, seeds=seeds, before=lambda j, i: wr.draw_into(wp, j))
        device_targets = self.warp_targets == "device"
        t0 = time.time()
        if device_targets:
            Y, flags = wr.targets_device(wp)          # ahead of the warp: it rewrites the rejected frames' records
            self._counts += torch.stack([(flags != 0).sum(), (flags == 2).sum()])
        else:
            Y, rejected = wr.targets(wp)
        self.label_seconds += time.time() - t0
        B, dev = len(idx), self.X_aug.device
        warped = torch.empty((B, aug.H, aug.W), dtype=torch.float32, device=dev)
        if (wr.H, wr.W) == (aug.H, aug.W):
            wr.apply(wp, out_f=warped)
        else:
            from .resize import resize_u8_device
            full = torch.empty((B, wr.H, wr.W), dtype=torch.uint8, device=dev)
            wr.apply(wp, out_u8=full)
            resize_u8_device(full, (aug.H, aug.W), out_f=warped)
            self.last_full = full             # the chunk's warped full-size frames (tests)
        aug.apply(p, out, src=warped)
        self.last_warp = wp
        if device_targets:
            return Y, 0
        if self._y_upload is None:
            self._y_upload = L.AsyncUploader(dev)
        return self._y_upload("Y", Y), int(rejected.sum())

    def _report_rejected(self):
        if self.warper is not None and self.warp_targets == "device":       # the epoch's one read back of the label path
            from .augmentation import UNWARPED_OVERFLOW
            self.rejected, overflowed = (int(v) for v in self._counts.tolist())
            self._counts.zero_()
            if overflowed:
                raise AssertionError(UNWARPED_OVERFLOW)
        if self.warper is not None:
            print("   Augmenting on the fly: %d warps rejected (a third ellipse in one grid cell): those frames keep their "
                  "unwarped targets this epoch" % self.rejected)

    def set_model(self, model):
        super().set_model(model)
        if hasattr(model, "set_train_frames"):
            model.set_train_frames(self.X, self.X_aug)
        if self.warper is not None and hasattr(model, "set_train_targets"):
            model.set_train_targets(self.Y, self.Y_aug)

    def on_epoch_begin(self, epoch, logs=None):
        if 0 != epoch % self.aug_every:
            return
        shard = getattr(self.model, "epoch_indices", None) if getattr(self.model, "world", 1) > 1 else None
        if shard is not None:
            return self._augment_shard(np.asarray(shard), getattr(self.model, "_epochs_seen", epoch))
        n = self.X_orig.shape[0]
        self.rejected, self.label_seconds = 0, 0.0
        on_device = self.params == "device"
        if on_device:                       # the key's epoch is the counter _augment_shard takes: the same draws at any world size
            import torch
            key_epoch = getattr(self.model, "_epochs_seen", epoch)
            every = torch.arange(n, dtype=torch.int32, device=self.X_aug.device)
        for lo in range(0, n, self.chunk):
            hi = min(n, lo + self.chunk)
            if (lo // self.chunk) % 16 == 0 or hi == n:
                print("   Augmenting on the fly: ", hi, "/", n, "\r", sep="", end="")
            if on_device:
                res = self._augment_chunk(np.arange(lo, hi), None, self.X_aug[lo:hi], key_epoch, every[lo:hi])
            else:
                res = self._augment_chunk(list(range(lo, hi)), None, self.X_aug[lo:hi])
            if res is not None:
                self.Y_aug[lo:hi].copy_(res[0])
                self.rejected += res[1]
        print("")
        self._report_rejected()


    def _augment_shard(self, shard, epoch):
        """Data parallel: only the samples this rank trains on in this epoch are augmented, each from its own RNG
        stream seeded by (seed, epoch, sample index) -- the augmented frame of a sample does not depend on the world
        size or on the rank that draws it."""
        import torch
        from . import parallel
        tmp = None
        self.rejected, self.label_seconds = 0, 0.0
        on_device = self.params == "device"
        if on_device:                       # the shard's indices go up once; the keyed stream needs no per-sample seeds
            every = torch.from_numpy(np.ascontiguousarray(shard, dtype=np.int32)).to(self.X_aug.device)
        for lo in range(0, len(shard), self.chunk):
            idx = shard[lo:lo + self.chunk]
            if tmp is None or tmp.shape[0] != len(idx):
                tmp = torch.empty((len(idx),) + tuple(self.X_aug.shape[1:]), device=self.X_aug.device)
            if on_device:
                res = self._augment_chunk(idx, None, tmp, epoch, every[lo:lo + self.chunk])
                where = every[lo:lo + self.chunk].to(torch.int64)
            else:
                seeds = [parallel.sample_seed(self.seed, epoch, i) for i in idx]
                res = self._augment_chunk(list(idx), seeds, tmp)
                where = torch.as_tensor(idx, dtype=torch.int64, device=self.X_aug.device)
            self.X_aug.index_copy_(0, where, tmp)
            if res is not None:
                self.Y_aug.index_copy_(0, where, res[0])
                self.rejected += res[1]
        self._report_rejected()


class FreshFakeESPI(Callback):
    """Each epoch: a FRESH set of synthetic training frames and targets from a fake_espi.FakeStream -- no files, and no
    frame is ever seen twice.  fit(X, Y) is called with this callback's X and Y (placeholders that only identify the
    training set: with X=None, cb.X is the device frame tensor itself -- no host copy of the frames is ever made -- and with
    Y=None, cb.Y is a host copy of the first targets); the frames fit() reads are cb.X_dev [n,H,W,1] and the targets cb.Y_dev
    [n, n_targets], registered through Model.set_train_frames / set_train_targets and refilled by stream.epoch() at every
    epoch begin.  The stream epoch is first_epoch + the number of epochs this callback has begun so far (it keeps counting
    over several fit() calls and over a change of model, as train_spnet.py's unfreeze makes).  Until the first epoch begins
    the tensors hold epoch first_epoch's frames, never garbage.

    Data parallel: every rank generates the same n frames (same seed, same epoch) into its own tensors and fit()'s
    sharding picks this rank's samples; no collective is added.

    With AugmentOnTheFly: build it on the DEVICE tensor, AugmentOnTheFly(cb.X_dev, cb.Y, ...), call fit(cb.X_dev, cb.Y, ...)
    and list this callback BEFORE it.  Order within an epoch: this callback writes the fresh frames into cb.X_dev, which is
    the augmenter's pristine set (it keeps a device tensor as it is); AugmentOnTheFly then writes cutout / salt and pepper
    / blur / band-pass mix-up of them into its X_aug, which is what fit() reads (it registers last).  The cutout fill
    range is the min / max of the frames AugmentOnTheFly was built on (epoch first_epoch's; a noisy fake-ESPI frame spans
    the whole range).

    warper (True, or an augmentation.DeviceWarper with device metadata for n frames of 384 x 512): the stream also keeps
    each epoch's full-size uint8 frames and label rows on the device (stream.epoch(keep_u8=True)) and the warper -- True:
    one built on those very tensors, cb.warper -- is refilled with them (set_frames) at every epoch begin, before the
    AugmentOnTheFly(cb.X_dev, cb.Y, warp_source=cb.warper, warp_targets="device") listed behind this callback warps them:
    fresh frames every epoch and a fresh flip / rotation / shift of each, no file and no label on the host."""

    def __init__(self, X, Y, stream, first_epoch=0, verbose=True, warper=None):
        super().__init__()
        self.stream, self.first_epoch, self.verbose = stream, int(first_epoch), verbose
        self.warper = None
        self.X_dev, self.Y_dev = stream.epoch(self.first_epoch, verbose=False, keep_u8=bool(warper))
        if warper:
            if warper is True:
                from .augmentation import DeviceWarper
                warper = DeviceWarper(stream.U_full, (stream.rows, stream.count), pred_grid=stream.pred_grid)
            self.warper = warper
            warper.set_frames(stream.U_full, stream.rows, stream.count)
        self.X = self.X_dev if X is None else X
        self.Y = self.Y_dev.cpu().numpy() if Y is None else Y
        if tuple(self.X.shape) != tuple(self.X_dev.shape) or tuple(self.Y.shape) != tuple(self.Y_dev.shape):
            raise ValueError("FreshFakeESPI: X / Y are %s / %s, the stream yields %s / %s"
                             % (tuple(self.X.shape), tuple(self.Y.shape), tuple(self.X_dev.shape), tuple(self.Y_dev.shape)))
        self.epochs_filled = []             # the stream epochs generated so far (first_epoch's initial fill not counted)

    def set_model(self, model):
        super().set_model(model)
        model.set_train_frames(self.X, self.X_dev)
        model.set_train_targets(self.Y, self.Y_dev)

    def on_epoch_begin(self, epoch, logs=None):
        e = self.first_epoch + len(self.epochs_filled)
        self.stream.epoch(e, self.X_dev, self.Y_dev, verbose=self.verbose and getattr(self.model, "rank", 0) == 0,
                          keep_u8=self.warper is not None)
        if self.warper is not None:
            self.warper.set_frames(self.stream.U_full, self.stream.rows, self.stream.count)
        self.epochs_filled.append(e)


# ----------------------------------------------------------------------------- checkpoints
class ParallelCheckpointCallback(Callback):
    def __init__(self, serial_model, filepath="weights.hdf5", save_every=1, dir='.'):
        super().__init__()
        self.model_to_save = serial_model
        self.save_every = save_every
        self.weights_path = dir + '/' + filepath
        self.model_path = dir + '/' + "spnet.model"

    def on_epoch_end(self, epoch, logs=None):
        if (1 == self.save_every) or ((0 == ((epoch + 1) % self.save_every)) and (epoch > 0)):
            os.makedirs(os.path.dirname(self.weights_path) or ".", exist_ok=True)
            print("Saving weights checkpoint to", self.weights_path)
            self.model_to_save.save_weights(self.weights_path)
            print("Saving entire model checkpoint to", self.model_path)
            self.model_to_save.save(self.model_path)


# ----------------------------------------------------------------------------- progress
hist, train_loss_hist, val_loss_hist, my_val_loss_hist, acc_hist = [], [], [], [], []
center_loss_hist, size_loss_hist, angle_loss_hist, noobj_loss_hist, rings_loss_hist = [], [], [], [], []
global_count = 0


class MyProgressCallback(Callback):
    def __init__(self, X_val=None, Y_val=None, val_file_list=None, log_dir="./logs", use_tb=False,
                 pred_shape=[3, 3, 4, 6], num_draw=40, make_plots=True):
        super().__init__()
        self.X_val, self.Y_val, self.val_file_list = X_val, Y_val, val_file_list
        self.log_dir, self.pred_shape = log_dir, pred_shape
        self.num_draw, self.make_plots = num_draw, make_plots
        os.makedirs(log_dir, exist_ok=True)
        self.loss_file = open(log_dir + '/losses.dat', 'a')
        self.loss_file.write('# epoch Train_total Val_total center size angle noobj class\n')

    def on_epoch_end(self, epoch, logs=None):
        from . import models
        global global_count
        logs = logs or {}
        global_count += 1
        hist.append(global_count)
        train_loss_total, val_loss_total = logs.get('loss'), logs.get('val_loss')
        train_loss_hist.append(train_loss_total)
        val_loss_hist.append(val_loss_total)
        m = self.Y_val.shape[0]
        print("\n MyProgressCallback: predicting, testing & saving plot")
        print("    Predicting... (m = ", m, " frames in val set)", sep="")
        t0 = time.time()
        Y_pred = self.model.predict(self.X_val)
        elapsed = time.time() - t0
        print("    ...elapsed time to predict = ", elapsed, "s.   FPS = ", m * 1.0 / elapsed)
        my_val_loss, parts = models.my_loss(self.Y_val, Y_pred)
        center_loss, size_loss, angle_loss, noobj_loss, rings_loss = parts
        for lst, v in zip((my_val_loss_hist, center_loss_hist, size_loss_hist, angle_loss_hist, noobj_loss_hist,
                           rings_loss_hist), (my_val_loss, center_loss, size_loss, angle_loss, noobj_loss, rings_loss)):
            lst.append(v)
        self.loss_file.write(f'{epoch} {train_loss_total} {my_val_loss} {center_loss} {size_loss} {angle_loss} '
                             f'{noobj_loss} {rings_loss}\n')
        self.loss_file.flush()
        if cf.loss_type != 'same':
            Y_pred[:, cf.ind_noobj::cf.vars_per_pred] = 1.0 / (1.0 + np.exp(-Y_pred[:, cf.ind_noobj::cf.vars_per_pred]))
        Yv, Yp = utils.denorm_Y(self.Y_val), utils.denorm_Y(Y_pred)
        (ring_miscounts, ring_truecounts, total_obj, false_obj_pos, false_obj_neg, true_obj_pos, true_obj_neg,
         pix_err, ipem) = diagnostics.calc_errors(Yp, Yv)
        mistakes = ring_miscounts + false_obj_pos + false_obj_neg
        class_acc = (total_obj - mistakes) * 100.0 / max(total_obj, 1)
        acc_hist.append(class_acc)
        print('    Losses: Epoch Train:total Val:total   center     size       angle      noobj      rings')
        print(f'          {epoch:3d}     {train_loss_total}   {val_loss_total}   {center_loss:.3e} '
              f' {size_loss:.3e}  {angle_loss:.3e}  {noobj_loss:.3e}  {rings_loss:.3e}')
        if self.make_plots:
            self._plot(class_acc)
        if self.val_file_list is not None and self.num_draw > 0:
            try:
                utils.show_pred_ellipses(Yv, Yp, self.val_file_list, num_draw=self.num_draw, log_dir=self.log_dir,
                                         ind_extra=ipem)
            except (FileNotFoundError, OSError) as exc:      # synthetic in-memory sets have no image files
                print("    (skipping overlay drawings:", exc, ")")
        print("    In whole val dataset:")
        print('        Mean pixel error =', np.mean(pix_err))
        print("        Max pixel error =", pix_err[ipem], " (index =", ipem, ").")
        tot = max(total_obj, 1)
        print("    Ring correct counts = ", ring_truecounts, ' / ', total_obj, '.   = ', 100 * ring_truecounts / tot,
              ' % ring-class accuracy', sep="")
        print("         Ring miscounts = ", ring_miscounts, ' / ', total_obj, sep="")
        print("        False positives = ", false_obj_pos, ' / ', total_obj, sep="")
        print("        False negatives = ", false_obj_neg, ' / ', total_obj, sep="")
        print("         True positives = ", true_obj_pos, ' / ', total_obj, sep="")
        print("         True negatives = ", true_obj_neg, sep="")
        print("    Total Mistakes = ", mistakes, ' / ', total_obj, '.   => ', class_acc,
              ' % class. accuracy rate (lack of mistakes)', sep="")

    def _plot(self, class_acc):
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        fig = plt.figure(figsize=(10, 3.75))
        ax = plt.subplot(121)
        for series, label in ((train_loss_hist, "Train"), (my_val_loss_hist, "Val: Total"), (center_loss_hist, "Val: Center"),
                              (size_loss_hist, "Val: Size"), (angle_loss_hist, "Val: Angle"),
                              (noobj_loss_hist, "Val: NoObj"), (rings_loss_hist, "Val: Rings")):
            ys = [np.nan if v is None else v for v in series]
            ax.loglog(hist, ys, '-', label=label)
        ax.set_xlabel('(Global) Epoch')
        ax.set_ylabel('Loss')
        ax.legend(loc='lower left', fancybox=True, framealpha=0.8)
        ax = plt.subplot(122, ylim=[0, 100])
        ax.plot(hist, acc_hist, '-', color='orange', label='Acc = {:5.2f} %'.format(class_acc))
        ax.set_xlabel('(Global) Epoch')
        ax.set_ylabel('Accuracy (%)')
        ax.legend(loc='lower right', fancybox=True, framealpha=0.8)
        fig.tight_layout()
        plt.savefig(self.log_dir + '/progress.png')
        plt.close(fig)
