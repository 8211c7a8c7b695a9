"""Augmentation of ESPI frames on the MI355X -- the surface of the reference's spnet/augmentation.py.

Train-time (AugmentOnTheFly, spnet/callbacks.py:272-341): cutout + salt-and-pepper + the reference's
no-op blur.  The random PARAMETERS are drawn on the host with numpy's global RNG in exactly the
reference's call order (so a seeded run reproduces the reference's augmented frames bit for bit),
the PIXEL work runs in HIP kernels on frames that never leave HBM (csrc/augment.hip).  Opt-in (draw_device,
draw_params_device; AugmentOnTheFly(params="device")): the parameters of a chunk drawn in HBM by one launch
(csrc/augment_params.hip) from a keyed stream of its own -- the same distributions, other values.

Offline warps (augment_preproc.py:56-100): flip / rotate / translate = one inverse-affine bilinear
gather kernel plus the reference's host-side metadata arithmetic.  DeviceWarper is the batched, device-resident form: the
whole flip -> rotate -> translate chain of a batch in one launch (csrc/warp.hip), bit-identical to the three calls, with the
metadata arithmetic and the target codec vectorised on the host (warp_metadata, warp_targets) -- the oracle -- and run on the
device by one more launch (csrc/targets.hip: encode_targets_device, DeviceWarper.targets_device), which keeps the labels of
device-resident metadata in HBM.

Band-pass mix-up (augmentation.py:10-62): BandpassPool holds the real frames and their low-frequency windows on the
device, BandpassMixer draws and applies the mix-up (csrc/bandpass.hip), bandpass_mixup is the reference's function.
"""
import glob
import os
import random

import numpy as np
import torch

from . import _lib as L
from .fake_espi import _cached_table

MAX_RECTS = 6


_stream = L.current_stream


def cleanup_angle(angle):
    """Wrap into [0,180) (spnet/augmentation.py:74-79)."""
    while angle < 0:
        angle += 180
    while angle >= 180:
        angle -= 180
    return angle


# ----------------------------------------------------------------------------- parameter draws
def draw_cutout(shape, lo, hi, max_regions=6, minsize=11, maxsize=75):
    """RNG call order of cutout_inplace (augmentation.py:117-134).  Returns [(r0,r1,c0,c1,value)]."""
    H, W = shape[0], shape[1]
    n = np.random.randint(0, high=max_regions + 1)
    out = []
    for _ in range(n):
        r0, c0 = np.random.randint(0, H - minsize), np.random.randint(0, W - minsize)
        dr, dc = np.random.randint(minsize, maxsize), np.random.randint(minsize, maxsize)
        r1, c1 = min(r0 + dr, H - 1), min(c0 + dc, W - 1)
        out.append((r0, r1, c0, c1, np.float32(np.random.uniform(lo, hi))))
    return out


def draw_saltpepper(shape, salt_vs_pepper=0.2, amount=0.004):
    """RNG call order of salt_n_pepa_inplace (augmentation.py:157-180).  None when the coin says skip,
    else int arrays (salt_rows, salt_cols, pepper_rows, pepper_cols)."""
    if np.random.choice(['good', 'not good']) != 'good':
        return None
    size = int(np.prod(shape))
    n_salt = int(np.ceil(amount * size * salt_vs_pepper))
    n_pepper = int(np.ceil(amount * size * (1.0 - salt_vs_pepper)))
    sr, sc = [np.random.randint(0, d - 1, n_salt) for d in shape[0:2]]
    pr, pc = [np.random.randint(0, d - 1, n_pepper) for d in shape[0:2]]
    return sr, sc, pr, pc


def saltpepper_counts(shape, salt_vs_pepper=0.2, amount=0.004):
    size = int(np.prod(shape))
    return int(np.ceil(amount * size * salt_vs_pepper)), int(np.ceil(amount * size * (1.0 - salt_vs_pepper)))


def draw_blur_gate(blur_prob_outer=0.4, blur_prob=0.3):
    """AugmentOnTheFly.blur + blur_inplace (callbacks.py:306-309, augmentation.py:66-70).  The
    reference discards cv2.GaussianBlur's result, so only the RNG consumption is reproduced.
    Returns the kernel size it would have used, or 0."""
    if np.random.rand() < blur_prob_outer:
        if np.random.random() <= blur_prob:
            return random.choice([3, 7])
    return 0


# ----------------------------------------------------------------------------- parameter draws on the device
AUG_ANGLE_MID = 2048              # spnet_augment_params: angle index k in 0..4096, angle = (k - 2048) * (20 / 2048) degrees
_AUG_TRIG = {}
_M32 = np.uint64(0xFFFFFFFF)


def aug_angle(k):
    """The quantised warp angle of index k, in degrees (float64; k = 2048 is 0)."""
    return (np.asarray(k, np.float64) - AUG_ANGLE_MID) * (20.0 / 2048.0)


def aug_trig_table(device=None):
    """(cos, sin) of np.deg2rad(aug_angle(k)), k = 0..4096, float64 [4097,2]: what rotation_matrix_2d computes for these
    angles, so the matrices spnet_augment_params forms from it have warp_minv's / warp_fwd's bits.  device: a cached device
    tensor instead of the numpy array."""
    def make():
        rad = np.deg2rad(aug_angle(np.arange(2 * AUG_ANGLE_MID + 1)))
        return np.stack([np.cos(rad), np.sin(rad)], 1)
    return _cached_table(_AUG_TRIG, make, device)


def _mix32(x):
    """The samplers' 32-bit mixer (csrc/counter_rng.h) on uint64 arrays holding uint32 values."""
    x = np.asarray(x, np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & _M32
    return x ^ (x >> np.uint64(16))


def _keyed_draw(key, k):
    return _mix32(key ^ np.uint64((k * 0x85ebca6b + 0xc2b2ae35) & 0xFFFFFFFF))


def draw_bandpass_keyed(seed, epoch, sample_index, n_real, bpmix_prob):
    """The band-pass mix-up's three draws per sample from the keyed stream of spnet_augment_params (slot 0, draws 5..7: the
    recipe is in include/spnet_hip.h), for a whole chunk in numpy: spnet_bandpass_apply takes a compacted list whose length
    the host must know, so these stay on the host.  -> (gate bool [B], table row int32 [B], scale float32 [B])."""
    idx = np.asarray(sample_index, np.int64).astype(np.uint64) & _M32
    seed_key = _mix32(_mix32(np.uint64((int(seed) & 0xFFFFFFFF) ^ 0x3c6ef372)) + np.uint64(int(epoch) & 0xFFFFFFFF))
    k0 = _mix32(_mix32(seed_key ^ idx))                                   # key(slot 0) = mix(skey + 0)
    gate = (_keyed_draw(k0, 5) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 < float(bpmix_prob)
    row = ((_keyed_draw(k0, 6) * np.uint64(max(4 * int(n_real), 1))) >> np.uint64(32)).astype(np.int32)
    s = np.float32(3) * ((_keyed_draw(k0, 7) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24))
    return gate, row, s


def _index_device(sample_index, device):
    """Sample indices, array-like (uploaded) or already an int32 device tensor, as an int32 device tensor."""
    if isinstance(sample_index, torch.Tensor):
        if not sample_index.is_cuda or sample_index.dtype != torch.int32 or sample_index.dim() != 1:
            raise ValueError("draw_device: sample indices as a tensor must be int32 [B] on the device")
        return sample_index.contiguous()
    return torch.from_numpy(np.ascontiguousarray(sample_index, dtype=np.int32)).to(device)


def draw_params_device(sample_index, seed, epoch, augmenter=None, warper=None):
    """ONE launch of spnet_augment_params on the current stream for the samples `sample_index` (array-like, or an int32
    device tensor, which is used as it is): the augmentation half for `augmenter`, the warp half for `warper`, either or
    both (they then share each sample's key).  Nothing is read back.  -> (augmentation dict or None, warp dict or None) of
    device tensors, see DeviceAugmenter.draw_device / DeviceWarper.draw_device."""
    if augmenter is None and warper is None:
        raise ValueError("draw_params_device: no augmenter and no warper")
    dev = (augmenter or warper).X.device
    index = _index_device(sample_index, dev)
    B = int(index.numel())
    ap = wp = None
    a = [0, 0, 0, 0, None, 1] + [None] * 6
    w = [0, 0, None, None, None]
    if augmenter is not None:
        g = augmenter
        npts = g.n_salt + g.n_pepper
        ibuf = torch.empty(B * (MAX_RECTS * 4 + 3 + 2 * npts), dtype=torch.int32, device=dev)      # one allocation
        cut = np.cumsum([0, B * MAX_RECTS * 4, B, B, B])
        ap = dict(index=index, rects=ibuf[cut[0]:cut[1]], nrect=ibuf[cut[1]:cut[2]], flag=ibuf[cut[2]:cut[3]],
                  ksize=ibuf[cut[3]:cut[4]], coords=ibuf[cut[4]:], vals=torch.empty(B * MAX_RECTS, device=dev))
        a = [g.H, g.W, g.n_salt, g.n_pepper, g.mm.data_ptr(), g.N] + \
            [ap[k].data_ptr() if ap[k].numel() else None for k in ("rects", "vals", "nrect", "coords", "flag", "ksize")]
    if warper is not None:
        rec = torch.empty(B * 8, dtype=torch.float64, device=dev)        # 64-byte records, 8-byte aligned
        fwd = torch.empty((B, 8), dtype=torch.float64, device=dev)
        wp = dict(index=index, records=rec.view(torch.int32), fwd=fwd, H=warper.H, W=warper.W)
        w = [warper.H, warper.W, aug_trig_table(dev).data_ptr(), rec.data_ptr() if B else None, fwd.data_ptr() if B else None]
    if B:
        with torch.cuda.device(dev):
            L.spnet_augment_params(int(seed) & 0xFFFFFFFF, int(epoch) & 0xFFFFFFFF, index.data_ptr(), B, *a, *w, _stream())
    return ap, wp


class DeviceAugmenter:
    """Keeps the pristine frames [N,H,W,1] in HBM and writes augmented batches into a device buffer."""

    def __init__(self, X_orig, real_blur=False, bandpass_real=None, bpmix_prob=0.3, device_decode=False):
        """bandpass_real (None = off, the reference's default: its bp_mixup call is commented out, callbacks.py:333): a
        directory of real *.png frames of the frames' size, a BandpassPool or a uint8 device tensor [R,H,W]; after the
        blur gate, np.random.rand() < bpmix_prob selects the frames that are band-pass mixed (callbacks.py:311-315).
        bpmix_prob <= 0 switches the stage off entirely (no draw is made)."""
        if not X_orig.is_cuda:
            raise RuntimeError("DeviceAugmenter needs device-resident frames (no CPU fallback)")
        self.X = X_orig.contiguous()
        self.N, self.H, self.W = X_orig.shape[0], X_orig.shape[1], X_orig.shape[2]
        self.shape = (self.H, self.W, 1)
        # False (default): the reference's blur, whose cv2.GaussianBlur result is discarded (augmentation.py:66-70:
        # RNG consumed, pixels untouched).  True: apply the blur that call computes (csrc/augment.hip).
        self.real_blur = real_blur
        mm = torch.empty(self.N, 2, device=self.X.device)
        scratch = torch.empty(self.N * 32, device=self.X.device)
        L.spnet_minmax(self.X.data_ptr(), self.N, self.H * self.W, mm.data_ptr(), scratch.data_ptr(), _stream())
        self.mm = mm                        # min/max of the pristine frames: cutout's fill range (draw_device reads it)
        self.mm_host = mm.cpu().numpy()
        self.n_salt, self.n_pepper = saltpepper_counts(self.shape)
        self._upload = None
        self.bpmix_prob = float(bpmix_prob)
        self.bp = None
        if bandpass_real is not None and self.bpmix_prob > 0:
            pool = bandpass_real if isinstance(bandpass_real, BandpassPool) else \
                BandpassPool.get(bandpass_real, self.H, self.W, self.X.device, device_decode=device_decode)
            if (pool.H, pool.W) != (self.H, self.W):
                raise ValueError("DeviceAugmenter: band-pass pool is %dx%d, the frames are %dx%d" % (pool.H, pool.W, self.H, self.W))
            self.bp = pool.mixer

    def draw(self, indices, seeds=None, before=None):
        """Host-side parameter draw for the given frame indices, reference RNG order per frame.  before (optional):
        before(j, i) is called for frame i (position j) after its seeding and ahead of its cutout draws -- where
        AugmentOnTheFly(warp=True) makes the frame's warp draws.  seeds (optional,
        one per frame): each frame's draws come from numpy / python streams seeded with its own seed (data parallel:
        a sample's augmentation then depends on its seed only, not on what was drawn before it); the process-wide
        RNG states are saved and restored around the draw, so later consumers of np.random / random are unaffected."""
        B = len(indices)
        npts = self.n_salt + self.n_pepper
        rects = np.zeros((B, MAX_RECTS, 4), np.int32)
        vals = np.zeros((B, MAX_RECTS), np.float32)
        nrect = np.zeros(B, np.int32)
        coords = np.zeros((B, 2, npts), np.int32)
        flag = np.zeros(B, np.int32)
        ksize = np.zeros(B, np.int32)
        saved = (np.random.get_state(), random.getstate()) if seeds is not None else None
        try:
            p = self._draw(indices, seeds, rects, vals, nrect, coords, flag, ksize, before)
            if self.bp is not None:
                p["bp_n"] = len(p["bp_sel"])
                for k, dt in (("bp_sel", np.int32), ("bp_row", np.int32), ("bp_s", np.float32)):
                    a = np.zeros(B, dt)             # fixed length B: one upload shape per batch size
                    a[:p["bp_n"]] = p[k]
                    p[k] = a
            return p
        finally:
            if saved is not None:       # the per-sample streams must not leak into the process-wide RNGs
                np.random.set_state(saved[0])
                random.setstate(saved[1])

    def _draw(self, indices, seeds, rects, vals, nrect, coords, flag, ksize, before=None):
        bp_sel, bp_row, bp_s = [], [], []
        for j, i in enumerate(indices):
            if seeds is not None:
                np.random.seed(int(seeds[j]))
                random.seed(int(seeds[j]))
            if before is not None:
                before(j, i)
            lo, hi = self.mm_host[i]
            rs = draw_cutout(self.shape, lo, hi)
            nrect[j] = len(rs)
            for k, (r0, r1, c0, c1, v) in enumerate(rs):
                rects[j, k] = (r0, r1, c0, c1)
                vals[j, k] = v
            sp = draw_saltpepper(self.shape)
            if sp is not None:
                flag[j] = 1
                coords[j, 0, :self.n_salt], coords[j, 1, :self.n_salt] = sp[0], sp[1]
                coords[j, 0, self.n_salt:], coords[j, 1, self.n_salt:] = sp[2], sp[3]
            ksize[j] = draw_blur_gate()
            if self.bp is not None and np.random.rand() < self.bpmix_prob:       # AugmentOnTheFly.bp_mixup gate
                i_real, flip, s = draw_bandpass(self.bp.pool.n_real)
                bp_sel.append(j)
                bp_row.append(4 * i_real + BP_FLIPS.index(flip))
                bp_s.append(s)
        p = dict(index=np.asarray(indices, np.int32), rects=rects, vals=vals, nrect=nrect, coords=coords, flag=flag,
                 ksize=ksize)
        if self.bp is not None:
            p.update(bp_sel=bp_sel, bp_row=bp_row, bp_s=bp_s)
        return p

    def draw_device(self, sample_index, seed, epoch, host_index=None):
        """The parameters of the samples `sample_index` drawn ON THE DEVICE (spnet_augment_params: a keyed stream of its own,
        every value a function of (seed, epoch, sample index) only; see include/spnet_hip.h) -> a dict of device tensors in
        draw()'s layout (index, rects, vals, nrect, coords, flag, ksize) that apply() takes without uploading anything.
        sample_index: array-like, or an int32 device tensor (used as it is).  With a band-pass pool the dict also holds
        bp_n (a host int) and host arrays bp_sel / bp_row / bp_s: the mix-up's draws come from the same keyed stream but are
        made on the host, vectorised over the chunk (draw_bandpass_keyed) -- they need the indices on the host, host_index
        when sample_index is a tensor (else it is copied back)."""
        p, _ = draw_params_device(sample_index, seed, epoch, augmenter=self)
        return self._add_bandpass_keyed(p, sample_index, seed, epoch, host_index)

    def _add_bandpass_keyed(self, p, sample_index, seed, epoch, host_index=None):
        if self.bp is not None:
            if host_index is None:
                host_index = sample_index.cpu().numpy() if isinstance(sample_index, torch.Tensor) else sample_index
            gate, row, s = draw_bandpass_keyed(seed, epoch, host_index, self.bp.pool.n_real, self.bpmix_prob)
            B = len(gate)
            sel = np.nonzero(gate)[0]
            p["bp_n"] = len(sel)
            for k, v, dt in (("bp_sel", sel, np.int32), ("bp_row", row[sel], np.int32), ("bp_s", s[sel], np.float32)):
                a = np.zeros(B, dt)                 # fixed length B, as draw() pads them
                a[:len(sel)] = v
                p[k] = a
        return p

    def _apply_device(self, p, out, src=None):
        """apply() for draw_device's dict: the same kernels on parameters that are already in HBM."""
        dev = self.X.device
        B = int(p["index"].numel())
        self._keep = p
        self.index_dev = p["index"]
        if B == 0:
            return out
        X = self.X if src is None else src
        L.spnet_cutout(X.data_ptr(), None if src is not None else p["index"].data_ptr(), out.data_ptr(), B, self.H, self.W,
                       p["rects"].data_ptr(), p["vals"].data_ptr(), p["nrect"].data_ptr(), _stream())
        mm = torch.empty(B * (2 + 32), device=dev)
        self._mm = mm
        L.spnet_minmax(out.data_ptr(), B, self.H * self.W, mm.data_ptr(), mm[2 * B:].data_ptr(), _stream())
        L.spnet_saltpepper(out.data_ptr(), B, self.H, self.W, p["coords"].data_ptr(), self.n_salt, self.n_pepper,
                           p["flag"].data_ptr(), mm.data_ptr(), _stream())
        if self.real_blur:                  # unconditionally: whether any frame drew a blur is not known here; ksize 0 copies
            tmp = torch.empty_like(out)
            L.spnet_gaussian_blur(out.data_ptr(), tmp.data_ptr(), B, self.H, self.W, p["ksize"].data_ptr(), _stream())
            out.copy_(tmp)
        if self.bp is not None and p["bp_n"] > 0:
            n = int(p["bp_n"])
            if self._upload is None:
                self._upload = L.AsyncUploader(dev)
            packed = self._upload("bp", np.concatenate([p["bp_sel"], p["bp_row"], p["bp_s"].view(np.int32)]))
            ws = torch.empty(L.spnet_bandpass_ws(n, self.H, self.W), device=dev)
            self._bp_ws, self._bp_up = ws, packed
            pool = self.bp.pool
            L.spnet_bandpass_apply(out.data_ptr(), 2, packed[:B].data_ptr(), B, n, self.H, self.W, pool.table.data_ptr(),
                                   4 * pool.n_real, packed[B:2 * B].data_ptr(), packed[2 * B:].view(torch.float32).data_ptr(),
                                   out.data_ptr(), 1, None, ws.data_ptr(), _stream())
        return out

    def apply(self, params, out, src=None):
        """out[j] = augmented copy of frame params['index'][j]; out is a device tensor [B,H,W,1].  src (optional, device
        float32 [B,H,W(,1)], not `out`): the batch's frames are read from src[j] instead (frames that were warped first).
        params: draw()'s host dict (packed and uploaded) or draw_device()'s device dict (nothing is uploaded)."""
        dev = self.X.device
        X = self.X
        if src is not None:
            if src.dtype != torch.float32 or not src.is_contiguous() or src.numel() != len(params["index"]) * self.H * self.W:
                raise ValueError("DeviceAugmenter.apply: src must be contiguous float32 [%d,%d,%d]" % (len(params["index"]), self.H, self.W))
        if isinstance(params["rects"], torch.Tensor):
            return self._apply_device(params, out, src)
        if src is not None:
            X = src
            params = dict(params, index=np.arange(len(params["index"]), dtype=np.int32))
        if self._upload is None:
            self._upload = L.AsyncUploader(dev)
        # ONE host -> device copy for the whole parameter set: every async copy from pinned memory is preceded by ~56 us
        # of idle GPU (rocprofv3 kernel trace: the gap in front of each __amd_rocclr_copyBuffer), so seven small uploads
        # cost a 12.5 ms step 0.4 ms.  All fields are 4-byte types: packed as int32 words, viewed back on the device.
        names = ("index", "rects", "vals", "nrect", "coords", "flag", "ksize")
        if self.bp is not None:
            names += ("bp_sel", "bp_row", "bp_s")
        flat = [np.ascontiguousarray(params[k]).reshape(-1).view(np.int32) for k in names]
        packed = self._upload("params", np.concatenate(flat))      # pinned ring + one async copy
        up, off = {}, 0
        for k, f in zip(names, flat):
            t = packed[off:off + f.size]
            up[k] = t.view(torch.float32) if params[k].dtype == np.float32 else t
            off += f.size
        B = len(params["index"])
        self._keep = up                    # keep the upload alive until the kernels have consumed it
        self.index_dev = up["index"]       # int32 frame indices of this batch on the device (label gathers reuse them)
        L.spnet_cutout(X.data_ptr(), up["index"].data_ptr(), out.data_ptr(), B, self.H, self.W,
                       up["rects"].data_ptr(), up["vals"].data_ptr(), up["nrect"].data_ptr(), _stream())
        mm = torch.empty(B * (2 + 32), device=dev)   # [B,2] result followed by B*32 floats of reduction scratch
        self._mm = mm
        L.spnet_minmax(out.data_ptr(), B, self.H * self.W, mm.data_ptr(), mm[2 * B:].data_ptr(), _stream())
        L.spnet_saltpepper(out.data_ptr(), B, self.H, self.W, up["coords"].data_ptr(), self.n_salt, self.n_pepper,
                           up["flag"].data_ptr(), mm.data_ptr(), _stream())
        if self.real_blur and params["ksize"].any():
            tmp = torch.empty_like(out)
            L.spnet_gaussian_blur(out.data_ptr(), tmp.data_ptr(), B, self.H, self.W, up["ksize"].data_ptr(), _stream())
            out.copy_(tmp)
        if self.bp is not None and params["bp_n"] > 0:
            # the gated frames only, in place, in network units: pixel = (x/2 + 1/2) * 255, mixed, back to [-1,1]
            n = int(params["bp_n"])
            ws = torch.empty(L.spnet_bandpass_ws(n, self.H, self.W), device=dev)
            self._bp_ws = ws
            pool = self.bp.pool
            L.spnet_bandpass_apply(out.data_ptr(), 2, up["bp_sel"].data_ptr(), B, n, self.H, self.W, pool.table.data_ptr(),
                                   4 * pool.n_real, up["bp_row"].data_ptr(), up["bp_s"].data_ptr(), out.data_ptr(), 1, None,
                                   ws.data_ptr(), _stream())
        return out

    def augment(self, indices, out):
        return self.apply(self.draw(indices), out)


# ----------------------------------------------------------------------------- in-place API on device frames
def cutout_inplace(img, max_regions=6, minsize=11, maxsize=75):
    """Reference signature (augmentation.py:117); `img` is ONE device frame [H,W,1]."""
    _require_cuda(img)
    H, W = img.shape[0], img.shape[1]
    mm = torch.empty(2 + 32, device=img.device)
    n = np.random.randint(0, high=max_regions + 1)
    if n == 0:
        return
    L.spnet_minmax(img.data_ptr(), 1, H * W, mm.data_ptr(), mm[2:].data_ptr(), _stream())
    lo, hi = mm[:2].cpu().numpy()
    rects = np.zeros((1, MAX_RECTS, 4), np.int32)
    vals = np.zeros((1, MAX_RECTS), np.float32)
    for k in range(n):
        r0, c0 = np.random.randint(0, H - minsize), np.random.randint(0, W - minsize)
        dr, dc = np.random.randint(minsize, maxsize), np.random.randint(minsize, maxsize)
        rects[0, k] = (r0, min(r0 + dr, H - 1), c0, min(c0 + dc, W - 1))
        vals[0, k] = np.random.uniform(lo, hi)
    r, v = torch.from_numpy(rects).to(img.device), torch.from_numpy(vals).to(img.device)
    nr = torch.tensor([n], dtype=torch.int32, device=img.device)
    L.spnet_cutout(img.data_ptr(), None, img.data_ptr(), 1, H, W, r.data_ptr(), v.data_ptr(), nr.data_ptr(), _stream())
    torch.cuda.current_stream().synchronize()


def salt_n_pepa_inplace(img, salt_vs_pepper=0.2, amount=0.004):
    """Reference signature (augmentation.py:157); `img` is ONE device frame [H,W,1]."""
    _require_cuda(img)
    sp = draw_saltpepper(tuple(img.shape), salt_vs_pepper, amount)
    if sp is None:
        return
    H, W = img.shape[0], img.shape[1]
    ns, npep = len(sp[0]), len(sp[2])
    coords = np.zeros((1, 2, ns + npep), np.int32)
    coords[0, 0, :ns], coords[0, 1, :ns], coords[0, 0, ns:], coords[0, 1, ns:] = sp
    c = torch.from_numpy(coords).to(img.device)
    flag = torch.ones(1, dtype=torch.int32, device=img.device)
    mm = torch.empty(2 + 32, device=img.device)
    L.spnet_minmax(img.data_ptr(), 1, H * W, mm.data_ptr(), mm[2:].data_ptr(), _stream())
    L.spnet_saltpepper(img.data_ptr(), 1, H, W, c.data_ptr(), ns, npep, flag.data_ptr(), mm.data_ptr(), _stream())
    torch.cuda.current_stream().synchronize()


def blur_inplace(img, blur_prob=0.3, kernel_size=None):
    """Bug-compatible with the reference (augmentation.py:66-70): consumes the RNG, leaves pixels alone."""
    if np.random.random() <= blur_prob:
        _ = kernel_size if kernel_size else random.choice([3, 7])


def _require_cuda(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("spnet_amd.augmentation operates on device tensors (no CPU fallback)")


# ----------------------------------------------------------------------------- offline warps
def _warp(img, minv):
    """img: uint8/float numpy [H,W,C]; minv: 2x3 destination->source map.  Bilinear, zero border."""
    if not torch.cuda.is_available():
        raise RuntimeError("spnet_amd.augmentation warps run on the GPU (no CPU fallback)")
    H, W, C = img.shape
    src = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).cuda()
    dst = torch.empty_like(src)
    m = torch.tensor(np.asarray(minv, np.float32).reshape(1, 6)).cuda()
    L.spnet_warp_affine(src.data_ptr(), dst.data_ptr(), 1, H, W, C, m.data_ptr(), _stream())
    out = dst.cpu().numpy()
    if img.dtype == np.uint8:
        out = np.clip(np.floor(out + 0.5), 0, 255).astype(np.uint8)
    return out


def invert_affine_cv2(M):
    """The inverse of a FORWARD 2x3 matrix as cv2.warpAffine forms it, operation by operation in double precision (OpenCV
    3.4 imgwarp.cpp, warpAffine)."""
    m = np.asarray(M, np.float64).reshape(2, 3).copy()
    D = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = m[1, 1] * D, m[0, 0] * D
    m[0, 0], m[0, 1], m[1, 0], m[1, 1] = A11, m[0, 1] * -D, m[1, 0] * -D, A22
    b1 = -m[0, 0] * m[0, 2] - m[0, 1] * m[1, 2]
    b2 = -m[1, 0] * m[0, 2] - m[1, 1] * m[1, 2]
    m[0, 2], m[1, 2] = b1, b2
    return m


def cv2_fixed_point_terms(M, H, W):
    """Row / column terms of cv2.warpAffine's fixed-point coordinate computation for a FORWARD 2x3 matrix M (OpenCV 3.4
    imgwarp.cpp, warpAffine + WarpAffineInvoker): M is inverted in double precision exactly as OpenCV does it, then
    adelta[x] = cvRound(M00*x*1024), bdelta[x] = cvRound(M10*x*1024), X0[y] = cvRound((M01*y + M02)*1024) + 16,
    Y0[y] = cvRound((M11*y + M12)*1024) + 16 (cvRound = round-half-even = np.rint).  Returns int32 arrays
    xrow [H,2] = (X0, Y0), xcol [W,2] = (adelta, bdelta)."""
    m = invert_affine_cv2(M)
    xs, ys = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    xcol = np.stack([np.rint(m[0, 0] * xs * 1024.0), np.rint(m[1, 0] * xs * 1024.0)], 1).astype(np.int32)
    xrow = np.stack([np.rint((m[0, 1] * ys + m[0, 2]) * 1024.0) + 16, np.rint((m[1, 1] * ys + m[1, 2]) * 1024.0) + 16],
                    1).astype(np.int32)
    return xrow, xcol


def _warp_cv2(img, M):
    """cv2.warpAffine(img, M, (W,H)) for a uint8 image [H,W,C] and a FORWARD matrix: OpenCV's fixed-point algorithm on
    the device (csrc/augment.hip: warp_affine_fixed_kernel)."""
    if not torch.cuda.is_available():
        raise RuntimeError("spnet_amd.augmentation warps run on the GPU (no CPU fallback)")
    H, W, C = img.shape
    xrow, xcol = cv2_fixed_point_terms(M, H, W)
    src = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32)).cuda()
    dst = torch.empty_like(src)
    xr, xc = torch.from_numpy(xrow).cuda(), torch.from_numpy(xcol).cuda()
    L.spnet_warp_affine_fixed(src.data_ptr(), dst.data_ptr(), 1, H, W, C, xr.data_ptr(), xc.data_ptr(), _stream())
    return dst.cpu().numpy().astype(np.uint8)


def _invert_affine(M):
    A = np.vstack([np.asarray(M, np.float64), [0, 0, 1]])
    return np.linalg.inv(A)[:2]


def rotation_matrix_2d(center, angle_deg, scale=1.0):
    """Same matrix as cv2.getRotationMatrix2D (positive angle = counter-clockwise on screen)."""
    a = scale * np.cos(np.deg2rad(angle_deg))
    b = scale * np.sin(np.deg2rad(angle_deg))
    cx, cy = center
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def flip_metadata(metadata, flip_param, width, height):
    """Metadata half of flip_image (augmentation.py:91-104)."""
    new_md = []
    for cx, cy, a, b, angle, rings in metadata:
        if flip_param in (0, -1):
            cy, angle = height - cy, -angle
        angle = cleanup_angle(angle)
        if flip_param in (1, -1):
            cx, angle = width - cx, 180 - angle
        angle = cleanup_angle(angle)
        new_md.append([cx, cy, a, b, angle, rings])
    return new_md


def flip_suffix(flip_param):
    return {0: "_v", 1: "_h"}.get(flip_param, "_vh")


def rotate_metadata(metadata, rot_angle, M):
    """Metadata half of rotate_image (augmentation.py:196-204); M: the forward rotation matrix."""
    new_md = []
    for cx, cy, a, b, angle, rings in metadata:
        angle = cleanup_angle(angle + rot_angle)
        p = M @ np.array([cx, cy, 1.0])
        new_md.append([int(round(p[0])), int(round(p[1])), a, b, angle, rings])
    return new_md


def chain_metadata(metadata, flip, angle, xt, yt, width, height):
    """(rows, file-name suffix) of flip_image -> rotate_image -> translate_image for one frame's rows as Python values (the
    types a CSV written from them shows); translate_image's part applies whenever a shift was drawn, i.e. (xt, yt) is
    given as None, None when its gate was 0."""
    md, suffix = list(metadata), ""
    if flip != -2:
        md, suffix = flip_metadata(md, flip, width, height), flip_suffix(flip)
    if angle != 0:
        md = rotate_metadata(md, angle, rotation_matrix_2d((width / 2, height / 2), angle, 1.0))
        suffix += "_r{:>.2f}".format(angle)
    if xt is not None:
        md = [[cx + xt, cy + yt, a, b, ang, rings] for cx, cy, a, b, ang, rings in md]
        suffix += "_t" + str(xt) + ',' + str(yt)
    return md, suffix


def flip_image(img, metadata, file_prefix, flip_param):
    """flip_param: -2 none, 0 vertical, 1 horizontal, -1 both (augmentation.py:82-112)."""
    if flip_param == -2:
        return img.copy(), list(metadata), file_prefix[:]
    height, width, _ = img.shape
    sx = -1.0 if flip_param in (1, -1) else 1.0
    sy = -1.0 if flip_param in (0, -1) else 1.0
    minv = [[sx, 0, (width - 1) if sx < 0 else 0], [0, sy, (height - 1) if sy < 0 else 0]]
    out = _warp(img, minv)
    return out, flip_metadata(metadata, flip_param, width, height), file_prefix + flip_suffix(flip_param)


def rotate_image(img, metadata, file_prefix, rot_angle, rot_origin=None):
    """Rotate about the centre, bilinear, zero fill; centres mapped through the same 2x3 matrix and
    rounded to int (augmentation.py:184-207)."""
    if rot_angle == 0:
        return img.copy(), list(metadata), file_prefix
    height, width, _ = img.shape
    if rot_origin is None:
        rot_origin = (width / 2, height / 2)
    M = rotation_matrix_2d(rot_origin, rot_angle, 1.0)
    # 8-bit images (the offline set, augment_preproc.py) take OpenCV's fixed-point path like the reference's call does
    out = _warp_cv2(img, M) if img.dtype == np.uint8 else _warp(img, _invert_affine(M))
    return out, rotate_metadata(metadata, rot_angle, M), file_prefix[:] + "_r{:>.2f}".format(rot_angle)


def translate_image(img, metadata, file_prefix, trans_index):
    """Integer shift of up to +-40 px per axis (augmentation.py:216-239)."""
    if trans_index == 0:
        return img.copy(), list(metadata), file_prefix
    trans_max = 40
    xt = int(round(trans_max * (2 * np.random.random() - 1)))
    yt = int(round(trans_max * (2 * np.random.random() - 1)))
    out = _warp_cv2(img, [[1, 0, xt], [0, 1, yt]]) if img.dtype == np.uint8 else _warp(img, [[1, 0, -xt], [0, 1, -yt]])
    new_md = [[cx + xt, cy + yt, a, b, angle, rings] for cx, cy, a, b, angle, rings in metadata]
    return out, new_md, file_prefix[:] + "_t" + str(xt) + ',' + str(yt)


def invert_image(img, metadata, file_prefix):
    return 255 - img, list(metadata), file_prefix + "_i"


# ----------------------------------------------------------------------------- batched warp chain
MAX_OBJECTS = 16                  # ellipses per frame the vectorised metadata path pads to (the data sets hold at most 6)
WARP_RECORD = np.dtype([("m", "<f8", (6,)), ("flip", "<i4"), ("xt", "<i4"), ("yt", "<i4"), ("pad", "<i4")])   # csrc/warp.hip
_IDENTITY_MINV = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])


def draw_warp(H, W):
    """The RNG calls of one pass of augment_one_file (augment_preproc.py:74-86) in its order: np.random.choice of the
    flip code, np.random.uniform(-20, 20) for the angle, np.random.randint(10) for translate_image's gate and, only when
    that is not 0, translate_image's two np.random.random() (spnet/augmentation.py:227-228).  Returns (flip, angle, xt,
    yt); the draws do not depend on the frame size."""
    flip, angle, xt, yt = draw_warp_gated()
    return flip, angle, xt or 0, yt or 0


def draw_warp_gated():
    """draw_warp with xt = yt = None when translate_image's gate was 0 (it then adds no '_t' suffix to the file name)."""
    flip = int(np.random.choice([-2, -1, 0, 1]))
    angle = float(np.random.uniform(-20, high=20))
    xt = yt = None
    if np.random.randint(10) != 0:
        trans_max = 40
        xt = int(round(trans_max * (2 * np.random.random() - 1)))
        yt = int(round(trans_max * (2 * np.random.random() - 1)))
    return flip, angle, xt, yt


def warp_minv(H, W, angle):
    """The six entries of the INVERTED matrix of rotate_image(angle) for an H x W frame, as cv2.warpAffine inverts it; the
    identity for angle == 0 (rotate_image returns the frame as it is)."""
    if angle == 0:
        return _IDENTITY_MINV.copy()
    return invert_affine_cv2(rotation_matrix_2d((W / 2, H / 2), angle, 1.0)).reshape(6)


def new_warp_params(indices, H, W):
    """Identity parameters for the frames `indices`: dict(index, flip, angle, xt, yt, minv [B,6], H, W)."""
    B = len(indices)
    return dict(index=np.asarray(indices, np.int32), flip=np.full(B, -2, np.int32), angle=np.zeros(B, np.float64),
                xt=np.zeros(B, np.int32), yt=np.zeros(B, np.int32), minv=np.tile(_IDENTITY_MINV, (B, 1)), H=int(H), W=int(W))


def set_warp(params, j, flip, angle, xt, yt):
    params["flip"][j], params["angle"][j], params["xt"][j], params["yt"][j] = flip, angle, xt, yt
    params["minv"][j] = warp_minv(params["H"], params["W"], angle)


def warp_chain_host(frames, params):
    """numpy restatement of spnet_warp_chain_u8 (tests, documentation): uint8 frames [n_src,H,W], output j from frame
    params['index'][j].  The single gather: destination (x, y) takes the rotated value at (u, v) = (x - xt, y - yt) or 0
    outside the image, and the four fixed-point bilinear taps of that value read the source through the flip."""
    frames = np.asarray(frames)
    H, W = frames.shape[1:3]
    out = np.zeros((len(params["index"]), H, W), np.uint8)
    for j, i in enumerate(params["index"]):
        m = params["minv"][j]
        flip, xt, yt = int(params["flip"][j]), int(params["xt"][j]), int(params["yt"][j])
        src = frames[min(max(int(i), 0), len(frames) - 1)].astype(np.int64)
        u, v = np.arange(W, dtype=np.float64) - xt, np.arange(H, dtype=np.float64) - yt
        ad, bd = np.rint(m[0] * u * 1024.0).astype(np.int64), np.rint(m[3] * u * 1024.0).astype(np.int64)
        X0 = np.rint((m[1] * v + m[2]) * 1024.0).astype(np.int64) + 16
        Y0 = np.rint((m[4] * v + m[5]) * 1024.0).astype(np.int64) + 16
        X, Y = (X0[:, None] + ad[None, :]) >> 5, (Y0[:, None] + bd[None, :]) >> 5
        sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31

        def at(y, x):
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            yy, xx = np.clip(y, 0, H - 1), np.clip(x, 0, W - 1)
            if flip in (0, -1):
                yy = H - 1 - yy
            if flip in (1, -1):
                xx = W - 1 - xx
            return np.where(ok, src[yy, xx], 0)
        w00 = np.minimum((32 - fy) * (32 - fx) * 32, 32767)
        val = (at(sy, sx) * w00 + at(sy, sx + 1) * ((32 - fy) * fx * 32) + at(sy + 1, sx) * (fy * (32 - fx) * 32) +
               at(sy + 1, sx + 1) * (fy * fx * 32) + (1 << 14)) >> 15
        inside = ((v >= 0) & (v < H))[:, None] & ((u >= 0) & (u < W))[None, :]
        out[j] = np.where(inside, np.clip(val, 0, 255), 0)
    return out


def pad_metadata(meta, max_objects=MAX_OBJECTS):
    """List (one entry per frame) of [cx,cy,a,b,angle,rings] row lists -> (rows float64 [B,max_objects,6] zero padded,
    count int32 [B]).  ValueError when a frame holds more objects."""
    if isinstance(meta, tuple):
        return meta
    B = len(meta)
    rows, count = np.zeros((B, max_objects, 6), np.float64), np.zeros(B, np.int32)
    for j, md in enumerate(meta):
        if len(md) > max_objects:
            raise ValueError("warp metadata: frame %d holds %d objects, at most %d are supported" % (j, len(md), max_objects))
        count[j] = len(md)
        if len(md):
            rows[j, :len(md)] = np.asarray(md, np.float64).reshape(len(md), 6)
    return rows, count


def _cleanup_angle_where(angle, mask):
    """cleanup_angle on the entries `mask` selects, in its add / subtract 180 form (the same roundings as the scalar loop)."""
    angle = angle.copy()
    while True:
        m = mask & (angle < 0)
        if not m.any():
            break
        angle[m] += 180
    while True:
        m = mask & (angle >= 180)
        if not m.any():
            break
        angle[m] -= 180
    return angle


def warp_metadata(meta, params):
    """The metadata arithmetic of flip_image -> rotate_image -> translate_image for a chunk of frames, in float64 with the
    reference's roundings: height - cy / width - cx and the angle reflections with cleanup_angle after each (flip code -2
    leaves the rows alone), angle + rot_angle, centres through the FORWARD rotation matrix and int(round()) (angle 0
    leaves the rows alone), then the integer shift.  meta: a list of row lists or pad_metadata's result for the frames of
    params, in their order.  Returns (rows [B,MAX_OBJECTS,6], count [B]).  The rotated centres are summed as
    (m00 cx + m01 cy) + m02; numpy's own M @ [cx, cy, 1] can differ from that in the last bit, which changes
    a centre only where it falls within one ulp of a half-integer."""
    rows, count = pad_metadata(meta)
    rows = rows.copy()
    H, W = params["H"], params["W"]
    B = rows.shape[0]
    if len(params["flip"]) != B:
        raise ValueError("warp_metadata: %d metadata entries for %d parameter sets" % (B, len(params["flip"])))
    flip = np.asarray(params["flip"])[:, None]
    rot = np.asarray(params["angle"], np.float64)[:, None]
    cx, cy, ang = rows[..., 0], rows[..., 1], rows[..., 4]
    every = np.ones(cx.shape, bool)
    fy, fx, fany = every & ((flip == 0) | (flip == -1)), every & ((flip == 1) | (flip == -1)), every & (flip != -2)
    cy[fy] = (H - cy)[fy]
    ang[fy] = -ang[fy]
    ang[...] = _cleanup_angle_where(ang, fany)
    cx[fx] = (W - cx)[fx]
    ang[fx] = (180 - ang)[fx]
    ang[...] = _cleanup_angle_where(ang, fany)
    rmask = every & (rot != 0)
    if rmask.any():
        M = np.stack([rotation_matrix_2d((W / 2, H / 2), a, 1.0) if a != 0 else np.eye(2, 3) for a in rot[:, 0]])
        ang[...] = _cleanup_angle_where(np.where(rmask, ang + rot, ang), rmask)
        px = M[:, 0, 0, None] * cx + M[:, 0, 1, None] * cy + M[:, 0, 2, None]
        py = M[:, 1, 0, None] * cx + M[:, 1, 1, None] * cy + M[:, 1, 2, None]
        cx[rmask] = np.rint(px)[rmask]
        cy[rmask] = np.rint(py)[rmask]
    cx += np.asarray(params["xt"], np.float64)[:, None]
    cy += np.asarray(params["yt"], np.float64)[:, None]
    rows[np.arange(rows.shape[1])[None, :] >= count[:, None]] = 0.0
    return rows, count


def _encode_targets(rows, count, pred_grid=(6, 6, 2)):
    """parse_meta_file's row processing -> true_to_pred_grid -> norm_Y (spnet/utils.py:260-286, 191-244, 181-184) for a
    chunk, bit-identical to the per-sample path.  Returns (Y float32 [B, prod(grid) * 8], overflow bool [B]): overflow
    marks the frames where a cell would receive more ellipses than it has slots (the reference's AssertionError); their
    rows of Y hold the ellipses that did fit."""
    from . import config as cf
    from . import utils
    pred_shape = np.array([pred_grid[0], pred_grid[1], pred_grid[2], cf.vars_per_pred], dtype=int)
    cx_min, cy_min, _, _, xbin, ybin, gridYi = utils.setup_means_and_ranges(pred_shape)
    nx, ny, ns = int(pred_shape[0]), int(pred_shape[1]), int(pred_shape[2])
    B, K = rows.shape[0], rows.shape[1]
    cx, cy, a, b, ang, rings = (rows[..., k] for k in range(6))
    swap = b > a
    a, b, ang = np.where(swap, b, a), np.where(swap, a, b), np.where(swap, ang + 90, ang)
    keep = (np.arange(K)[None, :] < count[:, None]) & (rings > 0.0)
    t = 2 * np.deg2rad(ang)
    obj = np.stack([cx, cy, a, b, np.cos(t), np.sin(t), np.zeros_like(cx), rings], -1)       # [B,K,8] float64
    order = np.lexsort((cy, cx, ~keep), axis=-1)                   # kept rows first, by (cx, cy), stable
    obj = np.take_along_axis(obj, order[..., None], 1)
    keep = np.take_along_axis(keep, order, 1)
    ix = np.clip(np.trunc((obj[..., 0] - cx_min) / xbin), 0, nx - 1).astype(np.int64)
    iy = np.clip(np.trunc((obj[..., 1] - cy_min) / ybin), 0, ny - 1).astype(np.int64)
    cell = ix * ny + iy
    same = (cell[:, :, None] == cell[:, None, :]) & keep[:, None, :] & (np.arange(K)[None, :] < np.arange(K)[:, None])[None]
    slot = same.sum(-1)                                            # earlier kept ellipses in the same cell
    overflow = (keep & (slot >= ns)).any(1)
    G = np.broadcast_to(gridYi, (B,) + gridYi.shape).copy()
    put = keep & (slot < ns)
    bi = np.broadcast_to(np.arange(B)[:, None], put.shape)
    G[bi[put], ix[put], iy[put], slot[put]] = obj[put].astype(G.dtype)
    return utils.norm_Y(G.reshape(B, -1)), overflow


def warp_targets(meta, params, pred_grid=(6, 6, 2)):
    """Network targets of warped frames: (Y float32 [B,576], rejected bool [B]) = warp_metadata, then the target codec
    vectorised over the chunk and bit-identical to writing the warped rows to a CSV and loading it (parse_meta_file's row
    processing -> true_to_pred_grid -> norm_Y).  On the host in numpy: a few hundred values per frame.

    Where the warp moves a third ellipse into a grid cell -- the reference's codec asserts -- the frame is REJECTED for this
    draw: its entries of `params` are reset to the identity IN PLACE and its row of Y holds its unwarped targets.  No
    redraw is made, so the RNG order is undisturbed.  Centres that the warp moves out of the image are KEPT: the codec
    clips them into the edge cells, exactly as the reference's true_to_pred_grid does (and 4-6 % of the frames have one)."""
    meta = pad_metadata(meta)
    rows, count = warp_metadata(meta, params)
    Y, rejected = _encode_targets(rows, count, pred_grid)
    if rejected.any():
        Y0, bad = _encode_targets(meta[0][rejected], meta[1][rejected], pred_grid)
        assert not bad.any(), UNWARPED_OVERFLOW
        Y[rejected] = Y0
        for j in np.nonzero(rejected)[0]:
            set_warp(params, j, -2, 0.0, 0, 0)
    return Y, rejected


_TRIG_2DEG = {}
UNWARPED_OVERFLOW = "the unwarped metadata itself puts more ellipses into a grid cell than it has slots"


def trig_2deg_table(device=None):
    """(cos, sin) of 2 * deg2rad(k) for the whole degrees k = 0..359 as float32 [360,2], computed in float64 as
    _encode_targets computes them: the table spnet_encode_targets reads for whole-degree angles (fake_espi.trig2_table's
    idiom).  device: a cached device tensor instead of the numpy array."""
    def make():
        t = 2 * np.deg2rad(np.arange(360, dtype=np.float64))
        return np.stack([np.cos(t), np.sin(t)], 1).astype(np.float32)
    return _cached_table(_TRIG_2DEG, make, device)


def warp_fwd(params):
    """float64 [B,8] for spnet_encode_targets: the six entries of the FORWARD rotation_matrix_2d of each frame of params
    (the identity for angle 0, where it is not used), the angle, one unused zero -- the matrices warp_metadata forms."""
    H, W = params["H"], params["W"]
    fwd = np.zeros((len(params["angle"]), 8), np.float64)
    fwd[:, 0] = fwd[:, 4] = 1.0
    for j, a in enumerate(np.asarray(params["angle"], np.float64)):
        if a != 0:
            fwd[j, :6] = rotation_matrix_2d((W / 2, H / 2), a, 1.0).reshape(6)
    fwd[:, 6] = params["angle"]
    return fwd


def encode_targets_device(rows, count, pred_grid=(6, 6, 2), fwd=None, records=None, frame_size=None):
    """_encode_targets on the device (spnet_encode_targets, csrc/targets.hip): rows float64 [B,K,6], count int32 [B] device
    tensors in pad_metadata's layout (K <= MAX_OBJECTS) -> (Y float32 [B, prod(pred_grid) * 8], flags int32 [B]) device
    tensors; flags 0 = fine, 1 = a cell would take more ellipses than it has slots (Y holds those that fit).  Enqueued on
    the current stream, nothing is copied to the host.  Whole-degree angles give the host codec's bits, others are within
    one float32 step on cos / sin.
    fwd (float64 [B,8], see warp_fwd) with records (the B 64-byte records of WARP_RECORD as a device tensor, 8-byte
    aligned) and frame_size = (H, W): warp_targets instead -- the rows are warped first; a frame whose warp overflows a cell
    has its unwarped rows encoded, its record overwritten with the identity IN PLACE and flag 1 (2: its unwarped rows
    overflow as well, where warp_targets asserts)."""
    for t, dt, name in ((rows, torch.float64, "rows"), (count, torch.int32, "count")):
        _require_cuda(t)
        if t.dtype != dt or not t.is_contiguous():
            raise ValueError("encode_targets_device: %s must be a contiguous %s device tensor" % (name, dt))
    if rows.dim() != 3 or rows.shape[2] != 6 or count.shape != (rows.shape[0],):
        raise ValueError("encode_targets_device: rows [B,K,6] and count [B], got %s and %s" % (tuple(rows.shape), tuple(count.shape)))
    if (fwd is None) != (records is None) or (fwd is not None and frame_size is None):
        raise ValueError("encode_targets_device: fwd, records and frame_size go together")
    B, K = int(rows.shape[0]), int(rows.shape[1])
    if fwd is not None:
        if fwd.dtype != torch.float64 or not fwd.is_contiguous() or fwd.numel() != B * 8 or not records.is_contiguous() or \
                records.numel() * records.element_size() != B * WARP_RECORD.itemsize:
            raise ValueError("encode_targets_device: fwd must be contiguous float64 [%d,8] and records %d records of %d bytes"
                             % (B, B, WARP_RECORD.itemsize))
    nx, ny, ns = (int(v) for v in pred_grid)
    H, W = (int(v) for v in frame_size) if frame_size is not None else (0, 0)
    dev = rows.device
    Y = torch.empty((B, nx * ny * ns * 8), dtype=torch.float32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    if B == 0:                           # (empty tensors have no address to pass)
        return Y, flags
    with torch.cuda.device(dev):
        L.spnet_encode_targets(rows.data_ptr(), count.data_ptr(), B, K, nx, ny, ns, H, W, trig_2deg_table(dev).data_ptr(),
                               L.ptr(fwd), L.ptr(records), Y.data_ptr(), flags.data_ptr(), _stream())
    return Y, flags


class DeviceWarper:
    """Keeps pristine full-size uint8 frames [N,H,W] in HBM and their metadata rows on the host -- or, given as a pair of
    device tensors (rows float64 [N,K,6], count int32 [N]), in HBM as well; warps batches of them with one launch
    (csrc/warp.hip) and computes the matching targets on the host, or on the device (csrc/targets.hip).
      draw(indices, seeds=None) -> params (draw_warp per frame; per-frame seeding as DeviceAugmenter.draw)
      draw_device(sample_index, seed, epoch) -> params drawn in HBM (records, fwd, index as device tensors), which
                                   targets_device and apply take as they are: no upload
      targets(params)           -> (Y, rejected), see warp_targets (resets rejected frames' parameters to the identity);
                                   host metadata only: the oracle path
      targets_device(params)    -> (Y, flags) device tensors, see encode_targets_device: params' records are uploaded,
                                   the kernel rewrites those of rejected frames, and the apply(params) that follows
                                   reuses them -- params on the host stay as drawn, and nothing is read back
      apply(params, out_u8=None, out_f=None)   out[j] = warp of frame params['index'][j]
      set_frames(X_u8, rows, count)            new frames and device metadata of the same shapes, copied in place"""

    def __init__(self, X_u8, meta=None, pred_grid=(6, 6, 2)):
        if isinstance(X_u8, np.ndarray):
            if not torch.cuda.is_available():
                raise RuntimeError("DeviceWarper runs on the GPU (no CPU fallback)")
            X_u8 = torch.from_numpy(np.ascontiguousarray(X_u8)).cuda()
        _require_cuda(X_u8)
        if X_u8.dim() == 4 and X_u8.shape[-1] == 1:
            X_u8 = X_u8[..., 0]
        if X_u8.dtype != torch.uint8 or X_u8.dim() != 3:
            raise ValueError("DeviceWarper expects uint8 frames [N,H,W(,1)], got %s %s" % (X_u8.dtype, tuple(X_u8.shape)))
        self.X = X_u8.contiguous()
        self.N, self.H, self.W = (int(v) for v in self.X.shape)
        if not (1 <= self.H <= 2048 and 1 <= self.W <= 2048):
            raise ValueError("DeviceWarper: frames of %d x %d (sizes 1 .. 2048)" % (self.H, self.W))
        self.pred_grid = tuple(pred_grid)
        self.meta = self.meta_dev = None
        if isinstance(meta, tuple) and isinstance(meta[0], torch.Tensor):
            self.meta_dev = self._check_meta_dev(*meta)
        elif meta is not None:
            self.meta = pad_metadata(meta)
            if self.meta[0].shape[0] != self.N:
                raise ValueError("DeviceWarper: %d metadata entries for %d frames" % (self.meta[0].shape[0], self.N))
        self._upload = None
        self._sent = None                   # (params, records, indices) of the last targets_device, for apply

    def _check_meta_dev(self, rows, count):
        if rows.device != self.X.device or count.device != self.X.device or rows.dtype != torch.float64 or \
                count.dtype != torch.int32 or rows.dim() != 3 or tuple(rows.shape[::2]) != (self.N, 6) or \
                not 1 <= rows.shape[1] <= MAX_OBJECTS or tuple(count.shape) != (self.N,):
            raise ValueError("DeviceWarper: device metadata is (rows float64 [%d,K<=%d,6], count int32 [%d]) on %s"
                             % (self.N, MAX_OBJECTS, self.N, self.X.device))
        return rows.contiguous(), count.contiguous()

    def set_frames(self, X_u8, rows, count):
        """Refill for a new epoch, in place: frames uint8 [N,H,W] and device metadata of the shapes this warper holds
        (tensors that ARE its own storage are left as they are).  Enqueued on the current stream."""
        if self.meta_dev is None:
            raise ValueError("DeviceWarper.set_frames: this warper holds host metadata")
        rows, count = self._check_meta_dev(rows, count)
        if X_u8.dtype != torch.uint8 or X_u8.device != self.X.device or X_u8.numel() != self.X.numel() or \
                rows.shape != self.meta_dev[0].shape:
            raise ValueError("DeviceWarper.set_frames: expected uint8 frames %s and rows %s"
                             % (tuple(self.X.shape), tuple(self.meta_dev[0].shape)))
        for dst, src in ((self.X, X_u8.reshape(self.X.shape)), (self.meta_dev[0], rows), (self.meta_dev[1], count)):
            if dst.data_ptr() != src.data_ptr():
                dst.copy_(src)
        self._sent = None

    def new_params(self, indices):
        return new_warp_params(indices, self.H, self.W)

    def draw_into(self, params, j):
        set_warp(params, j, *draw_warp(self.H, self.W))

    def draw(self, indices, seeds=None):
        params = self.new_params(indices)
        saved = (np.random.get_state(), random.getstate()) if seeds is not None else None
        try:
            for j in range(len(indices)):
                if seeds is not None:
                    np.random.seed(int(seeds[j]))
                    random.seed(int(seeds[j]))
                self.draw_into(params, j)
        finally:
            if saved is not None:
                np.random.set_state(saved[0])
                random.setstate(saved[1])
        return params

    def targets(self, params):
        if self.meta is None:
            raise ValueError("DeviceWarper.targets: no metadata was given")
        idx = np.asarray(params["index"], np.int64)
        return warp_targets((self.meta[0][idx], self.meta[1][idx]), params, self.pred_grid)

    def _send(self, params, fwd=None):
        """One host -> device copy: the records (8-byte aligned at the front), fwd (or nothing), then the source indices.
        Returns (records [16 B], fwd [B,8] float64 or None, indices [B]) as views of it."""
        B = len(params["index"])
        rec = np.zeros(B, WARP_RECORD)
        rec["m"], rec["flip"], rec["xt"], rec["yt"] = params["minv"], params["flip"], params["xt"], params["yt"]
        parts = [rec.view(np.int32).reshape(-1)] + ([] if fwd is None else [fwd.view(np.int32).reshape(-1)]) + \
                [np.asarray(params["index"], np.int32)]
        if self._upload is None:
            self._upload = L.AsyncUploader(self.X.device)
        packed = self._upload("warp" if fwd is None else "warp+fwd", np.concatenate(parts))
        self._keep = packed
        nf = 0 if fwd is None else 16 * B
        return packed[:16 * B], (packed[16 * B:16 * B + nf].view(torch.float64).view(B, 8) if nf else None), packed[16 * B + nf:]

    def draw_device(self, sample_index, seed, epoch):
        """The warp parameters of the samples `sample_index` (array-like or an int32 device tensor) drawn ON THE DEVICE
        (spnet_augment_params: flip, a rotation angle quantised to 20/2048 degrees, the shift; a keyed stream of its own,
        see include/spnet_hip.h) -> dict(index, records, fwd, H, W) of device tensors: the records apply() reads and the
        forward matrices targets_device() reads, with the bits warp_minv / warp_fwd give for those angles.  Nothing is
        uploaded or read back.  (With a DeviceAugmenter as well, draw_params_device fills both in one launch.)"""
        return draw_params_device(sample_index, seed, epoch, warper=self)[1]

    @staticmethod
    def _on_device(params):
        return isinstance(params.get("records"), torch.Tensor)

    def targets_device(self, params):
        if self.meta_dev is None:
            raise ValueError("DeviceWarper.targets_device: the metadata must be device tensors (rows, count)")
        if self._on_device(params):         # draw_device's: already in HBM
            rec, fwd, index = params["records"], params["fwd"], params["index"]
        else:
            rec, fwd, index = self._send(params, warp_fwd(params))
        self._sent = (params, rec, index)
        with torch.cuda.device(self.X.device):
            rows, count = self.meta_dev[0].index_select(0, index), self.meta_dev[1].index_select(0, index)
            return encode_targets_device(rows, count, self.pred_grid, fwd, rec, (self.H, self.W))

    def apply(self, params, out_u8=None, out_f=None):
        B = len(params["index"])
        if out_u8 is None and out_f is None:
            raise ValueError("DeviceWarper.apply: no output")
        for o, dt in ((out_u8, torch.uint8), (out_f, torch.float32)):
            if o is not None and (o.dtype != dt or o.device != self.X.device or not o.is_contiguous() or
                                  o.numel() != B * self.H * self.W):
                raise ValueError("DeviceWarper.apply: output must be a contiguous %s device tensor of %d x %d x %d elements"
                                 % (dt, B, self.H, self.W))
        if B == 0:
            return out_u8, out_f
        if self._sent is not None and self._sent[0] is params:      # targets_device's upload, rejected records rewritten
            _, rec, index = self._sent
        elif self._on_device(params):
            rec, index = params["records"], params["index"]
        else:
            rec, _, index = self._send(params)
        self._sent = None
        with torch.cuda.device(self.X.device):
            L.spnet_warp_chain_u8(self.X.data_ptr(), self.N, index.data_ptr(), rec.data_ptr(), B, self.H, self.W,
                                  L.ptr(out_u8), L.ptr(out_f), _stream())
        return out_u8, out_f


# ----------------------------------------------------------------------------- band-pass mix-up
BP_FLIPS = (-1, 0, 1, 2)          # np.random.choice([-1,0,1,2]) of augmentation.py:26; 2 = no flip
BP_DEFAULT_PATH = '/home/shawley/datasets/parsed_zooniverze_steelpan/'    # the reference's default argument
BGR2GRAY = (0.114, 0.587, 0.299)  # cv2.cvtColor(COLOR_BGR2GRAY) weights of B, G, R for float images


def draw_bandpass(n_real):
    """The RNG calls of one bandpass_mixup (augmentation.py:24-27, 51), in its order: random.choice over the sorted file
    list, np.random.choice([-1,0,1,2]), np.random.rand().  Returns (file index, flip code, s = 3 * rand as float32, the
    precision the reference's float32 spectra are scaled in)."""
    i = random.choice(range(n_real))          # consumes what random.choice(files) does: one _randbelow(len)
    flip = int(np.random.choice([-1, 0, 1, 2]))
    s = np.float32(np.random.rand() * 3)
    return i, flip, s


def draw_bandpass_batch(n_real, n, seeds=None):
    """n draws of draw_bandpass.  seeds (optional, one per sample): each sample's draws come from numpy / python streams
    seeded with its own seed; the process-wide RNG states are saved and restored around the draw (DeviceAugmenter.draw).
    Returns dict(real, flip, s, row), row = 4 * real + BP_FLIPS.index(flip): the row of BandpassPool.table."""
    real, flip, s = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    saved = (np.random.get_state(), random.getstate()) if seeds is not None else None
    try:
        for j in range(n):
            if seeds is not None:
                np.random.seed(int(seeds[j]))
                random.seed(int(seeds[j]))
            real[j], flip[j], s[j] = draw_bandpass(n_real)
    finally:
        if saved is not None:
            np.random.set_state(saved[0])
            random.setstate(saved[1])
    row = (4 * real + np.searchsorted(BP_FLIPS, flip)).astype(np.int32)
    return dict(real=real, flip=flip, s=s, row=row)


def bandpass_check_dims(H, W):
    if H < 16 or W < 16:
        raise ValueError("bandpass_mixup: frames must be at least 16 x 16 (the mixed 16 x 16 window of lowest "
                         "frequencies), got %d x %d" % (H, W))


def read_real_frames(path, H, W, device_decode=False, device=None, return_info=False):
    """The sorted *.png files of `path` (the reference's glob order is unspecified) read as greyscale uint8 [R,H,W].
    FileNotFoundError when there are none, ValueError naming the first file of another size.
    device_decode (additive): the frames come back as a uint8 DEVICE tensor.  Grey files (colour type 0, 8 bits: channel 0
    is what convert("L") gives) are decoded on the GPU (spnet_amd.png); every other file -- convert("L") weighs R, G and
    B -- is decoded here as before and uploaded into its place.  return_info: also the sorted indices of the files the
    host decoded (a grey file the kernels reject is among them)."""
    from PIL import Image
    files = sorted(glob.glob(os.path.join(path, '*.png')))
    if not files:
        raise FileNotFoundError("bandpass_mixup: no real *.png images in %r" % path)
    if device_decode:
        from . import png as P
        from .codec_host import map_pool
        if not torch.cuda.is_available():
            raise RuntimeError("bandpass_mixup: device_decode decodes on the GPU (there is no CPU decoder here)")
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        infos = map_pool(P.parse_png_file, files)
        out = torch.empty((len(files), H, W), dtype=torch.uint8, device=device)
        grey = [k for k, i in enumerate(infos) if i.device and i.colour_type == 0]
        host = [k for k in range(len(files)) if k not in set(grey)]
        for k in grey:                  # the size check of the host path, before anything is decoded
            if (infos[k].height, infos[k].width) != (H, W):
                raise ValueError("bandpass_mixup: real image %s is %dx%d, the frames are %dx%d"
                                 % (files[k], infos[k].height, infos[k].width, H, W))
        if grey:
            got, _, fell = P.decode_parsed_png([infos[k] for k in grey], [files[k] for k in grey], device, "first", True)
            out[torch.as_tensor(grey, device=device)] = got
            host = sorted(host + [grey[j] for j in fell])
        for k in (k for k in host if k not in grey):
            with Image.open(files[k]) as im:
                a = np.array(im.convert("L"), dtype=np.uint8)
            if a.shape != (H, W):
                raise ValueError("bandpass_mixup: real image %s is %dx%d, the frames are %dx%d" % (files[k], a.shape[0], a.shape[1], H, W))
            out[k] = torch.from_numpy(a).to(device)
        return (files, out, host) if return_info else (files, out)
    imgs = []
    for f in files:
        with Image.open(f) as im:
            a = np.asarray(im.convert("L"), dtype=np.uint8)
        if a.shape != (H, W):
            raise ValueError("bandpass_mixup: real image %s is %dx%d, the frames are %dx%d" % (f, a.shape[0], a.shape[1], H, W))
        imgs.append(a)
    return files, np.stack(imgs)


class BandpassPool:
    """The real frames of the mix-up on the device, uint8 [R,H,W], and the low-frequency windows of all four flips of
    each, table [R,4,16,16,2] fp32 (flip order BP_FLIPS), computed once.  src: a directory of *.png (sorted) or a uint8
    device tensor [R,H,W].  BandpassPool.get caches directory pools by (realpath, H, W, device).  device_decode (additive,
    directories only): the grey files are decoded on the GPU (read_real_frames): the same frames."""
    _cache = {}

    def __init__(self, src, H, W, device=None, device_decode=False):
        bandpass_check_dims(H, W)
        self.H, self.W = int(H), int(W)
        if isinstance(src, torch.Tensor):
            if src.dtype != torch.uint8 or src.dim() != 3 or tuple(src.shape[1:]) != (H, W) or src.shape[0] < 1:
                raise ValueError("BandpassPool: expected uint8 [R,%d,%d], got %s %s" % (H, W, src.dtype, tuple(src.shape)))
            _require_cuda(src)
            self.files, self.path = None, None
            self.images = src.contiguous()
        else:
            self.path = str(src)
            if not device_decode:
                self.files, host = read_real_frames(self.path, H, W)
            if device is None:
                if not torch.cuda.is_available():
                    raise RuntimeError("BandpassPool: the band-pass mix-up runs on the GPU (no CPU fallback)")
                device = torch.device("cuda", torch.cuda.current_device())
            if device_decode:
                self.files, self.images = read_real_frames(self.path, H, W, device_decode=True, device=device)
            else:
                self.images = torch.from_numpy(host).to(device)
        self.n_real = int(self.images.shape[0])
        dev = self.images.device
        win = torch.empty((len(BP_FLIPS), self.n_real, 16, 16, 2), dtype=torch.float32, device=dev)
        ws = torch.empty(L.spnet_bandpass_ws(self.n_real, H, W), device=dev)
        for fi, code in enumerate(BP_FLIPS):
            flip = torch.full((self.n_real,), code, dtype=torch.int32, device=dev)
            L.spnet_bandpass_project(self.images.data_ptr(), 0, self.n_real, H, W, flip.data_ptr(), win[fi].data_ptr(),
                                     ws.data_ptr(), _stream())
        self.table = win.transpose(0, 1).contiguous()
        torch.cuda.current_stream(dev).synchronize()       # flip / ws are released on return
        self.mixer = BandpassMixer(self)

    @classmethod
    def get(cls, src, H, W, device=None, device_decode=False):
        if isinstance(src, cls):
            return src
        if isinstance(src, torch.Tensor):
            return cls(src, H, W, device)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        key = (os.path.realpath(str(src)), int(H), int(W), str(device))
        pool = cls._cache.get(key)
        if pool is None:
            pool = cls._cache[key] = cls(src, H, W, device, device_decode=device_decode)
        return pool


class BandpassMixer:
    """draw(n, seeds=None) -> parameters (host, reference RNG order); apply(params, frames, ...) mixes frames [n,H,W]
    (or [n,H,W,1]) on the device: one packed upload of the parameters, four launches (csrc/bandpass.hip)."""

    def __init__(self, pool):
        self.pool = pool
        self._upload = None

    def draw(self, n, seeds=None):
        return draw_bandpass_batch(self.pool.n_real, n, seeds)

    def apply(self, params, frames, out_f=None, out_u8=None, units="pixel"):
        """frames: uint8, or float32 in `units` ("pixel" 0..255 | "network" [-1,1]); out_f (float32, same units) and / or
        out_u8 (uint8, round half to even) receive the mixed frames (either may be `frames` itself)."""
        pool = self.pool
        n = len(params["row"])
        if frames.shape[0] != n or frames.numel() != n * pool.H * pool.W:
            raise ValueError("BandpassMixer.apply: frames %s do not hold %d frames of %dx%d" % (tuple(frames.shape), n,
                                                                                           pool.H, pool.W))
        if out_f is None and out_u8 is None:
            raise ValueError("BandpassMixer.apply: no output")
        for o, dt in ((out_f, torch.float32), (out_u8, torch.uint8)):
            if o is not None and (o.dtype != dt or o.numel() != frames.numel() or not o.is_contiguous()):
                raise ValueError("BandpassMixer.apply: output must be contiguous %s of %d elements" % (dt, frames.numel()))
        if not frames.is_contiguous():
            raise ValueError("BandpassMixer.apply: frames must be contiguous")
        if frames.dtype == torch.uint8:
            kind = 0
        elif frames.dtype == torch.float32:
            kind = 2 if units == "network" else 1
        else:
            raise ValueError("BandpassMixer.apply: frames must be uint8 or float32, got %s" % frames.dtype)
        _require_cuda(frames)
        if n == 0:
            return
        dev = frames.device
        if self._upload is None:
            self._upload = L.AsyncUploader(dev)
        packed = self._upload("bp", np.concatenate([np.asarray(params["row"], np.int32),
                                                    np.asarray(params["s"], np.float32).view(np.int32)]))
        row, s = packed[:n], packed[n:].view(torch.float32)
        ws = torch.empty(L.spnet_bandpass_ws(n, pool.H, pool.W), device=dev)
        self._keep = (packed, ws)
        L.spnet_bandpass_apply(frames.data_ptr(), kind, None, n, n, pool.H, pool.W, pool.table.data_ptr(), 4 * pool.n_real,
                               row.data_ptr(), s.data_ptr(), L.ptr(out_f), int(units == "network"), L.ptr(out_u8),
                               ws.data_ptr(), _stream())


def bandpass_mixup(img_in, path_real=BP_DEFAULT_PATH):
    """Reference signature (augmentation.py:10-62): replace the 16 x 16 lowest spatial frequencies of the fake frame
    img_in with those of a random, randomly flipped real frame from path_real scaled by 3 * rand, take the magnitude of
    the inverse transform and min-max normalise it to 0..255 (a constant becomes 0).  Exactly the reference's three RNG
    calls (draw_bandpass).  img_in: numpy array or device tensor, [H,W], [H,W,1] or [H,W,3] (BGR); returns float32 of the
    same kind and shape.

    Fixed reference bugs: the real files are SORTED (glob order is unspecified); [H,W,1] (the generator's own frame
    shape; rows, cols = img_in.shape raised) is accepted and returned as [H,W,1]; [H,W,3] is reduced with cv2's float
    BGR2GRAY weights and the result replicated to 3 channels (the reference's cvCvtColor is a NameError); an empty or
    missing directory raises FileNotFoundError naming it (not IndexError); a real image of another size raises ValueError
    naming the file; frames smaller than 16 x 16 raise ValueError."""
    is_t = isinstance(img_in, torch.Tensor)
    shape = tuple(img_in.shape)
    if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] not in (1, 3)):
        raise ValueError("bandpass_mixup: expected [H,W], [H,W,1] or [H,W,3], got %s" % (shape,))
    H, W = shape[0], shape[1]
    bandpass_check_dims(H, W)
    if is_t:
        _require_cuda(img_in)
        dev = img_in.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("bandpass_mixup runs on the GPU (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    pool = BandpassPool.get(path_real, H, W, dev)
    params = pool.mixer.draw(1)
    x = img_in if is_t else torch.from_numpy(np.ascontiguousarray(img_in)).to(dev)
    if len(shape) == 3 and shape[2] == 3:
        x = x.to(torch.float32)
        x = (x[..., 0] * BGR2GRAY[0] + x[..., 1] * BGR2GRAY[1]) + x[..., 2] * BGR2GRAY[2]
    elif len(shape) == 3:
        x = x[..., 0]
    if x.dtype != torch.uint8:
        x = x.to(torch.float32)
    x = x.contiguous().reshape(1, H, W)
    out = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    pool.mixer.apply(params, x, out_f=out)
    out = out[0]
    if len(shape) == 3:
        out = out[..., None].expand(H, W, shape[2]).contiguous()
    return out if is_t else out.cpu().numpy()
