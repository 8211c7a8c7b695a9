"""spnet_augment_params (csrc/augment_params.hip) bit for bit against its host restatement (tests/helpers/
aug_params_ref.py), its guards, and what is built on it: DeviceAugmenter.draw_device / apply, DeviceWarper.draw_device /
targets_device / apply and callbacks.AugmentOnTheFly(params="device"), single-process and sharded -- each against the
EXISTING host-parameter path handed the restatement's values (the pixel kernels are the same, so equality is exact)."""
import random

import numpy as np
import pytest
import torch

from tests.helpers import aug_params_ref as R

pytestmark = pytest.mark.gpu

SEED, EPOCH = 7, 2 ** 31 + 12345        # a large epoch: the key takes it as uint32
# found with the restatement at (SEED, EPOCH): angle index 2048 (identity), translate gate off, cutout count 0 and 6,
# salt / pepper flag 0 (asserted in _ref below)
K2048, GATE_OFF, COUNT0, COUNT6, FLAG0 = 3599, 6, 3, 2, 0
HEAD = [5, 2, 900001, 70000, K2048, GATE_OFF, COUNT0, COUNT6, FLAG0]      # non-contiguous, beyond 2^16 and the table's end
N_TABLE = 100000                # rows of the min / max table: larger indices clamp to its last row
FULL = (384, 512)               # the warp's full frame size
PAD = 64
HIP_INVALID = 1
_REF = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _indices():
    rest = (np.arange(257 - len(HEAD), dtype=np.int64) * 7919 + 100003) % 1000003
    return np.concatenate([np.asarray(HEAD, np.int64), rest])


def _table():
    rng = np.random.RandomState(11)
    lo = rng.uniform(-1.0, -0.2, N_TABLE).astype(np.float32)
    return np.stack([lo, lo + rng.uniform(0.1, 1.2, N_TABLE).astype(np.float32)], 1)


def _ref(H, W):
    """The restated parameters of the 257 samples, once per frame size (a sample does not depend on its neighbours:
    tests/test_aug_params_cpu.py, so shorter launches are compared with a prefix)."""
    if (H, W) not in _REF:
        idx = _indices()
        a, w = R.augment(SEED, EPOCH, idx, H, W, _table()), R.warp(SEED, EPOCH, idx, *FULL)
        pos = {v: HEAD.index(v) for v in (K2048, GATE_OFF, COUNT0, COUNT6, FLAG0)}
        assert w["k"][pos[K2048]] == 2048 and w["gate"][pos[GATE_OFF]] == 0
        assert a["nrect"][pos[COUNT0]] == 0 and a["nrect"][pos[COUNT6]] == 6 and a["flag"][pos[FLAG0]] == 0
        assert (a["flag"][:5] == 1).any() and (a["ksize"] != 0).any() and (w["gate"][:5] == 1).any()
        _REF[(H, W)] = (a, w)
    return _REF[(H, W)]


def _launch(B, H, W, aug=True, warp=True, seed=SEED, epoch=EPOCH, full=FULL, index=None, raw_kw=None):
    """One raw launch into guarded buffers -> (status, dict of numpy arrays); the guards are checked."""
    from spnet_amd import _lib as L
    from spnet_amd import augmentation as A
    n_salt, n_pepper = R.saltpepper_counts(H, W)
    npts = n_salt + n_pepper
    idx = torch.from_numpy((_indices()[:B] if index is None else np.asarray(index)).astype(np.int32)).cuda()
    mm = torch.from_numpy(_table()).cuda()
    sizes = dict(rects=(B * 24, torch.int32), vals=(B * 6, torch.float32), nrect=(B, torch.int32),
                 coords=(B * 2 * npts, torch.int32), flag=(B, torch.int32), ksize=(B, torch.int32),
                 records=(B * 8, torch.float64), fwd=(B * 8, torch.float64))
    bufs = {k: torch.full((n + PAD,), -7, dtype=dt, device="cuda") for k, (n, dt) in sizes.items()}
    ptr = {k: (v.data_ptr() if (aug if k not in ("records", "fwd") else warp) else None) for k, v in bufs.items()}
    kw = dict(seed=seed, epoch=epoch, sample=idx.data_ptr(), B=B, H=H, W=W, n_salt=n_salt, n_pepper=n_pepper,
              mm=mm.data_ptr(), n_frames=N_TABLE, Hw=full[0], Ww=full[1], trig=A.aug_trig_table("cuda").data_ptr())
    kw.update(ptr)
    kw.update(raw_kw or {})
    rc = L._lib.spnet_augment_params(kw["seed"], kw["epoch"], kw["sample"], kw["B"], kw["H"], kw["W"], kw["n_salt"],
                                     kw["n_pepper"], kw["mm"], kw["n_frames"], kw["rects"], kw["vals"], kw["nrect"],
                                     kw["coords"], kw["flag"], kw["ksize"], kw["Hw"], kw["Ww"], kw["trig"], kw["records"],
                                     kw["fwd"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {}
    for k, (n, _) in sizes.items():
        h = bufs[k].cpu().numpy()
        assert (h[n:] == -7).all(), "the kernel wrote past the end of %s" % k
        out[k] = h[:n]
    return rc, out


def _untouched(out):
    return all((v == -7).all() for v in out.values())


def test_trig_table_is_the_helpers():
    from spnet_amd import augmentation as A
    assert A.aug_trig_table().tobytes() == R.trig_table().tobytes()


@pytest.mark.parametrize("H,W", [(16, 24), (384, 512)])
@pytest.mark.parametrize("B", [1, 5, 64, 257])
def test_kernel_equals_the_restatement(B, H, W):
    _need_gpu()
    a, w = _ref(H, W)
    rc, got = _launch(B, H, W)
    assert rc == 0
    npts = sum(R.saltpepper_counts(H, W))
    assert npts == {(16, 24): 3, (384, 512): 788}[(H, W)]
    for name, shape in (("rects", (B, 6, 4)), ("vals", (B, 6)), ("nrect", (B,)), ("coords", (B, 2, npts)), ("flag", (B,)),
                        ("ksize", (B,))):
        want = a[name][:B]
        assert got[name].dtype == want.dtype
        np.testing.assert_array_equal(got[name].reshape(shape).view(np.int32), want.view(np.int32),
                                      err_msg="%s (bit patterns)" % name)
    # the float64 records and fwd as bytes: the matrices have warp_minv's / warp_fwd's bits
    rec = got["records"].view(R.WARP_RECORD)
    for f in ("flip", "xt", "yt", "pad"):
        np.testing.assert_array_equal(rec[f], w["records"][f][:B], err_msg=f)
    bad = [j for j in range(B) if rec["m"][j].tobytes() != w["records"]["m"][j].tobytes()]
    assert not bad, "inverted matrices differ at batch positions %s, first: %r vs %r" % (
        bad[:5], rec["m"][bad[0]], w["records"]["m"][bad[0]])
    assert rec.tobytes() == w["records"][:B].tobytes()
    bad = [j for j in range(B) if got["fwd"].reshape(B, 8)[j].tobytes() != w["fwd"][j].tobytes()]
    assert not bad, "forward matrices differ at batch positions %s" % bad[:5]


def test_halves_alone_and_guards():
    _need_gpu()
    a, w = _ref(16, 24)
    B = 9
    both = _launch(B, 16, 24)[1]
    rc, only_a = _launch(B, 16, 24, warp=False)
    assert rc == 0 and (only_a["records"] == -7).all() and (only_a["fwd"] == -7).all()
    rc, only_w = _launch(B, 16, 24, aug=False)
    assert rc == 0 and all((only_w[k] == -7).all() for k in ("rects", "vals", "nrect", "coords", "flag", "ksize"))
    for k in ("rects", "vals", "nrect", "coords", "flag", "ksize"):
        np.testing.assert_array_equal(only_a[k], both[k])
    for k in ("records", "fwd"):
        assert only_w[k].tobytes() == both[k].tobytes()
    # a batch in another order and at another launch shape gives every sample the same values
    order = np.array([8, 3, 0, 7, 1])
    rc, perm = _launch(5, 16, 24, index=_indices()[order])
    assert rc == 0
    np.testing.assert_array_equal(perm["rects"].reshape(5, 6, 4), a["rects"][order])
    assert perm["records"].tobytes() == w["records"][order].tobytes()
    # the warp half depends on the full frame size it is given, not on the augmenter's
    rc, small = _launch(5, 16, 24, aug=False, full=(96, 128))
    assert rc == 0 and small["records"].tobytes() == R.warp(SEED, EPOCH, _indices()[:5], 96, 128)["records"].tobytes()
    for raw in (dict(B=-1), dict(sample=None), dict(rects=None, records=None), dict(H=11), dict(W=2049), dict(n_salt=-1),
                dict(n_frames=0), dict(mm=None), dict(vals=None), dict(nrect=None), dict(coords=None), dict(flag=None),
                dict(ksize=None), dict(Hw=0), dict(Ww=2049), dict(trig=None), dict(fwd=None)):
        rc, out = _launch(4, 16, 24, raw_kw=raw)
        assert rc == HIP_INVALID and _untouched(out), raw
    rc, out = _launch(4, 16, 24, raw_kw=dict(B=0))
    assert rc == 0 and _untouched(out)


# ----------------------------------------------------------------------------- what is built on the kernel
N, h, w_ = 8, 16, 24


def _frames(n=N, hh=h, ww=w_, seed=5):
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.uniform(-1, 1, (n, hh, ww, 1)).astype(np.float32)).cuda()


def _host_apply(A, X, ref, real_blur=False, src=None, bp=None, bp_ref=None):
    """The existing host-parameter path: DeviceAugmenter.apply on the restatement's values as host arrays."""
    aug = A.DeviceAugmenter(X.clone(), real_blur=real_blur, bandpass_real=bp, bpmix_prob=0.6)
    p = {k: ref[k] for k in ("index", "rects", "vals", "nrect", "coords", "flag", "ksize")}
    if bp_ref is not None:
        p.update(bp_ref)
    out = torch.empty((len(ref["index"]),) + tuple(X.shape[1:]), device="cuda")
    aug.apply(p, out, src=src)
    torch.cuda.synchronize()
    return out, aug


@pytest.mark.parametrize("real_blur", [False, True])
def test_augment_on_the_fly_device_params(real_blur):
    _need_gpu()
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    X = _frames()
    Y = np.zeros((N, 576), np.float32)
    cb = C.AugmentOnTheFly(X, Y, chunk=3, seed=SEED, real_blur=real_blur, params="device")
    state = np.random.get_state()
    cb.on_epoch_begin(7)
    torch.cuda.synchronize()
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2] == after[2]          # numpy's global stream is not consumed
    ref = R.augment(SEED, 7, np.arange(N), h, w_, cb.augmenter.mm_host)
    assert (ref["nrect"] > 0).any() and (ref["flag"] == 1).any()
    if real_blur:
        assert (ref["ksize"] != 0).any() and (ref["ksize"] == 0).any()
    want, _ = _host_apply(A, X, ref, real_blur=real_blur)
    assert torch.equal(cb.X_aug, want) and not torch.equal(want, X)
    # draw_device / apply directly, indices as a device tensor in another order
    order = torch.tensor([6, 1, 4], dtype=torch.int32, device="cuda")
    p = cb.augmenter.draw_device(order, SEED, 7)
    assert all(isinstance(p[k], torch.Tensor) and p[k].is_cuda for k in ("index", "rects", "vals", "nrect", "coords", "flag", "ksize"))
    out = torch.empty((3, h, w_, 1), device="cuda")
    cb.augmenter.apply(p, out)
    assert torch.equal(out, want[order.long()])
    # another epoch, other frames
    cb.on_epoch_begin(8)
    assert not torch.equal(cb.X_aug, want)


def test_bandpass_draws_from_the_same_keys():
    _need_gpu()
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    X = _frames()
    real = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (3, h, w_)).astype(np.uint8)).cuda()
    pool = A.BandpassPool(real, h, w_)
    cb = C.AugmentOnTheFly(X, np.zeros((N, 576), np.float32), chunk=5, seed=SEED, bandpass_real=pool, bpmix_prob=0.6,
                           params="device")
    cb.on_epoch_begin(2)
    torch.cuda.synchronize()
    ref = R.augment(SEED, 2, np.arange(N), h, w_, cb.augmenter.mm_host)
    draws = [R.bandpass_one(SEED, 2, i, 3, 0.6) for i in range(N)]
    assert any(g for g, _, _ in draws) and not all(g for g, _, _ in draws)
    want = torch.empty_like(X)
    for lo, hi in ((0, 5), (5, 8)):                 # the compacted list is per chunk
        sel = [j - lo for j in range(lo, hi) if draws[j][0]]
        bp = dict(bp_n=len(sel))
        for k, vals, dt in (("bp_sel", sel, np.int32), ("bp_row", [draws[lo + j][1] for j in sel], np.int32),
                            ("bp_s", [draws[lo + j][2] for j in sel], np.float32)):
            arr = np.zeros(hi - lo, dt)
            arr[:len(sel)] = vals
            bp[k] = arr
        sub = {k: v[lo:hi] for k, v in ref.items()}
        want[lo:hi], _ = _host_apply(A, X, sub, bp=pool, bp_ref=bp)
    no_bp, _ = _host_apply(A, X, ref)
    assert torch.equal(cb.X_aug, want) and not torch.equal(want, no_bp)


TRAIN_HW = (64, 96)             # the network-size frames of the warp test (resized from 384 x 512)


def _warp_setup(A):
    """8 full-size frames with device metadata (three or four ellipses each) and the network-size frames of them."""
    from spnet_amd.resize import resize_u8_device
    rng = np.random.RandomState(3)
    U = torch.from_numpy(rng.randint(0, 256, (N,) + FULL).astype(np.uint8)).cuda()
    meta = []
    for f in range(N):
        rows = []
        if f % 2 == 0:              # two ellipses in one grid cell and a third just across its edge: some warps are rejected
            rows += [[60.0 + f, 60.0, 30.0, 15.0, 10.0, 3.0], [90.0, 70.0 + f, 25.0, 12.0, 100.0, 5.0],
                     [118.0 + f, 62.0, 28.0, 14.0, 45.0, 2.0]]
        for _ in range(3 + f % 2 - len(rows)):
            rows.append([float(rng.randint(40, 470)), float(rng.randint(40, 350)), float(rng.randint(20, 60)),
                         float(rng.randint(10, 20)), float(rng.randint(0, 180)), float(rng.randint(1, 11))])
        meta.append(rows)
    rows, count = A.pad_metadata(meta, 7)
    _, overflow = A._encode_targets(rows, count)
    assert not overflow.any()
    X = torch.empty((N,) + TRAIN_HW, device="cuda")
    resize_u8_device(U, TRAIN_HW, out_f=X)
    Y, _ = A._encode_targets(rows, count)
    return U, (torch.from_numpy(rows).cuda(), torch.from_numpy(count).cuda()), X[..., None].contiguous(), Y


def _host_warp_path(A, U, meta_dev, X, index, epoch):
    """The existing path on host parameters built from the restatement -> (X_aug rows, Y rows, flags) of `index`."""
    from spnet_amd.resize import resize_u8_device
    wr = A.DeviceWarper(U, meta_dev)
    aug = A.DeviceAugmenter(X.clone())
    wp = R.host_warp_params(R.warp(SEED, epoch, index), *FULL)
    ref = R.augment(SEED, epoch, index, TRAIN_HW[0], TRAIN_HW[1], aug.mm_host)
    Yw, flags = wr.targets_device(wp)
    full = torch.empty((len(index),) + FULL, dtype=torch.uint8, device="cuda")
    wr.apply(wp, out_u8=full)
    warped = torch.empty((len(index),) + TRAIN_HW, device="cuda")
    resize_u8_device(full, TRAIN_HW, out_f=warped)
    out = torch.empty((len(index),) + TRAIN_HW + (1,), device="cuda")
    aug.apply(ref, out, src=warped)
    torch.cuda.synchronize()
    return out, Yw, flags


def test_warp_source_device_params_and_shards():
    _need_gpu()
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    U, meta_dev, X, Y = _warp_setup(A)
    epoch = 6
    want_X, want_Y, flags = _host_warp_path(A, U, meta_dev, X, np.arange(N), epoch)
    cb = C.AugmentOnTheFly(X, Y, chunk=3, seed=SEED, warp_source=A.DeviceWarper(U, meta_dev), warp_targets="device",
                           params="device")
    cb.on_epoch_begin(epoch)
    torch.cuda.synchronize()
    assert torch.equal(cb.X_aug, want_X) and torch.equal(cb.Y_aug, want_Y)
    assert flags.tolist() == [0, 0, 1, 0, 1, 0, 0, 0]          # (what the host codec rejects at this seed and epoch)
    assert cb.rejected == 2
    assert not torch.equal(cb.Y_aug.cpu(), torch.from_numpy(Y))                 # the targets were warped
    # DeviceWarper.draw_device alone: the records and fwd of the restatement, and the warp of them
    wr = A.DeviceWarper(U, meta_dev)
    wp = wr.draw_device([5, 2], SEED, epoch)
    ref = R.warp(SEED, epoch, [5, 2], *FULL)
    assert wp["records"].cpu().numpy().tobytes() == ref["records"].tobytes()
    assert wp["fwd"].cpu().numpy().tobytes() == ref["fwd"].tobytes()
    # sharded: the rows of a shard are the single-process rows of those samples; the others keep the pristine frames
    shard = np.array([6, 1, 4, 3, 0])
    sh = C.AugmentOnTheFly(X, Y, chunk=2, seed=SEED, warp_source=A.DeviceWarper(U, meta_dev), warp_targets="device",
                           params="device")
    sh._augment_shard(shard, epoch)
    torch.cuda.synchronize()
    rest = np.setdiff1d(np.arange(N), shard)
    assert torch.equal(sh.X_aug[shard], cb.X_aug[shard]) and torch.equal(sh.Y_aug[shard], cb.Y_aug[shard])
    assert torch.equal(sh.X_aug[rest], X[rest]) and torch.equal(sh.Y_aug[rest].cpu(), torch.from_numpy(Y[rest]))
    assert sh.rejected == int((flags[torch.from_numpy(shard).cuda()] != 0).sum())


def test_shard_equals_single_process_without_warp():
    _need_gpu()
    from spnet_amd import callbacks as C
    X = _frames()
    Y = np.zeros((N, 576), np.float32)
    one = C.AugmentOnTheFly(X, Y, chunk=8, seed=3, params="device")
    one.on_epoch_begin(9)
    shard = np.array([7, 2, 5])
    sh = C.AugmentOnTheFly(X, Y, chunk=2, seed=3, params="device")
    sh._augment_shard(shard, 9)
    rest = np.setdiff1d(np.arange(N), shard)
    assert torch.equal(sh.X_aug[shard], one.X_aug[shard]) and torch.equal(sh.X_aug[rest], X[rest])
    assert not torch.equal(one.X_aug[shard], X[shard])


def test_defaults_untouched():
    _need_gpu()
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    X = _frames()
    Y = np.zeros((N, 576), np.float32)
    outs = []
    for kw in (dict(), dict(params="host")):
        cb = C.AugmentOnTheFly(X, Y, chunk=3, seed=1, **kw)
        assert cb.params == "host"
        np.random.seed(1)
        random.seed(1)
        cb.on_epoch_begin(0)
        outs.append(cb.X_aug.clone())
    ref = A.DeviceAugmenter(X.clone())
    want = torch.empty_like(X)
    np.random.seed(1)
    random.seed(1)
    for lo in range(0, N, 3):
        hi = min(N, lo + 3)
        ref.apply(ref.draw(list(range(lo, hi))), want[lo:hi])
    torch.cuda.synchronize()
    assert torch.equal(outs[0], want) and torch.equal(outs[1], want) and not torch.equal(want, X)


def test_train_spnet_passes_the_flag_through(monkeypatch, tmp_path):
    _need_gpu()
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import train_spnet as T
    from spnet_amd import config as cf
    monkeypatch.setattr(cf, "model_type", "monolithic")
    seen = []

    class Reached(Exception):
        pass

    def spy(*a, **kw):
        seen.append(kw)
        raise Reached()
    monkeypatch.setattr(T.models, "setup_model", lambda *a, **kw: (object(), object()))
    monkeypatch.setattr(T.callbacks, "AugmentOnTheFly", spy)
    state = np.random.get_state()
    try:
        for flag, want in ((True, "device"), (False, "host")):
            with pytest.raises(Reached):
                T.train_network(fake_stream=4, fake_val=2, batch_size=4, epochs=1, warp=True, log_dir=str(tmp_path),
                                device_aug_params=flag)
            assert seen[-1]["params"] == want and seen[-1]["warp_targets"] == "device"
    finally:
        np.random.set_state(state)


def test_errors():
    _need_gpu()
    from spnet_amd import callbacks as C
    X = _frames()
    Y = np.zeros((N, 576), np.float32)
    with pytest.raises(ValueError, match="warp_files"):
        C.AugmentOnTheFly(X, Y, warp=True, warp_files=["f%d.png" % i for i in range(N)], params="device")
    with pytest.raises(ValueError, match="params"):
        C.AugmentOnTheFly(X, Y, params="gpu")
