"""The grid-target codec on the device (spnet_encode_targets, csrc/targets.hip) against the host codec it restates:
augmentation._encode_targets, warp_metadata and warp_targets (themselves pinned to the file path by test_fake_params_cpu.py
and test_warp_chain_cpu.py).  Y bit for bit and the flags equal -- except the cos / sin entries of frames that hold an
angle which is no whole degree: the device's float64 cos / sin and numpy's may differ in their last bits, i.e. after the
cast by at most one float32 step of the value (the division by the range 2 is exact).  Then the surfaces built on it:
FakeStream(targets="device"), DeviceWarper.targets_device, and fresh streamed frames warped afresh every epoch in Model.fit
(FreshFakeESPI(warper=True) + AugmentOnTheFly(warp_source=...))."""
import copy
import functools
import os
import random
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID = 1          # hipErrorInvalidValue
GRIDS = [(6, 6, 2), (4, 3, 3)]
TRAIN_HW = (64, 96)      # the smallest frames the stream tests run the engine at (tests/test_fake_params_gpu.py)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _hand_frames():
    """Every case the codec distinguishes, at most 7 rows each (rows = cx, cy, a, b, angle, rings)."""
    e6 = [(40 + 71 * k, 40 + 51 * k, 30, 20, 15, 2) for k in (0, 2, 3, 6)]          # on the cell edges of the 6 x 6 grid
    e4 = [(40 + 107 * k, 40 + 103 * k, 30, 20, 15, 2) for k in (0, 1, 3, 4)]        # ... of the 4 x 3 grid
    return [
        [],                                                                         # count 0: the blank grid
        [(100, 100, 20, 50, 30, 3)],                                                # b > a: swap, + 90
        [(100, 100, 50, 20, 30, 0), (300, 200, 40, 30, 45, 2), (310, 210, 40, 30, 45, -1)],     # rings <= 0 are dropped
        [(200, 120, 30, 20, 10, 1), (200, 110, 31, 21, 20, 2), (90, 300, 32, 22, 30, 3)],       # equal cx: by cy
        [(150, 150, 30, 20, 10, 1), (150, 150, 40, 25, 20, 2), (350, 250, 20, 50, 30, 3)],      # identical: original order
        e6, e4,
        [(10, 20, 30, 20, 15, 2), (500, 370, 30, 20, 15, 2), (-50, 400, 30, 20, 15, 2), (1e30, -1e30, 30, 20, 15, 2),
         (float("inf"), float("-inf"), 30, 20, 15, 2)],                             # left of 40, beyond 470 / 350: the clip
        [(130, 120, 30, 20, 15, 4), (120, 100, 31, 20, 15, 1), (125, 110, 32, 20, 15, 3), (121, 130, 33, 20, 15, 2),
         (122, 95, 34, 20, 15, 5)],                                                 # five in one cell of either grid: flag 1
        [(60, 60, 30, 20, 0, 1), (160, 60, 30, 20, 90, 2), (260, 60, 30, 20, 179, 3), (360, 60, 30, 20, 180, 4),
         (60, 260, 30, 20, 270, 5), (160, 260, 20, 30, 269, 6), (260, 260, 30, 20, 359, 7)],    # whole degrees (269 + 90 = 359)
        [(60, 60, 30, 20, 12.5, 1), (160, 60, 30, 20, 179.999, 2), (260, 60, 30, 20, -33.3, 3), (360, 60, 20, 30, 400.25, 4),
         (60, 260, 30, 20, 1e-9, 5), (160, 260, 30, 20, 44.99999999999999, 6),
         (260, 260, 20, 30, 270, 7)],                                               # no whole degrees (270 + 90 leaves the table)
    ]


def _random_frames(n, seed, whole=None):
    """0..6 ellipses per frame on a coarse lattice (equal centres and full cells happen); a frame's angles are all whole
    degrees or none is (whole: None = alternate)."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        w = (i % 2 == 0) if whole is None else whole
        rows = []
        for _ in range(rs.randint(0, 7)):
            ang = float(rs.randint(0, 180)) if w else float(rs.uniform(0, 180))
            rows.append((float(rs.randint(0, 52) * 10), float(rs.randint(0, 39) * 10), float(rs.randint(10, 90)),
                         float(rs.randint(10, 90)), ang, float(rs.randint(0, 12))))
        out.append(rows)
    return out


@functools.lru_cache(maxsize=None)
def _codec_case(K):
    """(rows [65,K,6], count [65]) with count beyond K and below 0 among them, and per grid the host codec's (Y, overflow)."""
    from spnet_amd import augmentation as A
    frames = _hand_frames() + _random_frames(65 - len(_hand_frames()), 5)
    rows, count = A.pad_metadata(frames, K)
    count = count.copy()
    rows[-1, :] = rows[8, :]             # a full row set under a count past K, and a negative count over real rows
    count[-1], count[-2] = 99, -3
    want = {g: A._encode_targets(rows, count, g) for g in GRIDS}
    for v in want.values():
        for a in v:
            a.setflags(write=False)
    rows.setflags(write=False)
    count.setflags(write=False)
    return rows, count, want


def _whole_frames(rows, count):
    """bool [B]: every angle the codec sees in the frame (after the b > a swap's + 90) is a whole degree in [0, 360)."""
    K = rows.shape[1]
    ang = np.where(rows[..., 3] > rows[..., 2], rows[..., 4] + 90, rows[..., 4])
    ok = (ang >= 0) & (ang < 360) & (ang == np.trunc(ang))
    return (ok | (np.arange(K)[None, :] >= count[:, None])).all(1)


def _check_Y(got, want, whole, what=""):
    """Bit for bit, but for the cos / sin entries of the frames that are not `whole`: one float32 step or 1e-15 there."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == np.float32 and want.dtype == np.float32
    B = got.shape[0]
    loose = np.zeros(got.shape, bool).reshape(B, -1, 8)
    loose[~whole, :, 4:6] = True
    loose = loose.reshape(got.shape)
    same = got.view(np.int32) == want.view(np.int32)
    bad = np.argwhere(~same & ~loose)
    assert bad.size == 0, "%s: %d entries differ in their bits, first (frame, entry) %s: %r != %r" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    where = np.argwhere(loose)
    g, w = got[loose].astype(np.float64), want[loose]
    tol = np.maximum(np.spacing(np.abs(w)).astype(np.float64), 1e-15)
    over = where[~(np.abs(g - w.astype(np.float64)) <= tol)]
    assert len(over) == 0, "%s: cos / sin off by more than one float32 step, first (frame, entry) %s: %r != %r" % (
        what, over[0], got[tuple(over[0])], want[tuple(over[0])])


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("K", [7, 16])
@pytest.mark.parametrize("B", [1, 2, 65])
def test_codec_equals_encode_targets(B, K, grid):
    _need_gpu()
    from spnet_amd import augmentation as A
    rows, count, want = _codec_case(K)
    Yw, overflow = want[grid]
    lo = 0 if B == 65 else 7             # B = 1, 2 start at the clip frame (the flagged frame is its neighbour)
    r, c = torch.from_numpy(rows[lo:lo + B].copy()).cuda(), torch.from_numpy(count[lo:lo + B].copy()).cuda()
    Y, flags = A.encode_targets_device(r, c, grid)
    assert Y.shape == (B, int(np.prod(grid)) * 8) and Y.dtype == torch.float32 and flags.dtype == torch.int32
    np.testing.assert_array_equal(flags.cpu().numpy(), overflow[lo:lo + B].astype(np.int32))
    _check_Y(Y.cpu().numpy(), Yw[lo:lo + B], _whole_frames(rows, np.clip(count, 0, K))[lo:lo + B], "K %d grid %s" % (K, grid))
    if B == 65:                          # what the frames were built for
        assert overflow[8] and overflow[-1] and not overflow[:8].any() and not _whole_frames(rows, count)[10]
        blank = A._encode_targets(rows[:1], count[:1], grid)[0]
        np.testing.assert_array_equal(Y[0].cpu().numpy(), blank[0])
        np.testing.assert_array_equal(Y[-2].cpu().numpy(), blank[0])      # count -3
    # B == 0: empty results
    Y0, f0 = A.encode_targets_device(r[:0].contiguous(), c[:0].contiguous(), grid)
    assert Y0.shape == (0, Y.shape[1]) and f0.shape == (0,)


def _record_array(A, params):
    rec = np.zeros(len(params["index"]), A.WARP_RECORD)
    rec["m"], rec["flip"], rec["xt"], rec["yt"] = params["minv"], params["flip"], params["xt"], params["yt"]
    return rec


def _sub_params(p, sel):
    return {k: (v[sel].copy() if isinstance(v, np.ndarray) else v) for k, v in p.items()}


@functools.lru_cache(maxsize=None)
def _warp_case():
    """64 frames of random metadata, their drawn parameters (every flip code, angle 0 and not, shifts 0 and +-40) and what
    warp_targets makes of them: (meta, params as drawn, params as warp_targets left them, Y, rejected, the encoded rows)."""
    from spnet_amd import augmentation as A
    H, W, n = 384, 512, 64
    frames = _random_frames(n, 11, whole=True)
    # two ellipses in cell (1, 1) of the 6 x 6 grid and a third that a shift of +40 moves in from cell (0, 1): rejected
    frames[5] = [(120.0, 100.0, 30.0, 20.0, 10.0, 1.0), (130.0, 110.0, 30.0, 20.0, 20.0, 2.0), (100.0, 100.0, 30.0, 20.0, 30.0, 3.0)]
    # ... and two in cell (4, 1) with a third in cell (5, 1) that the horizontal flip maps into cell (1, 1) together
    frames[9] = [(335.0, 100.0, 30.0, 20.0, 10.0, 1.0), (340.0, 110.0, 30.0, 20.0, 20.0, 2.0), (398.0, 100.0, 30.0, 20.0, 30.0, 3.0)]
    rs = np.random.RandomState(3)
    p = A.new_warp_params(list(range(n)), H, W)
    shifts = [0, 40, -40]
    for j in range(n):
        angle = 0.0 if j % 3 == 0 else float(rs.uniform(-20, 20))
        A.set_warp(p, j, [-2, -1, 0, 1][j % 4], angle, shifts[(j // 2) % 3], shifts[(j // 5) % 3])
    A.set_warp(p, 5, -2, 0.0, 40, 0)
    A.set_warp(p, 9, 1, 0.0, 0, 0)
    meta = A.pad_metadata(frames)
    drawn = copy.deepcopy(p)
    Y, rejected = A.warp_targets(meta, p)
    rows_enc, _ = A.warp_metadata(meta, p)                # rejected frames are at the identity now: their unwarped rows
    return meta, drawn, p, Y, rejected, rows_enc


def test_codec_with_warp_equals_warp_targets():
    _need_gpu()
    from spnet_amd import augmentation as A
    meta, drawn, after, Yw, rejected, rows_enc = _warp_case()
    assert rejected[5] and rejected[9] and 0 < rejected.sum() < len(rejected)
    assert set(drawn["flip"]) == {-2, -1, 0, 1} and (drawn["angle"] == 0).any() and (drawn["angle"] != 0).any()
    assert {0, 40, -40} <= set(drawn["xt"]) and {0, 40, -40} <= set(drawn["yt"])
    whole = _whole_frames(rows_enc, meta[1])
    assert whole.any() and not whole.all()
    n, H, W = len(rejected), drawn["H"], drawn["W"]
    rows, count = torch.from_numpy(meta[0]).cuda(), torch.from_numpy(meta[1]).cuda()
    # the entry point itself
    rec = torch.from_numpy(_record_array(A, drawn).view(np.int32).reshape(-1).copy()).cuda()
    fwd = torch.from_numpy(A.warp_fwd(drawn)).cuda()
    Y, flags = A.encode_targets_device(rows, count, (6, 6, 2), fwd, rec, (H, W))
    np.testing.assert_array_equal(flags.cpu().numpy(), rejected.astype(np.int32))
    _check_Y(Y.cpu().numpy(), Yw, whole, "warped")
    got = rec.cpu().numpy().view(A.WARP_RECORD)
    want = _record_array(A, after)       # rejected frames: the identity record; every other record untouched
    assert got.tobytes() == want.tobytes() and (want["flip"][rejected] == -2).all()
    # through DeviceWarper, frames picked in another order; apply() then warps with the rewritten records
    X = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda")
    wr = A.DeviceWarper(X, (rows, count))
    order = np.random.RandomState(1).permutation(n)
    p = _sub_params(drawn, order)
    before = copy.deepcopy(p)
    Y2, flags2 = wr.targets_device(p)
    np.testing.assert_array_equal(flags2.cpu().numpy(), rejected[order].astype(np.int32))
    _check_Y(Y2.cpu().numpy(), Yw[order], whole[order], "DeviceWarper")
    out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    wr.apply(p, out_u8=out)
    assert all(np.array_equal(p[k], before[k]) for k in ("flip", "angle", "xt", "yt", "minv"))    # the host's copy stays as drawn
    look = np.concatenate([np.nonzero(rejected[order])[0][:2], np.nonzero(~rejected[order])[0][:2]])
    ref = A.warp_chain_host(X.cpu().numpy(), _sub_params(_sub_params(after, order), look))
    np.testing.assert_array_equal(out[torch.from_numpy(look).cuda()].cpu().numpy(), ref)
    for j in np.nonzero(rejected[order])[0][:2]:          # a rejected frame is copied
        assert torch.equal(out[j], X[order[j]])
    with pytest.raises(ValueError):
        A.DeviceWarper(X, (rows, count)).targets(p)       # the host path needs host metadata
    with pytest.raises(ValueError):
        A.DeviceWarper(X[:2], [[], []]).targets_device(_sub_params(drawn, np.arange(2)))


def test_unwarped_overflow_is_flag_2():
    _need_gpu()
    from spnet_amd import augmentation as A
    frames = [[(120.0, 100.0, 30.0, 20.0, 10.0, 1.0), (130.0, 110.0, 30.0, 20.0, 20.0, 2.0), (125.0, 105.0, 30.0, 20.0, 30.0, 3.0)]]
    meta = A.pad_metadata(frames)
    p = A.new_warp_params([0], 384, 512)
    A.set_warp(p, 0, -2, 0.0, 5, 5)                       # the three stay in one cell, warped or not
    rec = torch.from_numpy(_record_array(A, p).view(np.int32).reshape(-1).copy()).cuda()
    Y, flags = A.encode_targets_device(torch.from_numpy(meta[0]).cuda(), torch.from_numpy(meta[1]).cuda(), (6, 6, 2),
                                       torch.from_numpy(A.warp_fwd(p)).cuda(), rec, (384, 512))
    assert flags.tolist() == [2]
    Yw, overflow = A._encode_targets(meta[0], meta[1])
    assert overflow.all()
    np.testing.assert_array_equal(Y.cpu().numpy(), Yw)    # the unwarped rows that fit
    assert rec.cpu().numpy().view(A.WARP_RECORD).tobytes() == _record_array(A, A.new_warp_params([0], 384, 512)).tobytes()
    with pytest.raises(AssertionError):
        A.warp_targets(meta, p)


def test_argument_errors_write_nothing():
    _need_gpu()
    from spnet_amd import _lib as L
    from spnet_amd import augmentation as A
    B = 3
    rows = torch.zeros((B, 17, 6), dtype=torch.float64, device="cuda")
    count = torch.ones(B, dtype=torch.int32, device="cuda")
    fwd = torch.zeros((B, 8), dtype=torch.float64, device="cuda")
    rec = torch.zeros(B * 16, dtype=torch.int32, device="cuda")
    trig = A.trig_2deg_table("cuda")
    Y = torch.full((B, 576), 7.0, dtype=torch.float32, device="cuda")
    flags = torch.full((B,), 9, dtype=torch.int32, device="cuda")

    def call(K=7, nx=6, fwd_=None, rec_=None, Y_=Y, count_=count, B=B):
        L.spnet_encode_targets(rows.data_ptr(), L.ptr(count_), B, K, nx, 6, 2, 384, 512, trig.data_ptr(), L.ptr(fwd_), L.ptr(rec_),
                               L.ptr(Y_), flags.data_ptr(), L.current_stream())
    for kw in (dict(K=0), dict(K=17), dict(fwd_=fwd), dict(rec_=rec), dict(Y_=None), dict(count_=None), dict(nx=0)):
        with pytest.raises(L.HipError, match="hipError_t %d$" % HIP_INVALID):
            call(**kw)
    call(B=0)                                              # success, nothing launched
    torch.cuda.synchronize()
    assert (Y == 7.0).all() and (flags == 9).all()
    call(fwd_=fwd, rec_=rec)                               # the same arguments, complete: runs
    torch.cuda.synchronize()
    assert (flags == 0).all() and not (Y == 7.0).any()
    with pytest.raises(ValueError):
        A.encode_targets_device(rows[:, :7].contiguous(), count, fwd=fwd)
    with pytest.raises(ValueError):
        A.encode_targets_device(rows[:, :7].contiguous().float(), count)


def test_fake_stream_device_targets_equal_host():
    _need_gpu()
    from spnet_amd import fake_espi as F
    n = 65
    dev, host = (F.FakeStream(n, seed=21, size=TRAIN_HW, chunk=32, targets=t) for t in ("device", "host"))
    assert F.FakeStream(n).targets == "device"
    for e in (0, 3):
        Xd, Yd = dev.epoch(e, verbose=False, keep_u8=(e == 3))
        Xh, Yh = host.epoch(e, verbose=False)
        assert torch.equal(Xd, Xh) and torch.equal(Yd, Yh) and dev.overflowed == host.overflowed
    # keep_u8: the frames at their full size and the label rows, on the device
    _, labels, U = F.generate_device(n, seed=21, params="device", first_frame=3 * n, want_u8=True, chunk=32)
    assert torch.equal(dev.U_full, U)
    from spnet_amd.augmentation import pad_metadata
    rows, count = pad_metadata(labels, 7)
    np.testing.assert_array_equal(dev.rows.cpu().numpy(), rows)
    np.testing.assert_array_equal(dev.count.cpu().numpy(), count)
    with pytest.raises(ValueError):
        host.epoch(0, verbose=False, keep_u8=True)
    with pytest.raises(ValueError):
        F.FakeStream(n, targets="gpu")


def test_streamed_frames_warped_in_fit(monkeypatch, capsys):
    _need_gpu()
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    monkeypatch.setattr(cf, "model_type", "monolithic")
    n = 8
    stream = F.FakeStream(n, seed=13, size=TRAIN_HW)
    fresh = C.FreshFakeESPI(None, None, stream, warper=True)
    assert fresh.warper.X.data_ptr() == stream.U_full.data_ptr() and (fresh.warper.H, fresh.warper.W) == (384, 512)
    with pytest.raises(ValueError):
        C.AugmentOnTheFly(fresh.X, fresh.Y, warp_source=fresh.warper)                  # needs warp_targets="device"
    with pytest.raises(ValueError):
        C.AugmentOnTheFly(fresh.X, fresh.Y, warp_targets="device")
    aug = C.AugmentOnTheFly(fresh.X, fresh.Y, chunk=n, seed=1, warp_source=fresh.warper, warp_targets="device")
    np.random.seed(3)
    random.seed(3)
    model = M.Model(TRAIN_HW + (1,), Y0size=576, seed=5)
    hist = model.fit(fresh.X, fresh.Y, batch_size=4, epochs=1, shuffle=False, verbose=0, callbacks=[fresh, aug])
    assert len(hist["loss"]) == 1 and np.isfinite(hist["loss"][0])
    assert model._train_frames[1] is aug.X_aug and model._train_targets[1] is aug.Y_aug and fresh.epochs_filled == [0]
    assert "warps rejected" in capsys.readouterr().out
    # the oracle: the stream's own labels and full-size frames of epoch 0 under the parameters that were drawn
    _, labels, U = F.generate_device(n, seed=13, params="device", first_frame=0, want_u8=True)
    assert torch.equal(fresh.warper.X, U)
    wp = copy.deepcopy(aug.last_warp)
    assert (wp["angle"] != 0).all() and list(wp["index"]) == list(range(n))
    meta = A.pad_metadata(labels)
    Yw, rejected = A.warp_targets(meta, wp)
    rows_enc, _ = A.warp_metadata(meta, wp)
    _check_Y(aug.Y_aug.cpu().numpy(), Yw, _whole_frames(rows_enc, meta[1]), "Y_aug")
    assert aug.rejected == int(rejected.sum())
    assert not torch.equal(aug.Y_aug, fresh.Y_dev)
    np.testing.assert_array_equal(aug.last_full.cpu().numpy(), A.warp_chain_host(U.cpu().numpy(), wp))


def test_train_spnet_accepts_fake_stream_with_warp(monkeypatch, tmp_path):
    _need_gpu()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import train_spnet as T
    from spnet_amd import augmentation as A
    from spnet_amd import config as cf
    monkeypatch.setattr(cf, "model_type", "monolithic")
    seen = {}
    real = T.fake_stream_data

    def spy(*a, **kw):
        seen["data"] = real(*a, **kw)
        return seen["data"]

    class Reached(Exception):
        pass

    def stop(*a, **kw):
        raise Reached()
    monkeypatch.setattr(T, "fake_stream_data", spy)
    monkeypatch.setattr(T.models, "setup_model", stop)
    state = np.random.get_state()
    try:
        with pytest.raises(Reached):                      # past the argument checks, at the model set-up
            T.train_network(fake_stream=4, fake_val=2, batch_size=4, epochs=1, warp=True, log_dir=str(tmp_path))
        fresh = seen["data"][4]
        assert isinstance(fresh.warper, A.DeviceWarper) and fresh.warper.N == 4 and fresh.warper.meta_dev is not None
        with pytest.raises(Reached):
            T.train_network(fake_stream=4, fake_val=2, batch_size=4, epochs=1, warp=True, noaugment=True, log_dir=str(tmp_path))
        assert seen["data"][4].warper is None
    finally:
        np.random.set_state(state)
