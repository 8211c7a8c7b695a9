"""Host restatement of spnet_augment_params (csrc/augment_params.hip; the recipe is the comment above its prototype in
include/spnet_hip.h): the same counter RNG in uint32 / uint64 integer arithmetic, the fill in numpy float32 and the shift in
float64 with every operation rounded on its own, and -- for the matrices -- the project's own warp_minv / warp_fwd on the
quantised angle.  Vectorised over the samples (a sample's values depend on its own key only); the band-pass draws, which the
product makes on the host, are restated one sample at a time in Python integers.  No GPU, no library, no threads."""
import numpy as np

from tests.helpers.fake_params_ref import mix, randint

MAX_RECTS = 6
SLOT_FRAME, SLOT_WARP, SLOT_POINTS = 0, 7, 8
ANGLE_MID = 2048
_M32 = 0xFFFFFFFF
_U32 = np.uint64(_M32)
WARP_RECORD = np.dtype([("m", "<f8", (6,)), ("flip", "<i4"), ("xt", "<i4"), ("yt", "<i4"), ("pad", "<i4")])


def draw(key, k):
    """u(key, k) for uint64 arrays (broadcast) or Python ints."""
    if isinstance(key, int) and isinstance(k, int):
        return mix(key ^ ((k * 0x85ebca6b + 0xc2b2ae35) & _M32))
    c = (np.asarray(k, np.uint64) * np.uint64(0x85ebca6b) + np.uint64(0xc2b2ae35)) & _U32
    return mix(np.asarray(key, np.uint64) ^ c)


def sample_key(seed, epoch, index):
    """skey of the samples `index` (any integers; taken modulo 2^32 as the kernel's casts do) -> uint64 array."""
    base = mix(mix((int(seed) & _M32) ^ 0x3c6ef372) + (int(epoch) & _M32))
    idx = np.asarray(index, np.int64).astype(np.uint64) & _U32
    return mix(np.uint64(base) ^ idx)


def slot_key(skey, slot):
    return mix(skey + np.uint64(slot))


def u01_f32(u):
    return (u >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def u01_f64(u):
    return (u >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def angle_of(k):
    return (np.asarray(k, np.float64) - ANGLE_MID) * (20.0 / 2048.0)


def trig_table():
    """[4097][2] float64 = (cos, sin) of np.deg2rad of the quantised angles."""
    rad = np.deg2rad(angle_of(np.arange(2 * ANGLE_MID + 1)))
    return np.stack([np.cos(rad), np.sin(rad)], 1)


def saltpepper_counts(H, W):
    size = H * W
    return int(np.ceil(0.004 * size * 0.2)), int(np.ceil(0.004 * size * (1.0 - 0.2)))


def augment(seed, epoch, index, H, W, mm, points=True):
    """The augmentation half -> dict(rects int32 [B,6,4], vals float32 [B,6], nrect, flag, ksize int32 [B], coords int32
    [B,2,npts] (points=False: left out)).  mm: float32 [N,2] min / max table, row = the sample index clamped."""
    index = np.asarray(index, np.int64)
    B = len(index)
    skey = sample_key(seed, epoch, index)
    k0 = slot_key(skey, SLOT_FRAME)
    nrect = randint(draw(k0, 0), 0, MAX_RECTS).astype(np.int32)
    flag = (draw(k0, 1) >> np.uint64(31)).astype(np.int32)
    blur = (u01_f32(draw(k0, 2)).astype(np.float64) < 0.4) & (u01_f32(draw(k0, 3)).astype(np.float64) <= 0.3)
    ksize = np.where(blur, np.where((draw(k0, 4) >> np.uint64(31)) != 0, 7, 3), 0).astype(np.int32)
    mm = np.asarray(mm, np.float32)
    row = np.clip(index, 0, len(mm) - 1)
    lo, hi = mm[row, 0], mm[row, 1]
    rects, vals = np.zeros((B, MAX_RECTS, 4), np.int32), np.zeros((B, MAX_RECTS), np.float32)
    for r in range(MAX_RECTS):
        kr = slot_key(skey, 1 + r)
        r0, c0 = randint(draw(kr, 0), 0, H - 12), randint(draw(kr, 1), 0, W - 12)
        dr, dc = randint(draw(kr, 2), 11, 74), randint(draw(kr, 3), 11, 74)
        r1, c1 = np.minimum(r0 + dr, H - 1), np.minimum(c0 + dc, W - 1)
        span = hi - lo
        prod = u01_f32(draw(kr, 4)) * span
        fill = lo + prod
        assert span.dtype == prod.dtype == fill.dtype == np.float32
        on = r < nrect
        rects[on, r] = np.stack([r0, r1, c0, c1], 1)[on]
        vals[on, r] = fill[on]
    out = dict(index=index.astype(np.int32), rects=rects, vals=vals, nrect=nrect, flag=flag, ksize=ksize)
    if points:
        n_salt, n_pepper = saltpepper_counts(H, W)
        npts = n_salt + n_pepper
        kp = slot_key(skey, SLOT_POINTS)[:, None]
        p = np.arange(npts, dtype=np.uint64)[None, :]
        rows = randint(draw(kp, 2 * p), 0, H - 2)
        cols = randint(draw(kp, 2 * p + np.uint64(1)), 0, W - 2)
        coords = np.stack([rows, cols], 1).astype(np.int32)
        coords[flag == 0] = 0
        out["coords"] = coords
    return out


def warp(seed, epoch, index, Hw=None, Ww=None):
    """The warp half -> dict(flip, k, gate, xt, yt int32 [B], angle float64 [B]) and, given the full frame size, records
    (WARP_RECORD [B]) and fwd (float64 [B,8]) through the project's warp_minv / warp_fwd."""
    index = np.asarray(index, np.int64)
    kw = slot_key(sample_key(seed, epoch, index), SLOT_WARP)
    flip = (draw(kw, 0) >> np.uint64(30)).astype(np.int32) - 2
    k = randint(draw(kw, 1), 0, 2 * ANGLE_MID).astype(np.int32)
    gate = (randint(draw(kw, 2), 0, 9) != 0).astype(np.int32)
    shift = []
    for d in (3, 4):
        u = u01_f64(draw(kw, d))
        twice = 2.0 * u
        centred = twice - 1.0
        shift.append(np.where(gate != 0, np.rint(40.0 * centred), 0.0).astype(np.int32))
    out = dict(index=index.astype(np.int32), flip=flip, k=k, gate=gate, xt=shift[0], yt=shift[1], angle=angle_of(k))
    if Hw is not None:
        from spnet_amd import augmentation as A
        rec = np.zeros(len(index), WARP_RECORD)
        rec["flip"], rec["xt"], rec["yt"] = flip, shift[0], shift[1]
        for j, a in enumerate(out["angle"]):
            rec["m"][j] = A.warp_minv(Hw, Ww, float(a))
        out["records"] = rec
        out["fwd"] = A.warp_fwd(dict(angle=out["angle"], H=Hw, W=Ww))
    return out


def host_warp_params(ref, Hw, Ww):
    """The restated warp draws as the host path's parameter dict (new_warp_params + set_warp with the quantised angle)."""
    from spnet_amd import augmentation as A
    p = A.new_warp_params(ref["index"], Hw, Ww)
    for j in range(len(ref["index"])):
        A.set_warp(p, j, int(ref["flip"][j]), float(ref["angle"][j]), int(ref["xt"][j]), int(ref["yt"][j]))
    return p


def bandpass_one(seed, epoch, index, n_real, prob):
    """The three band-pass draws of ONE sample in Python integers -> (gate bool, table row int, scale float32)."""
    skey = mix(mix(mix((int(seed) & _M32) ^ 0x3c6ef372) + (int(epoch) & _M32)) ^ (int(index) & _M32))
    k0 = mix(skey + SLOT_FRAME)
    gate = (draw(k0, 5) >> 8) * 2.0 ** -24 < prob
    row = (draw(k0, 6) * max(4 * n_real, 1)) >> 32
    s = np.float32(3) * (np.float32(draw(k0, 7) >> 8) * np.float32(2.0 ** -24))
    return bool(gate), int(row), np.float32(s)
