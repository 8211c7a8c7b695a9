"""The sampler of spnet_augment_params as its host restatement states it (tests/helpers/aug_params_ref.py; the recipe is
in include/spnet_hip.h): ranges and clamps, purity in (seed, epoch, sample index), the distributions, and the product's
vectorised band-pass draws against the restatement's per-sample ones.  No GPU, no library."""
import numpy as np
import pytest

from tests.helpers import aug_params_ref as R

SIZES = [(16, 24), (384, 512)]
SEED = 1                        # the distribution bounds below were checked to hold for this seed before it was fixed
N_DIST = 200000
_DIST = {}


def _mm(n, seed=0):
    rng = np.random.RandomState(seed)
    lo = rng.uniform(-1.0, -0.2, n).astype(np.float32)
    return np.stack([lo, lo + rng.uniform(0.1, 1.2, n).astype(np.float32)], 1)


def _dist():
    """The 200,000 samples of SEED, epoch 0, drawn once (no salt / pepper points, no matrices: neither is looked at here)."""
    if not _DIST:
        idx = np.arange(N_DIST)
        _DIST["a"] = R.augment(SEED, 0, idx, 384, 512, _mm(1), points=False)
        _DIST["w"] = R.warp(SEED, 0, idx)
    return _DIST["a"], _DIST["w"]


def _within_5_sigma(counts, probs, n, what):
    counts, probs = np.asarray(counts, np.float64), np.asarray(probs, np.float64)
    assert abs(probs.sum() - 1.0) < 1e-12 or len(probs) == 1
    z = (counts / n - probs) / np.sqrt(probs * (1.0 - probs) / n)
    assert np.abs(z).max() <= 5.0, "%s: frequencies %s, %s binomial standard deviations from %s" % (what, counts / n, z, probs)


@pytest.mark.parametrize("H,W", SIZES)
def test_ranges_and_clamps(H, W):
    n = 400
    idx = np.arange(n) * 977 + 3
    mm = _mm(n * 977 + 4)
    a = R.augment(5, 9, idx, H, W, mm)
    n_salt, n_pepper = R.saltpepper_counts(H, W)
    assert n_salt + n_pepper == {(16, 24): 3, (384, 512): 788}[(H, W)]
    assert a["coords"].shape == (n, 2, n_salt + n_pepper)
    assert a["nrect"].min() == 0 and a["nrect"].max() == 6
    r0, r1, c0, c1 = (a["rects"][..., k] for k in range(4))
    used = np.arange(6)[None, :] < a["nrect"][:, None]
    assert (a["rects"][~used] == 0).all() and (a["vals"][~used] == 0).all()
    assert (r0[used] >= 0).all() and (r0[used] <= H - 12).all() and (c0[used] >= 0).all() and (c0[used] <= W - 12).all()
    dr, dc = (r1 - r0)[used], (c1 - c0)[used]
    assert (r1[used] <= H - 1).all() and (c1[used] <= W - 1).all()
    assert ((dr >= 11) | (r1[used] == H - 1)).all() and (dr <= 74).all()
    assert ((dc >= 11) | (c1[used] == W - 1)).all() and (dc <= 74).all()
    if (H, W) == (16, 24):          # r0 <= 4 and dr >= 11: nearly every rectangle is cut at the last row, most at the last column
        assert (r1[used] == H - 1).mean() > 0.9 and (c1[used] == W - 1).mean() > 0.5 and (c1[used] < W - 1).any()
    else:
        assert (r1[used] == H - 1).any() and (r1[used] < H - 1).any() and dr.max() == 74 and dc.max() == 74
        assert dr.min() <= 11 and dc.min() <= 11
    lo, hi = mm[idx, 0][:, None], mm[idx, 1][:, None]
    assert ((a["vals"] >= lo) & (a["vals"] <= hi))[used].all()
    assert set(np.unique(a["flag"])) == {0, 1} and set(np.unique(a["ksize"])) == {0, 3, 7}
    rows, cols = a["coords"][:, 0], a["coords"][:, 1]
    on = a["flag"] == 1
    assert (a["coords"][~on] == 0).all()
    assert rows[on].min() == 0 and rows[on].max() == H - 2 and cols[on].min() == 0 and cols[on].max() == W - 2
    w = R.warp(5, 9, idx, H, W)
    assert set(np.unique(w["flip"])) == {-2, -1, 0, 1}
    assert w["k"].min() >= 0 and w["k"].max() <= 4096 and np.abs(w["angle"]).max() <= 20.0
    off = w["gate"] == 0
    assert off.any() and (w["xt"][off] == 0).all() and (w["yt"][off] == 0).all()
    assert np.abs(w["xt"]).max() <= 40 and np.abs(w["yt"]).max() <= 40
    assert w["records"]["pad"].max() == 0 and w["fwd"].shape == (n, 8) and (w["fwd"][:, 7] == 0).all()
    np.testing.assert_array_equal(w["fwd"][:, 6], w["angle"])


def test_angle_grid_and_identity():
    assert R.angle_of(2048) == 0.0 and R.angle_of(0) == -20.0 and R.angle_of(4096) == 20.0
    assert R.angle_of(2049) == 20.0 / 2048.0
    t = R.trig_table()
    assert t.shape == (4097, 2) and t.dtype == np.float64 and tuple(t[2048]) == (1.0, 0.0)
    # sample 3599 of (seed 7, epoch 2^31 + 12345) draws index 2048: both matrices are the identity, bit for bit (+0.0)
    w = R.warp(7, 2 ** 31 + 12345, [3599], 384, 512)
    assert w["k"][0] == 2048
    ident = np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    assert w["records"]["m"][0].tobytes() == ident.tobytes() and w["fwd"][0, :6].tobytes() == ident.tobytes()


def test_purity():
    mm = _mm(900002)
    idx = np.array([5, 2, 900001, 70000, 41])
    whole_a, whole_w = R.augment(3, 11, idx, 16, 24, mm), R.warp(3, 11, idx, 384, 512)
    order = np.array([3, 0, 4, 2, 1])
    perm_a, perm_w = R.augment(3, 11, idx[order], 16, 24, mm), R.warp(3, 11, idx[order], 384, 512)
    for k in ("rects", "vals", "nrect", "coords", "flag", "ksize"):
        np.testing.assert_array_equal(perm_a[k], whole_a[k][order], err_msg=k)
    for k in ("flip", "k", "xt", "yt", "records", "fwd"):
        np.testing.assert_array_equal(perm_w[k], whole_w[k][order], err_msg=k)
    for j, i in enumerate(idx):                     # alone
        one_a, one_w = R.augment(3, 11, [i], 16, 24, mm), R.warp(3, 11, [i], 384, 512)
        for k in ("rects", "vals", "nrect", "coords", "flag", "ksize"):
            np.testing.assert_array_equal(one_a[k][0], whole_a[k][j], err_msg=k)
        for k in ("flip", "k", "xt", "yt", "records", "fwd"):
            np.testing.assert_array_equal(one_w[k][0], whole_w[k][j], err_msg=k)
    # another seed, epoch or index: other values (64 samples each; equal draws of all of them would be a broken key)
    base = np.arange(64)
    ref_a, ref_w = R.augment(3, 11, base, 384, 512, mm), R.warp(3, 11, base)
    for seed, epoch, index in ((4, 11, base), (3, 12, base), (3, 11, base + 64), (3 + 2 ** 31, 11, base),
                               (3, 11 + 2 ** 31, base), (3, 11, base + 2 ** 16)):
        a, w = R.augment(seed, epoch, index, 384, 512, mm), R.warp(seed, epoch, index)
        assert not np.array_equal(a["rects"], ref_a["rects"]) and not np.array_equal(a["coords"], ref_a["coords"])
        assert not np.array_equal(w["k"], ref_w["k"]) and not np.array_equal(w["xt"], ref_w["xt"])
        assert (w["k"] != ref_w["k"]).mean() > 0.9


def test_distributions():
    a, w = _dist()
    n = N_DIST
    _within_5_sigma(np.bincount(a["nrect"], minlength=7), [1.0 / 7] * 7, n, "cutout count")
    _within_5_sigma(np.bincount(w["flip"] + 2, minlength=4), [0.25] * 4, n, "flip")
    _within_5_sigma([(a["flag"] == 1).sum(), (a["flag"] == 0).sum()], [0.5, 0.5], n, "salt / pepper gate")
    _within_5_sigma([(w["gate"] == 1).sum(), (w["gate"] == 0).sum()], [0.9, 0.1], n, "translate gate")
    _within_5_sigma([(a["ksize"] == 0).sum(), (a["ksize"] == 3).sum(), (a["ksize"] == 7).sum()], [0.88, 0.06, 0.06], n, "blur")
    on = w["gate"] == 1
    p = np.full(81, 1.0 / 80)
    p[0] = p[80] = 1.0 / 160            # the ends +-40 round from half an interval
    for k in ("xt", "yt"):
        _within_5_sigma(np.bincount(w[k][on] + 40, minlength=81), p, int(on.sum()), k)
    assert np.bincount(w["k"], minlength=4097).min() > 0        # every angle index occurs (48.8 expected of each)


def test_bandpass_draws_vectorised_equal_per_sample():
    from spnet_amd.augmentation import draw_bandpass_keyed
    idx = np.concatenate([np.arange(300), [900001, 70000, 2 ** 31 - 1]])
    for seed, epoch, n_real, prob in ((1, 0, 5, 0.3), (2 ** 32 - 1, 2 ** 31 + 12345, 1, 0.9), (9, 4, 1000, 0.05)):
        gate, row, s = draw_bandpass_keyed(seed, epoch, idx, n_real, prob)
        assert gate.dtype == bool and row.dtype == np.int32 and s.dtype == np.float32
        want = [R.bandpass_one(seed, epoch, int(i), n_real, prob) for i in idx]
        assert gate.tolist() == [g for g, _, _ in want]
        assert row.tolist() == [r for _, r, _ in want]
        assert s.tobytes() == np.array([v for _, _, v in want], np.float32).tobytes()
        assert row.min() >= 0 and row.max() < 4 * n_real and s.min() >= 0 and s.max() < 3
    gate, _, _ = draw_bandpass_keyed(SEED, 0, np.arange(N_DIST), 4, 0.3)
    _within_5_sigma([gate.sum(), (~gate).sum()], [0.3, 0.7], N_DIST, "band-pass gate")
