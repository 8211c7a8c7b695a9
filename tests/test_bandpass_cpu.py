"""Band-pass mix-up, host side: the windowed-DFT formulation against a literal transcription of the reference, the
RNG draws against the reference's three calls, and the documented errors (no GPU needed)."""
import os
import random

import numpy as np
import pytest
from PIL import Image

from tests.helpers import bandpass_ref as R


@pytest.mark.parametrize("H,W", [(384, 512), (331, 331), (97, 130)])
def test_windowed_dft_equals_literal_transcription(H, W):
    rng = np.random.RandomState(H * 7 + W)
    f = rng.randint(0, 256, (H, W)).astype(np.float64)
    t = rng.randint(0, 256, (H, W)).astype(np.float64)
    for flip in R.FLIPS:
        for s in (0.0, 1.7, 2.99):
            a = R.literal(f, t, flip, s)
            b = R.windowed(f, t, flip, s)
            assert a.max() > 254.0 and a.min() < 1.0              # normalised, not degenerate
            err = np.abs(a - b).max() / np.abs(a).max()
            assert err <= 1e-9, (H, W, flip, s, err)


def test_window_excludes_frequency_plus_8():
    """The window holds -8..7 on each axis for even and odd sizes: a pure +8 cosine is left to the fake frame, a pure -8
    one (the same real cosine's other half) is not -- so the mixed spectrum is not Hermitian and the magnitude matters."""
    for H, W in ((64, 64), (65, 67)):
        k = np.arange(-8, 8)
        d = np.fft.fftshift(np.fft.fftfreq(H) * H)[H // 2 - 8:H // 2 + 8]
        assert np.array_equal(np.rint(d), k)
        d = np.fft.fftshift(np.fft.fftfreq(W) * W)[W // 2 - 8:W // 2 + 8]
        assert np.array_equal(np.rint(d), k)
    H, W = 64, 64
    c = np.arange(W)
    f = np.tile(100 + 50 * np.cos(2 * np.pi * 8 * c / W), (H, 1))
    win = R.window(f)
    assert abs(win[8, 0]) > 1e3            # l = -8 inside the window
    # replacing the window with zeros removes the l = -8 half but keeps +8: a complex result
    eh, ew = R._window_mats(H, W)
    y = f - (eh.conj().T @ win @ ew.conj().T) / (H * W)
    assert np.abs(y.imag).max() > 1.0


def test_unscaled_inverse_cancels_in_minmax():
    rng = np.random.RandomState(3)
    f = rng.randint(0, 256, (40, 48)).astype(np.float64)
    t = rng.randint(0, 256, (40, 48)).astype(np.float64)
    a = R.literal(f, t, 1, 1.3)
    # the same pipeline with a scaled inverse
    fs, ts = np.fft.fftshift(np.fft.fft2(f)), np.fft.fftshift(np.fft.fft2(R.cv2_flip(t, 1)))
    mask = np.zeros(f.shape, bool)
    mask[20 - 8:20 + 8, 24 - 8:24 + 8] = True
    y = np.abs(np.fft.ifft2(np.fft.ifftshift(np.where(mask, 1.3 * ts, fs))))
    assert np.abs(np.clip(R.cv2_normalize_minmax(y), 0, 255) - a).max() < 1e-9


def test_draw_matches_reference_rng_calls():
    from spnet_amd import augmentation as A
    files = sorted("real_%03d.png" % i for i in range(17))
    for seed in (0, 5, 123):
        np.random.seed(seed)
        random.seed(seed)
        ref = R.reference_draw(files)
        ref_states = (np.random.get_state(), random.getstate())
        np.random.seed(seed)
        random.seed(seed)
        i, flip, s = A.draw_bandpass(len(files))
        assert (files[i], flip) == ref[:2]
        assert s == np.float32(ref[2]) and s.dtype == np.float32
        np_state, py_state = np.random.get_state(), random.getstate()
        assert py_state == ref_states[1]
        assert np_state[0] == ref_states[0][0] and np.array_equal(np_state[1], ref_states[0][1])
        assert np_state[2:] == ref_states[0][2:]


def test_seeded_batch_draw_is_per_sample_and_restores_global_state():
    from spnet_amd import augmentation as A
    files = sorted("f%d.png" % i for i in range(5))
    np.random.seed(77)
    random.seed(77)
    before = (np.random.get_state(), random.getstate())
    seeds = [11, 12, 13, 14]
    p = A.draw_bandpass_batch(len(files), len(seeds), seeds=seeds)
    after = (np.random.get_state(), random.getstate())
    assert after[1] == before[1] and np.array_equal(after[0][1], before[0][1]) and after[0][2] == before[0][2]
    for j, sd in enumerate(seeds):
        np.random.seed(sd)
        random.seed(sd)
        f, flip, s = R.reference_draw(files)
        assert files[p["real"][j]] == f and p["flip"][j] == flip and p["s"][j] == np.float32(s)
        assert p["row"][j] == 4 * p["real"][j] + R.FLIPS.index(flip)
    # a sample's draw depends on its seed only
    q = A.draw_bandpass_batch(len(files), 2, seeds=seeds[2:])
    assert np.array_equal(q["row"], p["row"][2:]) and np.array_equal(q["s"], p["s"][2:])


def _png(path, a):
    Image.fromarray(np.asarray(a, np.uint8)).save(path)


def test_empty_or_missing_directory_raises_file_not_found(tmp_path):
    from spnet_amd import augmentation as A
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("no images here")
    for d in (empty, tmp_path / "missing"):
        with pytest.raises(FileNotFoundError, match=str(d).replace("\\", "\\\\")):
            A.BandpassPool(str(d), 32, 48)


def test_size_mismatch_raises_value_error_naming_the_file(tmp_path):
    from spnet_amd import augmentation as A
    _png(tmp_path / "a.png", np.zeros((32, 48)))
    _png(tmp_path / "b.png", np.zeros((33, 48)))
    with pytest.raises(ValueError, match="b.png"):
        A.BandpassPool(str(tmp_path), 32, 48)


def test_real_frames_are_read_sorted_as_greyscale(tmp_path):
    from spnet_amd import augmentation as A
    names = ["c.png", "a.png", "b.png"]
    for i, n in enumerate(names):
        rgb = np.zeros((20, 24, 3), np.uint8)
        rgb[..., 0] = 10 * (i + 1)
        Image.fromarray(rgb).save(tmp_path / n)
    files, imgs = A.read_real_frames(str(tmp_path), 20, 24)
    assert [os.path.basename(f) for f in files] == ["a.png", "b.png", "c.png"]
    assert imgs.dtype == np.uint8 and imgs.shape == (3, 20, 24)
    expect = [np.asarray(Image.open(f).convert("L")) for f in files]
    assert all(np.array_equal(a, b) for a, b in zip(imgs, expect))


@pytest.mark.parametrize("H,W", [(15, 64), (64, 15), (8, 8)])
def test_frames_smaller_than_the_window_raise(tmp_path, H, W):
    from spnet_amd import augmentation as A
    _png(tmp_path / "a.png", np.zeros((H, W)))
    with pytest.raises(ValueError, match="16 x 16"):
        A.BandpassPool(str(tmp_path), H, W)
    with pytest.raises(ValueError, match="16 x 16"):
        A.bandpass_mixup(np.zeros((H, W), np.uint8), str(tmp_path))


# ---- the kernel-level helpers of bandpass_ref: the emulation of csrc/bandpass.hip sits within the derived bounds ----------
def _complex(F):
    return np.stack([F.real, F.imag], -1)


def _project_ratio(d, flip, mutant=None):
    """largest |emulate_project - window()| / project_bound over the frames of d [N,H,W] (float32 pixel values)"""
    got = R.emulate_project(d, flip=flip, mutant=mutant).astype(np.float64)
    worst = 0.0
    for n in range(len(d)):
        t = R.cv2_flip(d[n].astype(np.float64), 2 if flip is None else int(flip[n]))
        worst = max(worst, R.ratio(np.abs(got[n] - _complex(R.window(t))), R.project_bound(t)))
    return worst


def _apply_ratio(x, table, row, s, mutant=None, need_finite=True):
    got = R.emulate_apply(x, table, row, s, mutant=mutant).astype(np.float64)
    worst = 0.0
    for n in range(len(x)):
        b = R.apply_bound(x[n], table[row[n]], s[n])
        if need_finite:
            assert np.isfinite(b["bound"]).all()
        if np.isfinite(b["bound"]).all():                         # the bound's reference is mixed()
            assert np.abs(b["ref"] - R.mixed(x[n], table[row[n]], s[n])).max() <= 1e-6
        worst = max(worst, R.ratio(np.abs(got[n] - b["ref"]), b["bound"]))
    return worst


def _impulses(H, W):
    pos = R.edge_positions(H, W)
    return pos, np.stack([R.impulse_frame(H, W, r, c) for r, c in pos])


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_emulated_projection_is_within_project_bound(H, W):
    pos, x = _impulses(H, W)
    for shift, codes in enumerate(([-1, 0, 1, 2, 7], [0, 1, 2, 7, -1], [1, 2, 7, -1, 0])):
        flip = [codes[i % 5] for i in range(len(pos))]
        assert _project_ratio(x, flip) <= 1.0
    for r, c in pos:                                              # one term: a few ulp of A (ulp(200) = 2^-16)
        assert R.project_bound(R.impulse_frame(H, W, r, c)).max() <= 5 * 2.0 ** -16
    assert _project_ratio(R.dense_frames(3, H, W, H + W), [1, -1, 0]) <= 1.0
    assert _project_ratio(R.dense_frames(3, H, W, H + W + 1), None) <= 1.0
    assert np.array_equal(R.emulate_project(np.zeros((1, H, W), np.float32)), np.zeros((1, 16, 16, 2), np.float32))


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_reconstruction_cases_are_well_conditioned_and_emulation_within_recon_bound(H, W):
    table = R.recon_table(H, W)
    x = np.full((3, H, W), 77.0, np.float32)                      # constant: d = 0 and F = 0 exactly
    s = np.ones(3, np.float32)
    G = R.mix_g32(table, s, np.zeros_like(table), H, W)
    got = R.emulate_apply(x, table, np.arange(3), s).astype(np.float64)
    for n in range(3):
        b = R.recon_bound(G[n], np.zeros((H, W)), centred=False)
        assert b["range"] >= 0.25 * b["ymax"], (n, b["range"], b["ymax"])
        assert np.isfinite(b["bound"]).all() and b["bound"].max() < 1e-2
        assert R.ratio(np.abs(got[n] - b["ref"]), b["bound"]) <= 1.0


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_emulated_apply_is_within_the_propagated_bound(H, W):
    pos, x = _impulses(H, W)
    zero = np.zeros((1, 16, 16, 2), np.float32)
    n = len(pos)
    # at 16 x 16 the window is the whole spectrum: y = 0 in exact arithmetic and the bound is infinite (says nothing)
    assert _apply_ratio(x, zero, np.zeros(n, int), np.ones(n, np.float32), need_finite=(H, W) != (16, 16)) <= 1.0
    table = R.dense_table(4, H, W, 5)
    for s in R.S_VALUES:
        assert _apply_ratio(R.dense_frames(3, H, W, 9), table, np.array([3, 0, 2]), np.full(3, s, np.float32),
                            need_finite=(H, W) != (16, 16) or s > 0) <= 1.0


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_wrong_emulations_break_the_bounds_on_the_impulse_cases(H, W):
    """the evidence that the bounds can fail: three one-line bugs, each far outside them wherever its branch is reached"""
    pos, x = _impulses(H, W)
    if W > R.BP_TPB:                                              # a second column tile exists
        assert _project_ratio(x, None, mutant="phase") > 100.0
    else:
        assert _project_ratio(x, None, mutant="phase") <= 1.0
    if H % R.BP_RB:                                               # the last row block is ragged: it reads the next frame's rows
        assert _project_ratio(x, None, mutant="nr") > 100.0
    else:
        assert _project_ratio(x, None, mutant="nr") <= 1.0
    if (H, W) != (16, 16):
        n = len(pos)
        zero = np.zeros((1, 16, 16, 2), np.float32)
        assert _apply_ratio(x, zero, np.zeros(n, int), np.ones(n, np.float32), mutant="sign") > 100.0


def test_pixel_conversion_and_twiddles_of_the_emulation():
    v = R.network_value_of(R.IMPULSE)
    assert v is None or float(R.to_pixel32(v)) == R.IMPULSE
    assert float(R.to_pixel32(np.float32(1.0))) == 255.0 and float(R.to_pixel32(np.float32(-1.0))) == 0.0
    c, s = R.twiddle32(np.arange(8), 8)
    assert c[2] == 0 and c[6] == 0 and s[0] == 0 and s[4] == 0 and c[4] == -1 and s[6] == -1
    assert abs(float(c[1]) - np.sqrt(0.5)) <= 2.0 ** -25
