"""Band-pass mix-up on the MI355X (csrc/bandpass.hip) against the float64 restatement of the reference
(tests/helpers/bandpass_ref.py), and its three users: bandpass_mixup, the fake-ESPI generator and the on-the-fly
augmentation.

Tolerance: 4 x the error of a float32 scipy.fft run of the same pipeline against float64, floored at 1e-3 grey levels,
measured per case.  (Measured on an MI355X, 384x512 and 331x331: see the figures printed by
test_bandpass_mixup_matches_float64_reference.)"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from tests.helpers import bandpass_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def real_dir(path, H, W, n=3, seed=0):
    """n 'real' frames: low-frequency fringes plus noise, written as greyscale PNGs; returns (dir, uint8 [n,H,W])."""
    rng = np.random.RandomState(seed)
    os.makedirs(path, exist_ok=True)
    r, c = np.mgrid[0:H, 0:W]
    imgs = []
    for i in range(n):
        a = 110 + 60 * np.cos(2 * np.pi * (rng.uniform(1, 4) * r / H + rng.uniform(1, 4) * c / W)) + rng.normal(0, 20, (H, W))
        a = np.clip(np.rint(a), 0, 255).astype(np.uint8)
        Image.fromarray(a).save(os.path.join(path, "real_%02d.png" % (n - i)))       # written out of order
        imgs.append(a)
    return str(path), np.stack(imgs[::-1])


def fake_frame(H, W, seed):
    rng = np.random.RandomState(seed)
    r, c = np.mgrid[0:H, 0:W]
    a = 128 + 80 * np.sin(r / 7.0 + c / 11.0) + rng.normal(40, 40, (H, W))
    a = np.clip(np.rint(a), 0, 255) * rng.randint(0, 2, (H, W))
    return a.astype(np.uint8)


def tolerance(f, t, flip, s):
    ref = R.windowed(f, t, flip, s)
    e32 = np.abs(R.fft_pipeline(f, t, flip, s, np.float32) - ref).max()
    return ref, max(4.0 * e32, 1e-3), e32


def mix_ref(f, t, flip, s):
    return tolerance(f, t, flip, s)[:2]


@pytest.mark.parametrize("H,W", [(384, 512), (331, 331)])
def test_bandpass_mixup_matches_float64_reference(tmp_path, H, W):
    from spnet_amd.augmentation import bandpass_mixup
    d, reals = real_dir(tmp_path / "real", H, W)
    files = sorted(os.path.join(d, f) for f in os.listdir(d))
    for k in range(3):
        f = fake_frame(H, W, k)
        np.random.seed(k)
        random.seed(k)
        out = bandpass_mixup(f, d)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (H, W)
        np.random.seed(k)
        random.seed(k)
        fname, flip, s = R.reference_draw(files)
        ref, tol, e32 = tolerance(f, reals[files.index(fname)], flip, float(np.float32(s)))
        err = np.abs(out - ref).max()
        print("bandpass %dx%d case %d flip %d s %.3f: device err %.3e, float32 scipy err %.3e, tol %.3e"
              % (H, W, k, flip, s, err, e32, tol))
        assert err <= tol, (err, tol)
        assert out.min() >= 0 and out.max() <= 255 and out.max() > 250


def test_uint8_output_rounds_like_the_reference(tmp_path):
    import torch
    from spnet_amd.augmentation import BandpassPool
    H, W = 384, 512
    d, reals = real_dir(tmp_path / "real", H, W, n=4, seed=1)
    mixer = BandpassPool.get(d, H, W).mixer
    fr = np.stack([fake_frame(H, W, 10 + i) for i in range(6)])
    p = mixer.draw(6, seeds=list(range(100, 106)))
    x = torch.from_numpy(fr).cuda()
    of = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    ou = torch.empty_like(x)
    mixer.apply(p, x, out_f=of, out_u8=ou)
    of, ou = of.cpu().numpy(), ou.cpu().numpy()
    assert np.array_equal(ou, R.to_u8(of))                    # the uint8 output is the float output, rounded
    for j in range(6):
        ref, tol = mix_ref(fr[j], reals[p["real"][j]], int(p["flip"][j]), float(p["s"][j]))
        assert np.abs(of[j] - ref).max() <= tol
        ref_u8 = R.to_u8(ref)
        near_half = np.abs(ref - np.floor(ref) - 0.5) <= tol
        bad = (ou[j] != ref_u8) & ~near_half
        assert not bad.any(), (j, int(bad.sum()))


def test_deterministic_and_independent_of_batch_position(tmp_path):
    import torch
    from spnet_amd.augmentation import BandpassPool
    H, W = 331, 331
    d, _ = real_dir(tmp_path / "real", H, W, n=5, seed=2)
    mixer = BandpassPool.get(d, H, W).mixer
    fr = torch.from_numpy(np.stack([fake_frame(H, W, 50 + i) for i in range(64)])).cuda()
    p = mixer.draw(64, seeds=list(range(64)))

    def run(params, frames):
        o = torch.empty(frames.shape, dtype=torch.float32, device="cuda")
        mixer.apply(params, frames.contiguous(), out_f=o)
        return o.cpu().numpy()
    a, b = run(p, fr), run(p, fr)
    assert np.array_equal(a, b)
    j = 37
    alone = run({k: v[j:j + 1] for k, v in p.items()}, fr[j:j + 1])
    assert np.array_equal(alone[0], a[j])
    q = {k: np.roll(v, 5) for k, v in p.items()}                 # the same frame at position 42 of another batch
    moved = run(q, torch.roll(fr, 5, 0))
    assert np.array_equal(moved[42], a[j])


def test_edge_cases(tmp_path):
    import torch
    from spnet_amd.augmentation import BandpassPool, bandpass_mixup
    H, W = 96, 128
    d, reals = real_dir(tmp_path / "real", H, W, seed=3)
    mixer = BandpassPool.get(d, H, W).mixer
    # constant fake frame, s = 0: all zeros (cv2.normalize of a constant)
    for v, kind in ((100, torch.uint8), (0, torch.uint8), (37.5, torch.float32)):
        x = torch.full((1, H, W), v, dtype=kind, device="cuda")
        o = torch.full((1, H, W), -1.0, device="cuda")
        mixer.apply(dict(row=np.array([5], np.int32), s=np.array([0.0], np.float32)), x, out_f=o)
        assert torch.count_nonzero(o).item() == 0
    f = fake_frame(H, W, 7)
    np.random.seed(9)
    random.seed(9)
    base = bandpass_mixup(f, d)
    for shaped in (f[..., None], torch.from_numpy(f).cuda(), torch.from_numpy(f[..., None]).cuda()):
        np.random.seed(9)
        random.seed(9)
        out = bandpass_mixup(shaped, d)
        assert tuple(out.shape) == tuple(shaped.shape)
        if isinstance(out, torch.Tensor):
            assert out.is_cuda
            out = out.cpu().numpy()
        assert np.array_equal(out.reshape(H, W), base)
    # [H,W,3] BGR: cv2's float BGR2GRAY weights, the result replicated to 3 channels
    bgr = np.stack([f, np.roll(f, 3, 0), np.roll(f, 5, 1)], -1)
    np.random.seed(9)
    random.seed(9)
    out = bandpass_mixup(bgr, d)
    assert out.shape == (H, W, 3) and np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    gray = bgr[..., 0] * 0.114 + bgr[..., 1] * 0.587 + bgr[..., 2] * 0.299
    np.random.seed(9)
    random.seed(9)
    files = sorted(os.path.join(d, n) for n in os.listdir(d))
    fname, flip, s = R.reference_draw(files)
    ref, tol = mix_ref(gray, reals[files.index(fname)], flip, float(np.float32(s)))
    assert np.abs(out[..., 0] - ref).max() <= max(tol, 1e-2)


def test_generator_with_bandpass(tmp_path):
    import torch
    from spnet_amd import fake_espi as F
    from spnet_amd.augmentation import draw_bandpass_batch
    d, reals = real_dir(tmp_path / "real", F.IM_H, F.IM_W, n=4, seed=4)
    X0, lab0, U0 = F.generate_device(6, seed=3, want_u8=True)
    # the draws depend on (n, seed) only: the same draws mix the plain frames of any chunking
    p = draw_bandpass_batch(len(reals), 6, seeds=F.bandpass_seeds(6, 3))
    for chunk in (1024, 4):
        Xp, labp, Up = F.generate_device(6, seed=3, want_u8=True, chunk=chunk)
        X1, lab1, U1 = F.generate_device(6, seed=3, want_u8=True, bandpass_real=d, chunk=chunk)
        assert lab1 == lab0 and labp == lab0
        assert not torch.equal(U1, Up)
        u1, up = U1.cpu().numpy(), Up.cpu().numpy()
        assert np.array_equal(X1.cpu().numpy(), F.to_network_input(u1))      # X = the PNG round trip of the uint8 frame
        for j in range(6):
            ref, tol = mix_ref(up[j], reals[p["real"][j]], int(p["flip"][j]), float(p["s"][j]))
            assert np.abs(u1[j].astype(np.float64) - ref).max() <= 0.5 + tol
    X2, lab2, U2 = F.generate_device(6, seed=3, want_u8=True)
    assert lab2 == lab0 and torch.equal(X2, X0) and torch.equal(U2, U0)   # without the argument: the plain frames


def test_write_dataset_bp_path_is_a_loadable_dataset(tmp_path):
    from spnet_amd import fake_espi as F
    from spnet_amd import utils as U
    d, _ = real_dir(tmp_path / "real", F.IM_H, F.IM_W, n=2, seed=5)
    plain, bp = tmp_path / "Train", tmp_path / "TrainBP"
    X, labels = F.write_dataset(str(plain), 6, seed=2, bandpass_real=d, bp_path=str(bp))
    names = sorted(os.listdir(bp))
    assert len(names) == 12 and all(n.endswith(("_bp.png", "_bp.csv")) for n in names)
    assert sorted(os.listdir(plain)) == sorted(n.replace("_bp", "") for n in names)
    for i in range(6):
        stem = "steelpan_%07d" % i
        assert open(bp / (stem + "_bp.csv")).read() == open(plain / (stem + ".csv")).read()
    Xb, Yb, files, _ = U.build_dataset(path=str(bp) + "/", load_frac=1.0, set_means_ranges=True)
    Xp, Yp, _, _ = U.build_dataset(path=str(plain) + "/", load_frac=1.0, set_means_ranges=True)
    assert len(files) == 6 and Xb.shape == Xp.shape and Yb.shape == Yp.shape


def _frames(B, H, W, seed):
    import torch
    f = np.stack([fake_frame(H, W, seed + i) for i in range(B)])
    return torch.from_numpy(f.astype(np.float32) / 255.0 * 2.0 - 1.0)[..., None].cuda().contiguous()


def test_on_the_fly_prob_zero_is_bit_identical(tmp_path):
    import torch
    from spnet_amd.augmentation import DeviceAugmenter
    H, W = 96, 128
    d, _ = real_dir(tmp_path / "real", H, W, seed=6)
    X = _frames(8, H, W, 20)
    a0, a1 = DeviceAugmenter(X), DeviceAugmenter(X, bandpass_real=d, bpmix_prob=0.0)
    o0, o1 = torch.empty_like(X), torch.empty_like(X)
    np.random.seed(4)
    random.seed(4)
    a0.augment(list(range(8)), o0)
    np.random.seed(4)
    random.seed(4)
    a1.augment(list(range(8)), o1)
    assert torch.equal(o0, o1)


def test_on_the_fly_prob_one_mixes_the_augmented_frames(tmp_path):
    import torch
    from spnet_amd.augmentation import DeviceAugmenter
    H, W = 96, 128
    d, reals = real_dir(tmp_path / "real", H, W, seed=7)
    X = _frames(6, H, W, 30)
    base, mix = DeviceAugmenter(X), DeviceAugmenter(X, bandpass_real=d, bpmix_prob=1.0)
    idx, seeds = list(range(6)), [1000 + i for i in range(6)]
    o0, o1 = torch.empty_like(X), torch.empty_like(X)
    base.apply(base.draw(idx, seeds=seeds), o0)            # cutout + salt-and-pepper only
    p = mix.draw(idx, seeds=seeds)
    mix.apply(p, o1)
    assert p["bp_n"] == 6 and list(p["bp_sel"]) == idx
    pix0 = (o0.cpu().numpy()[..., 0].astype(np.float64) / 2 + 0.5) * 255
    pix1 = (o1.cpu().numpy()[..., 0].astype(np.float64) / 2 + 0.5) * 255
    for j in idx:
        row = int(p["bp_row"][j])
        ref, tol = mix_ref(pix0[j], reals[row // 4], R.FLIPS[row % 4], float(p["bp_s"][j]))
        assert np.abs(pix1[j] - ref).max() <= tol + 1e-3          # + the [-1,1] round trip


def test_on_the_fly_seeded_draws_agree_across_shards(tmp_path):
    import torch
    from spnet_amd.augmentation import DeviceAugmenter
    H, W = 96, 128
    d, _ = real_dir(tmp_path / "real", H, W, seed=8)
    X = _frames(8, H, W, 40)
    aug = DeviceAugmenter(X, bandpass_real=d, bpmix_prob=0.5)
    idx, seeds = list(range(8)), [7000 + 3 * i for i in range(8)]
    whole = torch.empty_like(X)
    p = aug.draw(idx, seeds=seeds)
    assert 0 < p["bp_n"] < 8
    aug.apply(p, whole)
    parts = []
    for lo, hi in ((0, 4), (4, 8)):
        o = torch.empty((hi - lo,) + tuple(X.shape[1:]), device="cuda")
        aug.apply(aug.draw(idx[lo:hi], seeds=seeds[lo:hi]), o)
        parts.append(o)
    assert torch.equal(torch.cat(parts), whole)


def test_train_cli_with_bp_real(tmp_path):
    from spnet_amd import fake_espi as F
    data = tmp_path / "data"
    F.write_dataset(str(data / "Train"), 48, seed=1)
    F.write_dataset(str(data / "Val"), 16, seed=2)
    d, _ = real_dir(tmp_path / "real", 331, 331, n=3, seed=9)          # the training frames' size (model_type monolithic)
    work = tmp_path / "work"
    work.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_spnet.py"), "-d", str(data), "-b", "8", "-e", "1",
                        "--bp_real", d, "--bpmix_prob", "0.5"], cwd=str(work), env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert "SPNet execution completed." in r.stdout
