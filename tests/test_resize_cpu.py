"""Device resize, host side (no GPU needed): the integer tap tables and the numpy restatement of Pillow's 8-bit Lanczos
resampler (spnet_amd/resize.py) against PIL.Image.resize itself -- exactly, every pixel -- the recorded Pillow behaviour
(tests/golden/resize_pil.npz) and the int32 accumulator's range."""
import os

import numpy as np
import pytest
from PIL import Image

from spnet_amd import resize as RZ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W) -> (OH, OW): the network size, the 'simple' layout's, the same size (no pass), one pass only, an enlargement,
# a small odd frame reduced on both axes, one output row
CASES = [((384, 512), (331, 331)), ((384, 512), (224, 224)), ((384, 512), (384, 512)), ((384, 512), (331, 512)),
         ((96, 128), (131, 150)), ((47, 61), (29, 17)), ((47, 61), (1, 47))]


def frames(H, W, seed=0):
    """uniform noise, 0/255 binary, smooth fringes: uint8 [3, H, W]"""
    rs = np.random.RandomState(seed + 31 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([rs.randint(0, 256, (H, W)), rs.randint(0, 2, (H, W)) * 255,
                     127.5 + 127.5 * np.sin(xx / 9.0 + yy / 23.0) * np.cos(yy / 7.0)]).astype(np.uint8)


def pil_resize(a, OH, OW):
    """The input codec's own call (utils._load_one): RGB, resize, channel 0."""
    return np.asarray(Image.fromarray(a).convert("RGB").resize((OW, OH), Image.LANCZOS), dtype=np.uint8)[:, :, 0]


def test_installed_pillow_resizes_as_recorded():
    """The fixture pins the Pillow behaviour every other test here (and the kernel) is held to: a failure HERE means the
    installed Pillow's resampler drifted from the recorded one, not that the restatement or the kernel is wrong."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "resize_pil.npz"), allow_pickle=False)
    for k, (OH, OW) in enumerate(g["sizes"]):
        got = pil_resize(g["frame"], int(OH), int(OW))
        assert np.array_equal(got, g["resized_%d" % k]), \
            "Pillow drifted: %d pixels differ at %dx%d from Pillow %s's result" % (
                int((got != g["resized_%d" % k]).sum()), OH, OW, g["pillow_version"])


def test_restatement_equals_recorded_pillow():
    g = np.load(os.path.join(ROOT, "tests", "golden", "resize_pil.npz"), allow_pickle=False)
    for k, (OH, OW) in enumerate(g["sizes"]):
        assert np.array_equal(RZ.resize_u8_host(g["frame"], (int(OH), int(OW))), g["resized_%d" % k]), (OH, OW)


@pytest.mark.parametrize("src,dst", CASES)
def test_restatement_equals_pillow_exactly(src, dst):
    (H, W), (OH, OW) = src, dst
    X = frames(H, W)
    got = RZ.resize_u8_host(X, (OH, OW))
    assert got.shape == (3, OH, OW) and got.dtype == np.uint8
    for i in range(3):
        ref = pil_resize(X[i], OH, OW)
        assert np.array_equal(got[i], ref), "%d of %d pixels differ (frame %d, %s -> %s)" % (
            int((got[i] != ref).sum()), ref.size, i, src, dst)


def test_tap_tables():
    """Layout (first index, count, taps, zero padding), windows inside the axis and rising with the output index (the
    kernel takes a tile's source range from its first and last entry), taps summing to 2^22 within their rounding, the
    widths the kernel keeps in registers for the network size, and the cache."""
    for I, O in [(512, 331), (384, 331), (512, 224), (128, 150), (61, 17), (47, 1), (2048, 1), (1, 2048), (7, 7)]:
        t = RZ.lanczos_taps(I, O)
        assert t.dtype == np.int32 and t.shape[0] == O and not t.flags.writeable
        lo, cnt = t[:, 0].astype(int), t[:, 1].astype(int)
        assert (lo >= 0).all() and (cnt >= 1).all() and (lo + cnt <= I).all() and cnt.max() == t.shape[1] - 2
        assert (np.diff(lo) >= 0).all() and (np.diff(lo + cnt) >= 0).all()
        for o in range(O):
            assert not t[o, 2 + cnt[o]:].any()
        # (each tap is rounded to the nearest integer: the sum is off by at most half a unit per tap)
        assert (np.abs(t[:, 2:].astype(np.int64).sum(axis=1) - (1 << 22)) <= cnt / 2 + 1).all(), (I, O)
        assert np.abs(t[:, 2:]).max() < RZ.TAP_LIMIT
        assert RZ.lanczos_taps(I, O) is t
    assert RZ.lanczos_taps(512, 331).shape == (331, 2 + 10)
    assert RZ.lanczos_taps(384, 331).shape == (331, 2 + 7)
    with pytest.raises(ValueError):
        RZ.lanczos_taps(0, 5)


def test_accumulator_fits_int32_for_every_tested_pair():
    """Pillow accumulates in a C int: 255 * sum|k| + 2^21 must stay below 2^31 for every size pair the CPU and GPU tests
    use (it does: the largest is 512 -> 331 at 0.70 * 2^31), or the kernel would have to wrap the same way."""
    pairs = set()
    for (H, W), (OH, OW) in CASES + [((64, 80), (41, 53)), ((64, 80), (64, 37)), ((64, 80), (100, 129))]:
        pairs.add((W, OW))
        pairs.add((H, OH))
    for I, O in sorted(pairs):
        if I != O:
            bound = RZ.accumulator_bound(RZ.lanczos_taps(I, O))
            assert bound < 2 ** 31, "%d -> %d: the accumulator can reach %d" % (I, O, bound)


def test_host_resize_argument_forms():
    X = frames(47, 61)
    assert np.array_equal(RZ.resize_u8_host(X, 20), RZ.resize_u8_host(X, (20, 20)))
    assert np.array_equal(RZ.resize_u8_host(X[0], (47, 61)), X[0])
    with pytest.raises(TypeError):
        RZ.resize_u8_host(X.astype(np.float32), 20)
