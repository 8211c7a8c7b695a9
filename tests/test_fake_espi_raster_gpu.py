"""spnet_amd/csrc/espi.hip pixel by pixel against the float64 restatement of its own specification (tests/helpers/
espi_raster_ref.py, pinned on the CPU by tests/test_fake_espi_cpu.py): the noise-free canvas EQUALS the reference wherever
no comparison was decided by less than 1e-3 px, on drawn frames and on crafted launches chosen for the indexing and the
branches; the labelled ring count can be read back from the device's pixels; the sensor model's dropout mask is the
reference's bit for bit and its noise is the reference's to one grey level; the two outputs are one codec apart."""
import numpy as np
import pytest
import torch

from tests.helpers import espi_raster_ref as R

pytestmark = pytest.mark.gpu

PAD = 4096                      # guard elements behind every output: the kernel must not write past N*H*W
GUARD_U8, GUARD_F = 77, 7.0     # neither is a canvas level / a network input


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _launch(waves, nodes, nn, H, W, seed=0, noise=0, want_f=True, want_u8=True):
    """One spnet_fake_espi launch into guarded buffers -> (out_f [N,H,W] float32 or None, out_u8 [N,H,W] uint8 or None)."""
    from spnet_amd import _lib as L
    N = len(nn)
    n = N * H * W
    wd, ndd, nnd = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (waves, nodes, nn))
    Xf = torch.full((n + PAD,), GUARD_F, dtype=torch.float32, device="cuda") if want_f else None
    U = torch.full((n + PAD,), GUARD_U8, dtype=torch.uint8, device="cuda") if want_u8 else None
    L.spnet_fake_espi(wd.data_ptr(), ndd.data_ptr(), nnd.data_ptr(), N, H, W, seed, noise, L.ptr(Xf), L.ptr(U),
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = []
    for buf, guard in ((Xf, GUARD_F), (U, GUARD_U8)):
        if buf is None:
            out.append(None)
            continue
        host = buf.cpu().numpy()
        assert (host[n:] == guard).all(), "the kernel wrote past the end of its output"
        out.append(host[:n].reshape(N, H, W))
    return out


def _assert_equal_where_clear(dev, ref, margin, what):
    near = margin < R.NEAR_TIE
    differ = dev != ref
    print("%s: %d of %d pixels near a tie (%.4f %%), %d of those differ; %d differ elsewhere"
          % (what, int(near.sum()), near.size, 100.0 * near.mean(), int((differ & near).sum()), int((differ & ~near).sum())))
    bad = np.argwhere(differ & ~near)
    assert len(bad) == 0, (what, [(tuple(int(v) for v in b), int(dev[tuple(b)]), int(ref[tuple(b)]), float(margin[tuple(b)]))
                                  for b in bad[:8]])
    assert near.sum() < R.NEAR_TIE_SHARE * near.size, what


@pytest.mark.parametrize("count_range,seed", [((1, 7), 5), ((0, 6), 4)])
def test_drawn_frames_equal_the_specification(count_range, seed):
    """(frame, y, x) of every pixel: the device canvas of generate_device == canvas_ref of the same draw_params."""
    _need_gpu()
    from spnet_amd import fake_espi as F
    X, labels, U = F.generate_device(4, seed=seed, noise=False, want_u8=True, count_range=count_range)
    (waves, nodes, nn), lists = R.drawn_launch(4, seed, count_range)
    if count_range == (0, 6):
        assert 0 in nn.tolist() and nn.max() > 0               # a frame without any antinode
    assert [[tuple(nd[:6]) for nd in fr] for fr in lists] == [[tuple(r) for r in fr] for fr in labels]
    ref, margin = R.canvas_ref(waves, nodes, nn, F.IM_H, F.IM_W)
    dev = U.cpu().numpy()
    assert set(np.unique(dev)) <= {R.BLACK, R.GREY, R.RING}
    _assert_equal_where_clear(dev, ref, margin, "drawn %s seed %d" % (count_range, seed))
    checked = R.check_labels_in_pixels(dev, lists)              # the CSV's ring count and start colour, read from the frame
    assert checked == sum(len(fr) for fr in lists)
    np.testing.assert_array_equal(X.cpu().numpy()[..., 0], F.to_network_input(dev)[..., 0])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_crafted_launches_equal_the_specification(name):
    _need_gpu()
    H, W, waves, nodes, nn = R.case_launch(name)
    ref, margin = R.canvas_ref(waves, nodes, nn, H, W)
    Xf, dev = _launch(waves, nodes, nn, H, W)
    assert set(np.unique(dev)) <= {R.BLACK, R.GREY, R.RING}     # every pixel written (the guard value is none of these)
    _assert_equal_where_clear(dev, ref, margin, name)
    assert np.array_equal(Xf, ((dev.astype(np.float32) / np.float32(255) - np.float32(0.5)) * np.float32(2)))


@pytest.fixture(scope="module")
def sensor_case():
    _need_gpu()
    H, W, waves, nodes, nn = R.case_launch(R.SENSOR_CASE)
    _, canvas = _launch(waves, nodes, nn, H, W, noise=0, want_f=False)
    ref, margin = R.canvas_ref(waves, nodes, nn, H, W)
    assert np.array_equal(canvas[margin >= R.NEAR_TIE], ref[margin >= R.NEAR_TIE])
    canvas.setflags(write=False)
    return H, W, waves, nodes, nn, canvas


@pytest.mark.parametrize("seed", [12345, 0xfffffff3])
def test_sensor_model_is_the_reference_mask_and_noise(sensor_case, seed):
    """Dropout: the device's zeros are the reference's h3 bit, pixel for pixel.  Noise: every kept pixel is
    min(canvas + clip(rint(n), 0, 255), 255) of the float64 Box-Muller value or one grey level beside it (the kernel's
    __logf / __cosf against float64 log / cos move n across a rounding boundary for a few pixels), at most 1 % of them.
    Measured on an MI355X: 0 of 18,628 and 0 of 18,611 kept pixels one level off (0 %), none further."""
    H, W, waves, nodes, nn, canvas = sensor_case
    mask, noisy, n = R.sensor_ref(canvas, seed, H, W)
    _, dev = _launch(waves, nodes, nn, H, W, seed=seed, noise=1, want_f=False)
    assert 0.45 < mask.mean() < 0.55
    assert (dev[mask] == 0).all()                                # every pixel whose h3 bit is set is dropped
    kept = ~mask
    off = np.abs(dev.astype(np.int64) - noisy.astype(np.int64))[kept]
    share = float((off == 1).mean())
    print("seed %#x: %d kept pixels, %d one grey level off (%.4f %%), largest difference %d"
          % (seed, off.size, int((off == 1).sum()), 100 * share, int(off.max())))
    assert off.max() <= 1                                        # nothing else is touched by dropout, no other noise value
    assert share <= 0.01
    bright = noisy >= 2                                          # where the kept value cannot itself be 0: the masks are EQUAL
    assert np.array_equal((dev == 0)[bright], mask[bright])
    for a in range(3):                                           # frames of one launch draw from different counters
        for b in range(a + 1, 3):
            assert not np.array_equal(mask[a], mask[b]) and not np.array_equal(dev[a] == 0, dev[b] == 0)
            assert not np.array_equal(n[a], n[b])
    assert not np.array_equal(mask[0, 0], mask[0, 1])            # ... and so do rows


def test_outputs_are_one_codec_apart(sensor_case):
    from spnet_amd import _lib as L
    H, W, waves, nodes, nn, _ = sensor_case
    seed = 424242
    Xf, U = _launch(waves, nodes, nn, H, W, seed=seed, noise=1)
    ud = torch.from_numpy(U.copy()).cuda()
    want = torch.full((U.size,), float("nan"), device="cuda")
    L.spnet_u8_to_input(ud.data_ptr(), want.data_ptr(), U.size, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(Xf.ravel().view(np.uint32), want.cpu().numpy().view(np.uint32))
    only_f, none_u = _launch(waves, nodes, nn, H, W, seed=seed, noise=1, want_u8=False)
    none_f, only_u = _launch(waves, nodes, nn, H, W, seed=seed, noise=1, want_f=False)
    assert none_u is None and none_f is None
    assert np.array_equal(only_f.view(np.uint32), Xf.view(np.uint32)) and np.array_equal(only_u, U)
    wd, ndd, nnd = (torch.from_numpy(a).cuda() for a in (waves, nodes, nn))
    with pytest.raises(L.HipError):
        L.spnet_fake_espi(wd.data_ptr(), ndd.data_ptr(), nnd.data_ptr(), 3, H, W, seed, 1, None, None,
                          torch.cuda.current_stream().cuda_stream)
