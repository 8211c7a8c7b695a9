"""csrc/masks.hip through spnet_amd/masks.py against the Python-integer restatement (tests/helpers/mask_ref.py): exact
equality everywhere.  Every test guards its angles with assert_trig_safe (a condition on the inputs, see mask_ref).

Shapes are the smallest at which the kernels can still go wrong: 40 x 56 (no multiple of the 64 x 16 tile, W % 16 != 0: byte
stores), 33 x 130 (three tiles across and down, byte stores), 16 x 64 (exactly one tile, the 16-byte stores) and both again
with `out` one byte off; the comparison on frames of 1, 63 and 4,099 pixels (16-byte loads on frame 0, byte loads on the
misaligned frames 1 and 2, a tail after the vector part).  One full-size case: 72 rows a frame from a prediction grid."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from spnet_amd import masks as MK
from tests.helpers import mask_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = "hipError_t 1$"           # hipErrorInvalidValue


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(rows, count):
    return (torch.from_numpy(np.ascontiguousarray(rows, np.float64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(count, np.int32)).cuda())


def _raw_masks(rows_d, count_d, H, W, offset, fill=0xA5):
    """spnet_ring_masks into a buffer `offset` bytes past a 16-byte aligned address; (masks, the bytes around them)."""
    from spnet_amd import _lib as L
    B, K = rows_d.shape[:2]
    buf = torch.full((B * H * W + 32,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    L.spnet_ring_masks(rows_d.data_ptr(), count_d.data_ptr(), B, K, H, W, buf.data_ptr() + offset, L.current_stream())
    host = buf.cpu().numpy()
    return host[offset:offset + B * H * W].reshape(B, H, W), np.concatenate([host[:offset], host[offset + B * H * W:]])


def test_g1_case_table():
    _need_gpu()
    names, rows, count = R.table_arrays()
    R.assert_trig_safe(rows[..., 4])
    want = R.ring_masks(rows, count, R.TABLE_H, R.TABLE_W)
    got = MK.ring_masks_device(*_dev(rows, count), H=R.TABLE_H, W=R.TABLE_W)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), name
    assert np.count_nonzero(want[names.index("one pixel")]) == 1
    # a host list of label lists goes through pad_metadata; B == 0 succeeds and does nothing
    labels = [[tuple(r) for r in rows[i, :min(max(count[i], 0), R.TABLE_K)]] for i in range(len(names))]
    assert np.array_equal(MK.ring_masks_device(labels, H=R.TABLE_H, W=R.TABLE_W).cpu().numpy(), want)
    empty = MK.ring_masks_device(torch.zeros((0, 4, 6), dtype=torch.float64, device="cuda"),
                                 torch.zeros((0,), dtype=torch.int32, device="cuda"), H=8, W=8)
    assert tuple(empty.shape) == (0, 8, 8)


def _tiling_rows(H, W):
    """One ellipse over every tile of the frame, one exactly tangent to the border between the first two tile columns
    (x = 64: its rightmost pixel centre 63.5 lies ON the rim), a small one inside the last tile, a circle on a tile corner."""
    rows = [(W / 2.0, H / 2.0, 0.75 * W, 0.75 * H, 0, 1),
            (43.5, 8.5, 20, 5, 0, 2),
            (W - 6.0, H - 4.0, 4, 2, 45, 3),
            (64, 16, 3, 3, 0, 4)]
    return np.asarray([rows], np.float64), np.asarray([len(rows)], np.int32)


@pytest.mark.parametrize("H,W", [(33, 130), (16, 64)])
def test_g2_tiling_and_store_paths(H, W):
    _need_gpu()
    rows, count = _tiling_rows(H, W)
    R.assert_trig_safe(rows[..., 4])
    want = R.ring_masks(rows, count, H, W)
    assert want[0, 8, 63] == 20 and (W <= 64 or want[0, 8, 64] != 20)            # tangent: the rim pixel is in, the next is not
    for ty in range(0, H, 16):
        for tx in range(0, W, 64):
            assert (want[0, ty:ty + 16, tx:tx + 64] == 10).any(), (ty, tx)      # the big ellipse is in every tile
    rows_d, count_d = _dev(rows, count)
    for offset in (0, 1):
        got, around = _raw_masks(rows_d, count_d, H, W, offset)
        assert np.array_equal(got, want), offset
        assert (around == 0xA5).all(), offset                                   # nothing outside [B][H][W] is written
    assert np.array_equal(MK.ring_masks_device(rows_d, count_d, H=H, W=W).cpu().numpy(), want)


def _random_grid(B, seed):
    rng = np.random.RandomState(seed)
    Y = np.zeros((B, 72, 8), np.float32)
    Y[..., 0], Y[..., 1] = rng.uniform(0, 512, (B, 72)), rng.uniform(0, 384, (B, 72))
    Y[..., 2], Y[..., 3] = rng.uniform(4, 40, (B, 72)), rng.uniform(4, 30, (B, 72))
    th = rng.uniform(0, 2 * np.pi, (B, 72))
    Y[..., 4], Y[..., 5] = np.cos(th), np.sin(th)
    Y[..., 6], Y[..., 7] = rng.uniform(0, 1, (B, 72)), rng.uniform(0, 11, (B, 72))
    return Y.reshape(B, 576)


def test_g3_masks_from_predictions_full_size():
    _need_gpu()
    Y = _random_grid(2, 11)
    g = Y.astype(np.float64).reshape(2, 72, 8)
    angle = np.rad2deg(np.arctan2(g[..., 5], g[..., 4]) / 2.0)
    a = np.where(g[..., 6] >= 0.5, 0.0, g[..., 2])
    rows = np.stack([g[..., 0], g[..., 1], a, g[..., 3], angle, g[..., 7]], -1)
    R.assert_trig_safe(angle)
    want = R.ring_masks(rows, [72, 72], 384, 512)
    assert 20 < np.count_nonzero(a) < 124 and np.unique(want).size > 20
    for Yin in (Y, torch.from_numpy(Y).cuda()):
        got = MK.masks_from_predictions(Yin)
        assert got.is_cuda and tuple(got.shape) == (2, 384, 512)
        assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("n_pixels", [1, 63, 4099])
def test_g4_mask_compare(n_pixels):
    _need_gpu()
    from spnet_amd import _lib as L
    N, tol0 = 3, 5
    rng = np.random.RandomState(n_pixels)
    p = rng.choice([0, 0, 10, 20, 30, 200], (N, n_pixels)).astype(np.uint8)
    t = rng.choice([0, 0, 10, 25, 36, 255], (N, n_pixels)).astype(np.uint8)
    if n_pixels >= 63:                  # every class, and |p - t| exactly tol and tol + 1, in every frame
        p[:, :6] = [0, 40, 40, 40, 9, 0]
        t[:, :6] = [0, 40 + tol0, 40 - tol0 - 1, 40 - tol0, 0, 9]
        assert all((R.compare_counts(p, t, tol0)[n] > 0).all() for n in range(N))
    else:
        p[:, 0], t[:, 0] = [0, 40, 40], [0, 40 + tol0, 40 + tol0 + 1]           # bg_bg, a hit at exactly tol, a miss at tol + 1
    for offset in (0, 1):
        pb = torch.zeros(N * n_pixels + 16, dtype=torch.uint8, device="cuda")
        tb = torch.zeros(N * n_pixels + 16, dtype=torch.uint8, device="cuda")
        pb[offset:offset + N * n_pixels] = torch.from_numpy(p.reshape(-1)).cuda()
        tb[offset:offset + N * n_pixels] = torch.from_numpy(t.reshape(-1)).cuda()
        for tol in (0, 5, 255):
            counts = torch.full((N + 2, 5), -7, dtype=torch.int32, device="cuda")
            L.spnet_mask_compare(pb.data_ptr() + offset, tb.data_ptr() + offset, N, n_pixels, tol, counts.data_ptr() + 20,
                                 L.current_stream())
            got = counts.cpu().numpy()
            want = R.compare_counts(p, t, tol)
            assert np.array_equal(got[1:N + 1], want), (offset, tol)
            assert (got[0] == -7).all() and (got[N + 1] == -7).all()            # other frames' rows are not disturbed
            assert (got[1:N + 1].sum(1) == n_pixels).all()
    # the public wrapper: the five sums and the three ratios
    res = MK.compare_masks_device(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda(), tol=5)
    want = R.compare_counts(p, t, 5).sum(0).tolist()
    assert [res[k] for k in MK.COUNT_NAMES] == want
    assert res == MK.metrics_from_counts(*want) == MK.compare_masks_host(p, t, 5)


def test_g5_invalid_arguments_write_nothing():
    _need_gpu()
    from spnet_amd import _lib as L
    H, W, K = 8, 16, 4
    rows = torch.zeros((1, 130, 6), dtype=torch.float64, device="cuda")
    rows[0, :, :] = torch.tensor([8.0, 4.0, 5.0, 3.0, 0.0, 2.0], dtype=torch.float64)
    count = torch.full((4,), 1, dtype=torch.int32, device="cuda")
    out = torch.full((H * W,), 0x5A, dtype=torch.uint8, device="cuda")
    st = L.current_stream()
    r, c, o = rows.data_ptr(), count.data_ptr(), out.data_ptr()
    for args in ((None, c, 1, K, H, W, o), (r, None, 1, K, H, W, o), (r, c, 1, K, H, W, None),
                 (r, c, 1, 0, H, W, o), (r, c, 1, 129, H, W, o), (r, c, 1, K, 0, W, o), (r, c, 1, K, H, 0, o),
                 (r, c, 1, K, 16385, W, o), (r, c, -1, K, H, W, o), (r + 4, c, 1, K, H, W, o), (r, c + 2, 1, K, H, W, o)):
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_ring_masks(*args, st)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0x5A).all()
    L.spnet_ring_masks(r, c, 1, K, H, W, o, st)                                 # the same arguments, valid: it paints
    assert (out.cpu().numpy().reshape(H, W)[4, 8] == 20)

    p = torch.zeros(64, dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 5), -7, dtype=torch.int32, device="cuda")
    pp, cc = p.data_ptr(), counts.data_ptr()
    for args in ((None, pp, 1, 64, 5, cc), (pp, None, 1, 64, 5, cc), (pp, pp, 1, 64, 5, None), (pp, pp, 1, 0, 5, cc),
                 (pp, pp, -1, 64, 5, cc), (pp, pp, 1, 64, 256, cc), (pp, pp, 1, 64, -1, cc), (pp, pp, 1, 64, 5, cc + 2)):
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_mask_compare(*args, st)
    torch.cuda.synchronize()
    assert (counts.cpu().numpy() == -7).all()
    with pytest.raises(ValueError):
        MK.ring_masks_device(rows, count[:1], H=0, W=W)
    with pytest.raises(ValueError):
        MK.compare_masks_device(p.reshape(1, 8, 8), p.reshape(1, 8, 8), tol=256)


def test_g6_fake_espi_parameters_end_to_end():
    _need_gpu()
    from spnet_amd import fake_espi as F
    _, nodes, nnode = F.draw_params_device(4, seed=3)
    labels = F.labels_from_params(nodes, nnode)
    assert sum(len(r) for r in labels) >= 4
    R.assert_trig_safe([r[4] for rows in labels for r in rows])
    want = R.masks_of_labels(labels, F.IM_H, F.IM_W)
    got = MK.ring_masks_device(*F.rows_from_params(nodes, nnode), H=F.IM_H, W=F.IM_W)
    assert np.array_equal(got.cpu().numpy(), want)
    assert want.max() == max(10 * r[5] for rows in labels for r in rows)


def test_g6_gen_fake_espi_masks_on_the_device(tmp_path):
    """gen_dataset(masks=True) with the three writers: the masks decode to the restatement's masks of the CSV rows, the
    frames and CSV files are those of a run without masks."""
    _need_gpu()
    from PIL import Image
    import gen_fake_espi as G
    plain = G.gen_dataset(datapath=str(tmp_path / "plain"), numframes=3, seed=4)
    want = None
    for name, kw in (("pillow", {}), ("dev", {"device_png": True}), ("lz", {"device_png_lz": True})):
        labels = G.gen_dataset(datapath=str(tmp_path / name), numframes=3, seed=4, masks=True, **kw)
        assert labels == plain
        if want is None:
            R.assert_trig_safe([r[4] for rows in labels for r in rows])
            want = R.masks_of_labels(labels, 384, 512)
        for i in range(3):
            stem = "steelpan_%07d" % i
            assert np.array_equal(np.asarray(Image.open(tmp_path / name / "Train" / "masks" / (stem + ".png"))), want[i]), name
            assert (tmp_path / name / "Train" / (stem + ".csv")).read_text() == (tmp_path / "plain" / "Train" / (stem + ".csv")).read_text()
            assert np.array_equal(np.asarray(Image.open(tmp_path / name / "Train" / (stem + ".png"))),
                                  np.asarray(Image.open(tmp_path / "plain" / "Train" / (stem + ".png"))))


def test_g6_evaluate_mask_metric_cli(tmp_path):
    _need_gpu()
    import re
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    data = tmp_path / "data"
    F.write_dataset(str(data) + "/", 4, seed=6)
    model = M.Model((331, 331, 1), Y0size=576, seed=8)
    model.save(str(tmp_path / "full_model.h5"))
    del model
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_spnet.py"), "-d", str(data), "-b", "4", "-l", "logs/e/",
                        "--mask_metric"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    for ratio in ("pixel_acc", "object_iou", "ring_acc"):
        assert re.search(ratio + r" = (None|[0-9.e-]+)", r.stdout), ratio
    counts = [int(re.search(k + r" = (\d+)", r.stdout).group(1)) for k in MK.COUNT_NAMES]
    assert sum(counts) == 4 * 384 * 512
    assert counts[1] + counts[2] + counts[4] > 0                                # the true masks are not empty
    log = (tmp_path / "logs" / "e" / "mask_metric.txt").read_text()
    assert all(("%s = %d" % (k, v)) in log for k, v in zip(MK.COUNT_NAMES, counts)) and "pixel_acc = " in log
