"""spnet_amd/masks.py without a GPU: the host rule against the Python-integer restatement (tests/helpers/mask_ref.py), the
rule against the analytic raster of diagnostics.create_ellipse_image, the value map, `gen_fake_espi.py --masks` on a machine
without a GPU, and the metric's arithmetic."""
import math
import os

import numpy as np
import pytest
from PIL import Image

from spnet_amd import diagnostics as D
from spnet_amd import masks as MK
from tests.helpers import mask_ref as R


@pytest.fixture(scope="module")
def table():
    names, rows, count = R.table_arrays()
    R.assert_trig_safe(rows[..., 4])
    want = R.ring_masks(rows, count, R.TABLE_H, R.TABLE_W)
    want.setflags(write=False)
    return names, rows, count, want


def test_c1_host_rule_equals_the_restatement(table):
    names, rows, count, want = table
    got = MK.ring_masks_host(rows, count, R.TABLE_H, R.TABLE_W)
    for i, name in enumerate(names):
        assert np.array_equal(got[i], want[i]), name
    # the culling box holds every painted pixel: painting without it gives the same masks
    assert np.array_equal(MK.ring_masks_host(rows, count, R.TABLE_H, R.TABLE_W, use_box=False), want)
    # a list of label lists is pad_metadata's layout
    labels = [[tuple(r) for r in rows[i, :min(max(count[i], 0), R.TABLE_K)]] for i in range(len(names))]
    assert np.array_equal(MK.ring_masks_host(labels, H=R.TABLE_H, W=R.TABLE_W), want)


def test_c1_the_table_shows_what_it_names(table):
    names, rows, count, want = table
    m = dict(zip(names, want))
    assert m["centred"].max() == 30 and m["centred"][20, 28] == 30 and m["centred"][0, 0] == 0
    for edge, sl in (("left", np.s_[:, 0]), ("right", np.s_[:, -1]), ("top", np.s_[0, :]), ("bottom", np.s_[-1, :])):
        assert m["crosses " + edge][sl].any(), edge
    four = m["crosses all four"]
    assert four[:, 0].any() and four[:, -1].any() and four[0].any() and four[-1].any() and not four[0, 0] and not four[-1, -1]
    assert not m["wholly outside"].any() and not m["count 0"].any() and not m["count below 0"].any()
    assert m["centre outside, rim inside"][20, 0] == 60 and m["centre outside, rim inside"][39, 55] == 70
    assert np.count_nonzero(m["one pixel"]) == 1 and m["one pixel"][7, 10] == 110
    assert set(np.unique(m["painter order"])) == {0, 10, 20, 30} and m["painter order"][22, 26] == 30
    assert m["a zero erases"][20, 28] == 0 and m["a zero erases"][20, 18] == 40
    assert np.count_nonzero(m["count above K"] == 90) > 0                       # the fourth row: count 9 is clamped to K = 4
    assert not m["rows that paint nothing"].any() and not m["more that paint nothing"].any()
    assert set(np.unique(m["nothing, then something"])) == {0, 30}
    assert not np.array_equal(m["angle 0"], m["angle 1"]) and not np.array_equal(m["angle 45"], m["angle 135"])


C2_CASES = [(40.0, 36.0, 30.0, 12.0, 25.0), (47.3, 41.9, 6.0, 6.0, 0.0), (50.25, 30.5, 9.0, 33.0, 110.0),
            (10.0, 70.0, 28.5, 17.25, 7 * R.Q), (64.0, 40.0, 6.0, 20.0, 90.0), (48.0, 40.0, 44.0, 38.0, 135.0)]


@pytest.mark.parametrize("cx,cy,a,b,angle", C2_CASES)
def test_c2_against_the_analytic_raster(cx, cy, a, b, angle):
    """create_ellipse_image samples the ellipse at integer coordinates, the mask rule at pixel centres (x + 1/2, y + 1/2): the
    same ellipse is therefore handed to the rule half a pixel further down and right.  Then the set mask > 0 differs from the
    analytic raster only where the fp64 level (u/a)^2 + (v/b)^2 is within 0.5 / min(a, b) of 1 (the quantisations move the
    rim by less than 1/8 pixel, the level changes by about 2 / min(a, b) per pixel there; twice that), and nowhere else."""
    nx, ny = 96, 80
    t2 = 2.0 * math.radians(angle)
    args = (cx, cy, a, b, math.cos(t2), math.sin(t2), 0.0, 3.0)
    analytic = D.create_ellipse_image(args, nx=nx, ny=ny) > 0
    ang = np.arctan2(args[5], args[4]) / 2.0
    R.assert_trig_safe([np.rad2deg(ang)])
    got = MK.ring_masks_host([[(cx + 0.5, cy + 0.5, a, b, np.rad2deg(ang), 3.0)]], H=ny, W=nx)[0]
    assert set(np.unique(got)) <= {0, 30}
    xs, ys = np.meshgrid(np.arange(nx), np.arange(ny))
    dx, dy = xs - cx, ys - cy
    u = dx * np.cos(-ang) + dy * np.sin(-ang)
    v = -dx * np.sin(-ang) + dy * np.cos(-ang)
    level = (u / a) ** 2 + (v / b) ** 2
    differ = (got > 0) != analytic
    assert analytic.sum() > 100
    assert not differ[np.abs(level - 1.0) > 0.5 / min(a, b)].any(), int(differ.sum())


def test_c3_value_map():
    rings = [0, 0.09, 0.1, 1, 7.34, 11, 25.5, 25.6, 1e9, -3]
    want = [0, 0, 1, 10, 73, 110, 255, 255, 255, 0]
    for r, w in zip(rings, want):
        assert MK.quantise_row((5, 5, 3, 3, 0, r))[6] == w == R.value_of(r), r
        got = MK.ring_masks_host([[(5, 5, 4, 4, 0, 1), (5.5, 5.5, 2, 2, 0, r)]], H=10, W=10)[0]
        assert got[5, 5] == w and got[5, 2] == 10, r                             # the second row paints its value, zeros too
    assert MK.quantise_row((5, 5, 3, 3, 0, float("nan"))) is None
    got = MK.ring_masks_host([[(5, 5, 4, 4, 0, 1), (5.5, 5.5, 2, 2, 0, float("nan"))]], H=10, W=10)[0]
    assert got[5, 5] == 10                                                      # NaN rings: the row paints nothing


def _read_csv_rows(path):
    text = open(path).read().strip()
    return [tuple(float(v) for v in line.split(",")) for line in text.splitlines() if line != "0,0,0,0,0,0.0"]


def test_c4_gen_fake_espi_masks_without_a_gpu(tmp_path, monkeypatch):
    import torch
    import gen_fake_espi as G
    from spnet_amd import utils as U
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError):                                           # without --masks nothing changed
        G.main(["-d", str(tmp_path / "plain"), "-n", "3"])
    out = tmp_path / "set"
    G.main(["-d", str(out), "-n", "3", "--masks", "--seed", "5"])
    train = out / "Train"
    names = ["steelpan_%07d" % i for i in range(3)]
    labels = [_read_csv_rows(train / (n + ".csv")) for n in names]
    assert sum(len(r) for r in labels) >= 3
    R.assert_trig_safe([r[4] for rows in labels for r in rows])
    want = R.masks_of_labels(labels, 384, 512)
    for i, n in enumerate(names):
        got = np.asarray(Image.open(train / "masks" / (n + ".png")))
        assert got.dtype == np.uint8 and got.shape == (384, 512)
        assert np.array_equal(got, want[i]), n
        assert got.max() == max(int(10 * r[5]) for r in labels[i])
    assert sorted(os.listdir(train / "masks")) == [n + ".png" for n in names]
    # the loaders glob path + '*.png', not recursively: the masks are invisible to them
    X, Y, files, _ = U.build_dataset(path=str(train) + "/", shuffle=False)
    assert [os.path.basename(f) for f in files] == [n + ".png" for n in names] and len(X) == len(Y) == 3


def test_c5_metric_arithmetic():
    m = MK.metrics_from_counts(70, 12, 8, 6, 4)
    assert [m[k] for k in MK.COUNT_NAMES] == [70, 12, 8, 6, 4]
    assert m["pixel_acc"] == 82 / 100 and m["object_iou"] == 20 / 30 and m["ring_acc"] == 12 / 20
    m = MK.metrics_from_counts(50, 0, 0, 0, 0)                                   # nothing anywhere
    assert m["pixel_acc"] == 1.0 and m["object_iou"] is None and m["ring_acc"] is None
    m = MK.metrics_from_counts(5, 0, 0, 3, 2)                                    # objects, but never both
    assert m["pixel_acc"] == 0.5 and m["object_iou"] == 0.0 and m["ring_acc"] is None
    m = MK.metrics_from_counts(0, 0, 0, 0, 0)
    assert m["pixel_acc"] is None and m["object_iou"] is None and m["ring_acc"] is None
    # the host comparison counts as the restatement does, and tol is the only thing that moves hit <-> miss
    p = np.array([[0, 0, 10, 15, 16, 200, 0, 7]], np.uint8)
    t = np.array([[0, 3, 15, 10, 10, 200, 0, 0]], np.uint8)
    for tol, want in ((0, [2, 1, 3, 1, 1]), (5, [2, 3, 1, 1, 1]), (255, [2, 4, 0, 1, 1])):
        got = MK.compare_masks_host(p, t, tol)
        assert [got[k] for k in MK.COUNT_NAMES] == want == R.compare_counts(p, t, tol)[0].tolist()
    with pytest.raises(ValueError):
        MK.compare_masks_host(p, t, 256)
