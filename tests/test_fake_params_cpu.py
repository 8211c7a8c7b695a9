"""The device parameter sampler's recipe, checked on the host (no GPU): tests/helpers/fake_params_ref.py restates
spnet_fake_espi_params (include/spnet_hip.h) in numpy; here its stream is checked for the generator's invariants, for the
same distributions as the reference-ordered host stream (fake_espi.draw_params), for independence of how a frame range is
split, and FakeStream's target path against the file path (rows_to_csv -> parse_meta_file -> true_to_pred_grid -> norm_Y)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "helpers"))
import fake_params_ref as R  # noqa: E402

H, W = 384, 512
N_INV = 2000
# Frames per stream of the distribution test.  Chosen on the CPU: at this count fake_espi.draw_params compared with ITSELF
# at two different seeds (frame_seeds(1500, 0) against frame_seeds(1500, 1), and 2 against 3) passes the same
# four-standard-error check on all six statistics.
N_DIST = 1500


@pytest.fixture(scope="module")
def streams():
    return {cr: R.params(0, N_INV, seed=0, count_range=cr) for cr in ((1, 7), (0, 6))}


@pytest.mark.parametrize("cr", [(1, 7), (0, 6)])
def test_invariants_of_the_restated_stream(streams, cr):
    p = streams[cr]
    waves, nodes, nnode, tries, count = p["waves"], p["nodes"], p["nnode"], p["tries"], p["count"]
    amp, wl, thick, slope, spacing = waves.T
    assert ((amp >= 10) & (amp <= 200) & (amp == np.rint(amp))).all()
    assert ((wl >= 100) & (wl <= W // 2) & (wl == np.rint(wl))).all()
    assert ((thick >= 15) & (thick <= 40) & (thick == np.rint(thick))).all()
    assert ((slope >= -1.5) & (slope < 1.5)).all()
    lo = thick + thick * np.trunc(np.abs(np.float32(1.5) * slope))
    assert ((spacing >= lo) & (spacing <= H // 3)).all()
    assert ((count >= cr[0]) & (count <= cr[1])).all() and set(np.unique(count)) == set(range(cr[0], cr[1] + 1))
    assert (nnode <= count).all() and (nnode >= 0).all()
    # the tries table: one entry per antinode drawn, -2 beyond; accepted entries = nnode
    drawn = np.arange(7)[None, :] < count[:, None]
    assert ((tries == -2) == ~drawn).all()
    assert ((tries[drawn] >= -1) & (tries[drawn] < R.MAX_TRIES)).all()
    assert ((tries >= 0).sum(1) == nnode).all()
    valid = np.arange(7)[None, :] < nnode[:, None]
    assert ((nodes[..., 7] == 1.0) == valid).all() and (nodes[~valid] == 0).all()
    cx, cy, a, b, ang, rings, start = (nodes[..., k][valid] for k in range(7))
    assert (nodes[valid] == np.rint(nodes[valid])).all()
    assert (a >= b).all() and (b >= 15).all() and (a <= W // 3).all() and (b <= H // 3).all()
    assert ((ang >= 1) & (ang <= 180)).all()
    assert ((rings >= 1) & (rings <= 11) & (b / rings >= 4)).all()
    assert set(np.unique(start)) == {0.0, 1.0}
    assert ((cx >= a) & (cx <= W - a) & (cy >= b) & (cy <= H - b)).all()
    for f, boxes in enumerate(p["boxes"]):
        assert len(boxes) == nnode[f]
        for i, q in enumerate(boxes):
            # the box the sampler kept is the box of the row it wrote, recomputed here in float64
            rcx, rcy, ra, rb, rang = (float(v) for v in nodes[f, i, :5])
            rad = np.radians(rang)
            dx = np.sqrt(ra ** 2 * np.cos(rad) ** 2 + rb ** 2 * np.sin(rad) ** 2)
            dy = np.sqrt(ra ** 2 * np.sin(rad) ** 2 + rb ** 2 * np.cos(rad) ** 2)
            np.testing.assert_allclose(q, (rcx - dx, rcy - dy, rcx + dx, rcy + dy), rtol=0, atol=1e-3)
            assert q[0] >= 0 and q[1] >= 0 and q[2] <= W and q[3] <= H
            for r in boxes[:i]:
                assert q[2] < r[0] or q[0] > r[2] or q[3] < r[1] or q[1] > r[3], (f, i)


def _frame_stats(waves, node_rows, counts):
    """Per-frame samples of the six statistics: antinode count, mean a, mean b, mean rings (frames with an antinode),
    wave thickness, wave spacing.  Frames are independent draws, antinodes of one frame are not: the standard errors are
    taken over frames."""
    has = [r for r in node_rows if len(r)]
    return {"count": np.asarray(counts, np.float64),
            "a": np.array([np.mean([n[2] for n in r]) for r in has]),
            "b": np.array([np.mean([n[3] for n in r]) for r in has]),
            "rings": np.array([np.mean([n[5] for n in r]) for r in has]),
            "thick": np.asarray([w[2] for w in waves], np.float64),
            "spacing": np.asarray([w[4] for w in waves], np.float64)}


def _host_stats(seeds, cr):
    from spnet_amd import fake_espi as F
    drawn = [F.draw_params(s, cr)[:2] for s in seeds]
    return _frame_stats([d[0] for d in drawn], [d[1] for d in drawn], [len(d[1]) for d in drawn])


def _assert_same_distribution(s1, s2):
    for k in s1:
        x, y = s1[k], s2[k]
        se = np.sqrt(x.var(ddof=1) / len(x) + y.var(ddof=1) / len(y))
        d = abs(x.mean() - y.mean())
        print("%-8s %.4f vs %.4f: difference %.4f, standard error %.4f (%.2f)" % (k, x.mean(), y.mean(), d, se, d / se))
        assert d <= 4 * se, (k, x.mean(), y.mean(), se)


def test_same_distributions_as_the_reference_ordered_stream():
    from spnet_amd import fake_espi as F
    p = R.params(0, N_DIST, seed=0, count_range=(1, 7))
    rows = [[tuple(p["nodes"][f, j, :7]) for j in range(p["nnode"][f])] for f in range(N_DIST)]
    ours = _frame_stats(p["waves"], rows, p["nnode"])
    _assert_same_distribution(ours, _host_stats(F.frame_seeds(N_DIST, 0), (1, 7)))


def test_chunk_independence():
    whole = R.params(0, 100, seed=5)
    first, second = R.params(0, 50, seed=5), R.params(50, 50, seed=5)
    for k in ("waves", "nodes", "nnode", "tries"):
        np.testing.assert_array_equal(whole[k], np.concatenate([first[k], second[k]]))
    other = R.params(0, 50, seed=6)
    assert not np.array_equal(other["nodes"], first["nodes"])
    # a frame index past 2^32 takes the high word into the key
    far = R.params(2 ** 40 - 3, 3, seed=5)
    assert not np.array_equal(far["waves"], R.params(2 ** 32 - 3, 3, seed=5)["waves"])


def test_targets_equal_the_file_path(streams, tmp_path):
    """FakeStream's target path on restated parameters against the CSV round trip, frame by frame and bit for bit; a frame
    with a third ellipse in one grid cell (the file path asserts there) must equal bench.labels_to_Y's 'keep the first
    two'.  The restated stream itself is too well spread to hold such a frame (none among its first 12,000 frames at
    (7, 7) nor at (1, 7)): three hand-placed small ellipses in cell (0, 0) stand in for it."""
    from bench import labels_to_Y
    from spnet_amd import fake_espi as F
    from spnet_amd import utils as U
    n = 300
    p = R.params(0, n, seed=0, count_range=(7, 7))
    labels = F.labels_from_params(p["nodes"], p["nnode"])
    assert [len(r) for r in labels] == p["nnode"].tolist()
    assert all(type(row) is tuple and all(type(v) is int for v in row) for r in labels for row in r)
    crowded = [[(90, 58, 17, 15, 90, 2), (20, 60, 16, 15, 90, 1), (300, 200, 60, 30, 45, 3), (55, 62, 16, 15, 30, 1)],
               [(90, 58, 17, 15, 90, 2), (20, 60, 16, 15, 90, 1), (55, 62, 15, 16, 30, 1), (60, 70, 15, 15, 1, 1)]]
    labels = labels + crowded
    Y, overflow = F.targets_from_labels(labels)
    assert Y.dtype == np.float32 and Y.shape == (n + 2, 576)
    pred_shape = np.array([6, 6, 2, 8])
    csv = tmp_path / "frame.csv"
    for f in range(n + 2):
        csv.write_text(F.rows_to_csv(labels[f]))
        rows = np.array(U.parse_meta_file(str(csv)))
        try:
            want, third = U.norm_Y(U.true_to_pred_grid(rows, pred_shape).flatten()[None])[0].astype(np.float32), False
        except AssertionError:              # true_to_pred_grid: a third ellipse in one cell
            want, third = labels_to_Y([labels[f]])[0], True
        assert bool(overflow[f]) == third == (f >= n), f
        np.testing.assert_array_equal(Y[f], want, err_msg="frame %d" % f)
    # ... and the default stream, whole, against the benchmark's own codec
    p = streams[(1, 7)]
    labels = F.labels_from_params(p["nodes"][:300], p["nnode"][:300])
    Y, overflow = F.targets_from_labels(labels)
    assert not overflow.any()
    np.testing.assert_array_equal(Y, labels_to_Y(labels))
