"""Batched warp chain, host side (no GPU needed): the RNG order of draw_warp, the vectorised metadata arithmetic and target
codec against the per-sample three-step path (tests/helpers/warp_chain_ref.py over oracle/warp_ref.py), the rejection rule,
and the numpy restatement of the single-gather kernel against the three image steps."""
import numpy as np
import pytest

from oracle import warp_ref as WR
from spnet_amd import augmentation as A
from spnet_amd import fake_espi
from tests.helpers import warp_chain_ref as R

H, W = 384, 512


def _literal_draw():
    flip = np.random.choice([-2, -1, 0, 1])
    angle = np.random.uniform(-20, 20)
    ti = np.random.randint(10)
    xt = yt = 0
    if ti != 0:
        xt = int(round(40 * (2 * np.random.random() - 1)))
        yt = int(round(40 * (2 * np.random.random() - 1)))
    return int(flip), float(angle), xt, yt, ti


def _seed_with_gate(zero):
    for seed in range(1000):
        np.random.seed(seed)
        if (_literal_draw()[4] == 0) == zero:
            return seed
    raise AssertionError("no seed found")


@pytest.mark.parametrize("zero", [True, False])
def test_draw_warp_consumes_the_rng_like_the_reference_sequence(zero):
    seed = _seed_with_gate(zero)
    np.random.seed(seed)
    want = _literal_draw()
    state_want = np.random.get_state()
    np.random.seed(seed)
    got = A.draw_warp(H, W)
    state_got = np.random.get_state()
    assert got == want[:4]
    assert (want[4] == 0) == zero and ((got[2], got[3]) == (0, 0) or not zero)
    assert state_got[2] == state_want[2] and np.array_equal(state_got[1], state_want[1])


def _params(cases):
    p = A.new_warp_params(list(range(len(cases))), H, W)
    for j, c in enumerate(cases):
        A.set_warp(p, j, *c)
    return p


MD = [[100, 140, 120, 60, 30.0, 7], [400, 300, 50, 20, 170.0, 2], [256, 192, 80, 80, 0.0, 11], [30.5, 370.25, 20, 45, 91.5, 0]]
CASES = [(f, a, xt, yt) for f in (-2, 0, 1, -1) for a in (0, 20.0, -20.0, 3.25, 17.5, -11.125)
         for xt, yt in ((0, 0), (40, -40), (-7, 13))]


def test_warp_metadata_equals_the_three_steps_row_for_row():
    p = _params(CASES)
    rows, count = A.warp_metadata([MD] * len(CASES), p)
    assert rows.shape == (len(CASES), A.MAX_OBJECTS, 6) and (count == len(MD)).all()
    for j, (f, a, xt, yt) in enumerate(CASES):
        want = R.warp_meta(MD, f, a, xt, yt, W, H)
        got = rows[j, :count[j]].tolist()
        assert got == want, (CASES[j], got, want)
    assert not rows[:, len(MD):].any()
    # frames with different object counts in one chunk, one of them empty
    mixed = [MD[:1], [], MD]
    rows, count = A.warp_metadata(mixed, _params(CASES[5:8]))
    for j in range(3):
        assert rows[j, :count[j]].tolist() == R.warp_meta(mixed[j], *CASES[5 + j], W, H)


def test_flip_none_and_angle_zero_leave_rows_untouched():
    md = [[100, 140, 120, 60, 190.0, 7]]            # an angle cleanup_angle would change: the steps must not run at all
    rows, _ = A.warp_metadata([md], _params([(-2, 0.0, 0, 0)]))
    assert rows[0, 0].tolist() == md[0]


def _label_sets(count_range, n=2000, seed=3):
    sets = []
    for s in fake_espi.frame_seeds(n, seed):
        _, nodes, _ = fake_espi.draw_params(int(s), count_range)
        sets.append(sorted([[cx, cy, a, b, float(ang), rings] for cx, cy, a, b, ang, rings, _ in nodes], key=lambda r: (r[0], r[1])))
    return sets


@pytest.mark.parametrize("count_range", [(1, 7), (0, 6)])
def test_warp_targets_equal_the_per_sample_codec(count_range):
    sets = _label_sets(count_range)
    n = len(sets)
    np.random.seed(11)
    cases = [A.draw_warp(H, W) for _ in range(n)]
    p = _params(cases)
    Y, rejected = A.warp_targets(sets, p)
    assert Y.shape == (n, 576) and Y.dtype == np.float32
    outside = 0
    for j in range(n):
        md = R.warp_meta(sets[j], *cases[j], W, H)
        outside += any(not (0 <= r[0] < W and 0 <= r[1] < H) for r in md)
        if rejected[j]:
            with pytest.raises(AssertionError):
                R.targets(md)
            np.testing.assert_array_equal(Y[j], R.targets(sets[j]))
            assert (p["flip"][j], p["angle"][j], p["xt"][j], p["yt"][j]) == (-2, 0.0, 0, 0)
        else:
            np.testing.assert_array_equal(Y[j], R.targets(md))
    print("count_range %s: %d of %d rejected, %d with a centre outside the image" % (count_range, int(rejected.sum()), n, outside))
    assert rejected.sum() <= n // 100            # condition of the issue: at most 1 % rejected
    assert outside > 0                           # frames with a centre outside the image exist and were kept (compared above)


def test_third_ellipse_in_one_cell_is_rejected():
    # cells are 71 x 51 px from (40, 40): two ellipses in cell (2, 2), a third one cell to the left that a shift of +10 brings in
    md = [[190, 150, 30, 20, 10.0, 3], [200, 160, 30, 20, 20.0, 4], [175, 165, 30, 20, 30.0, 5]]
    other = [[100, 100, 30, 20, 10.0, 3]]
    p = _params([(-2, 0.0, 10, 0), (1, 5.0, 3, 4)])
    Y, rejected = A.warp_targets([md, other], p)
    assert rejected.tolist() == [True, False]
    np.testing.assert_array_equal(Y[0], R.targets(md))
    np.testing.assert_array_equal(Y[1], R.targets(R.warp_meta(other, 1, 5.0, 3, 4, W, H)))
    assert (p["flip"][0], p["angle"][0], p["xt"][0], p["yt"][0]) == (-2, 0.0, 0, 0)
    np.testing.assert_array_equal(p["minv"][0], [1, 0, 0, 0, 1, 0])
    assert (p["flip"][1], p["angle"][1], p["xt"][1], p["yt"][1]) == (1, 5.0, 3, 4)


def test_more_than_sixteen_objects_raise():
    md = [[20 + 25 * k, 30 + 20 * k, 10, 5, 1.0, 1] for k in range(17)]
    with pytest.raises(ValueError):
        A.warp_metadata([md], _params([(0, 1.0, 0, 0)]))
    A.warp_metadata([md[:16]], _params([(0, 1.0, 0, 0)]))


def _frames(h, w, n=2, seed=0):
    rs = np.random.RandomState(seed + 31 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([rs.randint(0, 256, (h, w)), 127.5 + 127.5 * np.sin(xx / 9.0 + yy / 23.0) * np.cos(yy / 7.0)][:n]).astype(np.uint8)


@pytest.mark.parametrize("hw", [(96, 128), (17, 23)])
def test_single_gather_restatement_equals_the_three_steps(hw):
    h, w = hw
    X = _frames(h, w)
    cases = [(f, a, xt, yt) for f in (-2, 0, 1, -1) for a in (0, 20.0, -20.0, 3.25)
             for xt, yt in ((0, 0), (9, -5), (-40, 40), (w + 3, 0))]
    p = A.new_warp_params([j % 2 for j in range(len(cases))], h, w)
    for j, c in enumerate(cases):
        A.set_warp(p, j, *c)
    out = A.warp_chain_host(X, p)
    for j, c in enumerate(cases):
        np.testing.assert_array_equal(out[j], R.warp_image(X[j % 2], *c), err_msg=str(c))


def test_shift_is_the_fixed_point_warp_of_a_translation():
    X = _frames(40, 52)[0]
    for xt, yt in ((0, 0), (7, -3), (-40, 12), (60, 0)):
        np.testing.assert_array_equal(R.shift(X, xt, yt), WR.warp_affine_cv2(X[..., None], [[1, 0, xt], [0, 1, yt]])[..., 0])


def test_read_metadata_rows(tmp_path):
    from spnet_amd import utils
    f = tmp_path / "a.csv"
    f.write_text("300,100,20,50,30,4\n100,200,60,30,45.5,0\n300,100,20,50,30,4\n100,150,10,10,0,2\n")
    rows = utils.read_metadata(str(f))
    assert rows == [[100, 150, 10, 10, 0.0, 2], [100, 200, 60, 30, 45.5, 0], [300, 100, 20, 50, 30.0, 4]]
    (tmp_path / "e.csv").write_text("")
    assert utils.read_metadata(str(tmp_path / "e.csv")) == []
