"""The float64 restatement of the device fake-ESPI generator (tests/helpers/espi_raster_ref.py), pinned on the CPU before
tests/test_fake_espi_raster_gpu.py holds spnet_amd/csrc/espi.hip to it pixel by pixel: it rasterises what the oracle's
stroked polylines rasterise (the bounds the device is held to in tests/test_fake_espi_gpu.py), float32 can change it only
within 1e-3 px of a threshold and such pixels are rare, the kernel's four-outline window loses nothing, the labelled ring
count can be read back from its pixels, and its hash is the kernel's."""
import random

import numpy as np
import pytest

from spnet_amd import fake_espi as F
from tests.helpers import espi_raster_ref as R

H, W = F.IM_H, F.IM_W


@pytest.fixture(scope="module")
def drawn():
    """The 12 frames of frame_seeds(12, 5): parameter table, node lists, float64 canvas and margin."""
    (waves, nodes, nn), lists = R.drawn_launch(12, 5)
    canvas, margin = R.canvas_ref(waves, nodes, nn, H, W)
    canvas.setflags(write=False)
    margin.setflags(write=False)
    return (waves, nodes, nn), lists, canvas, margin


def test_reference_meets_the_oracle_bounds_of_the_device_test(drawn):
    from oracle import espi_ref as E
    _, _, canvas, _ = drawn
    seeds = F.frame_seeds(12, 5)[:4]
    ref = [E.frame_params(random.Random(s), np.random.RandomState(s)) for s in seeds]
    oracle = np.stack([E.raster(r[0], r[2]) for r in ref])
    mine = canvas[:4]
    assert set(np.unique(mine)) <= {R.BLACK, R.GREY, R.RING}
    differ = float((mine != oracle).mean())
    print("float64 specification vs oracle raster: canvas pixels that differ: %.2f %%" % (100 * differ))
    assert differ < 0.06
    for v in (R.BLACK, R.GREY, R.RING):
        d = abs(float((mine == v).mean()) - float((oracle == v).mean()))
        print("  area of level %d differs by %.3f %%" % (v, 100 * d))
        assert d < 0.02, v


def test_near_ties_are_rare_in_drawn_frames(drawn):
    _, _, _, margin = drawn
    near = int((margin < R.NEAR_TIE).sum())
    print("drawn frames: %d of %d pixels within %g px of a threshold (%.4f %%)" % (near, margin.size, R.NEAR_TIE, 100.0 * near / margin.size))
    assert near < R.NEAR_TIE_SHARE * margin.size


def test_float32_changes_the_canvas_only_at_near_ties(drawn):
    (waves, nodes, nn), _, canvas, margin = drawn
    win = R.canvas_f32(waves, nodes, nn, H, W, window=True)
    full = R.canvas_f32(waves, nodes, nn, H, W, window=False)
    assert np.array_equal(win, full)                          # the jc-1 .. jc+2 window drops no outline
    differ = win != canvas
    print("float32 (numpy) vs float64: %d pixels differ, all of them near ties" % int(differ.sum()))
    assert not (differ & (margin >= R.NEAR_TIE)).any()


@pytest.mark.parametrize("count_range,seed", [((1, 7), 5), ((0, 6), 4)])
def test_labelled_ring_counts_are_in_the_pixels(drawn, count_range, seed):
    if count_range == (1, 7):
        _, lists, canvas, _ = drawn
    else:
        (waves, nodes, nn), lists = R.drawn_launch(4, seed, count_range)
        assert 0 in nn.tolist() and nn.max() > 0
        canvas, _ = R.canvas_ref(waves, nodes, nn, H, W)
    checked = R.check_labels_in_pixels(canvas, lists)
    assert checked == sum(len(nd) for nd in lists) > 0        # drawn antinodes never overlap: every one is checked


def test_ring_runs_notice_a_miscounted_or_shifted_antinode(drawn):
    """The property has teeth: one outline fewer, or the other start colour, in the pixels fails it."""
    _, lists, _, _ = drawn
    node = next(nd for nd in lists[0] if nd[5] >= 2)
    for wrong in (node[:5] + (node[5] - 1, node[6]), node[:6] + (1 - node[6],)):
        waves, nodes, nn = R.pack([((20.5, 150, 20.5, 0.3, 120.5), [wrong])])
        canvas, _ = R.canvas_ref(waves, nodes, nn, H, W)
        with pytest.raises(AssertionError):
            R.check_labels_in_pixels(canvas, [[node]])
    waves, nodes, nn = R.pack([((20.5, 150, 20.5, 0.3, 120.5), [node])])
    assert R.check_labels_in_pixels(R.canvas_ref(waves, nodes, nn, H, W)[0], [[node]]) == 1


# ------------------------------------------------------------------------------------------------------ crafted launches
def _all_nodes():
    for name in R.CASES:
        _, _, _, nodes, nn = R.case_launch(name)
        for k in range(len(nn)):
            yield name, k, nodes[k], int(nn[k])


def test_crafted_table_covers_the_listed_cases():
    shapes = sorted((h, w) for h, w, _ in R.CASES.values())
    assert shapes == [(1, 64), (24, 520), (37, 331), (40, 300)] and all(len(fr) == 3 for _, _, fr in R.CASES.values())
    live = [(name, k, nd[a]) for name, k, nd, n in _all_nodes() for a in range(n) if nd[a, 7] != 0]
    counts = {n for _, _, _, n in _all_nodes()}
    assert {0, 7} <= counts
    assert any(n >= 3 and any(nd[a, 7] == 0 and nd[a - 1, 7] != 0 and nd[a + 1, 7] != 0 for a in range(1, n - 1)) for _, _, nd, n in _all_nodes())
    assert any(nd[n:, 7].any() for _, _, nd, n in _all_nodes())                      # valid nodes parked past nnode
    assert {(int(nd[5]), int(nd[6])) for _, _, nd in live} >= {(r, s) for r in (0, 1, 5, 11) for s in (0, 1)}
    ratio = [float(np.float32(min(nd[2], nd[3])) / np.float32(max(2 * int(nd[5]), 1))) for _, _, nd in live]
    assert 2.5 in ratio and 3.5 in ratio and min(ratio) < 0.5
    assert np.rint(np.float32(2.5)) == 2 and np.rint(np.float32(3.5)) == 4
    angles = {float(nd[4]) for _, _, nd in live}
    assert {0.0, 90.0, 180.0} <= angles and any(a != int(a) for a in angles)
    assert any(nd[2] == nd[3] for _, _, nd in live)                                   # a circle
    assert any(not (0 <= nd[0] < R.CASES[name][1] and 0 <= nd[1] < R.CASES[name][0]) for name, k, nd in live)
    assert any(nd[0] == int(nd[0]) and nd[1] == int(nd[1]) and 0 <= nd[0] < R.CASES[name][1] and 0 <= nd[1] < R.CASES[name][0]
               for name, k, nd in live)                                               # a pixel exactly at a centre
    waves = [(name, w_) for name in R.CASES for w_ in R.case_launch(name)[2]]
    slopes = [float(w_[3]) for _, w_ in waves]
    assert min(slopes) < 0 and max(slopes) > 0 and 0.0 in slopes
    assert any(w_[4] < w_[2] for _, w_ in waves) and any(w_[4] > R.CASES[name][0] for name, w_ in waves)


def _canvas(name, edit=None):
    H_, W_, waves, nodes, nn = R.case_launch(name)
    if edit is not None:
        nodes, nn = nodes.copy(), nn.copy()
        edit(nodes, nn)
    return R.canvas_ref(waves, nodes, nn, H_, W_)[0]


def test_crafted_cases_show_what_they_are_for():
    """Each branch the table is built for changes the reference canvas: a kernel that ignored it could not equal it."""
    base = _canvas("two_blocks_40x300")

    def count_all(nodes, nn):
        nn[:] = 7
    assert (_canvas("two_blocks_40x300", count_all) != base)[[0, 2]].any(axis=(1, 2)).all()     # slots past nnode

    def revive(nodes, nn):
        nodes[1, 3, 7] = 1.0
    assert (_canvas("two_blocks_40x300", revive) != base)[1].any()                            # the valid = 0 slot

    def half_away(nodes, nn):                        # thickness 3 instead of rint(2.5) = 2: one more pixel of outline
        nodes[2, 0, 3] = 15.01
    assert (_canvas("two_blocks_40x300", half_away) != base)[2].any()
    odd = _canvas("odd_37x331")

    def swap(nodes, nn):
        nodes[2, [0, 1]] = nodes[2, [1, 0]]
    assert (_canvas("odd_37x331", swap) != odd)[2].any()                                      # drawing order of an overlap
    waves_only = _canvas("two_blocks_40x300", lambda nodes, nn: nn.fill(0))
    assert base[1, 19, 20] == R.BLACK and waves_only[1, 19, 20] == R.GREY                     # the pixel AT a centre is painted
    assert (odd[0] == R.GREY).any() and (odd[0] == R.BLACK).mean() > 0.8                      # spacing < thick, holes at j < 0
    three = _canvas("three_blocks_24x520")
    assert (three[0, :, :130] == R.GREY).all() and (three[0, :, 180:230] == R.BLACK).all()    # the line-count bound
    assert (three[0, :, 512:] == R.RING).any() and (three[2, :, 512:] == R.RING).any()        # paint in the last x-block
    assert (_canvas("one_row_1x64") != R.GREY).any(axis=(1, 2)).all()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_crafted_launch_near_ties_and_float32(name):
    H_, W_, waves, nodes, nn = R.case_launch(name)
    canvas, margin = R.canvas_ref(waves, nodes, nn, H_, W_)
    near = int((margin < R.NEAR_TIE).sum())
    print("%s: %d of %d pixels within %g px of a threshold (%.4f %%)" % (name, near, margin.size, R.NEAR_TIE, 100.0 * near / margin.size))
    assert near < R.NEAR_TIE_SHARE * margin.size
    win = R.canvas_f32(waves, nodes, nn, H_, W_, window=True)
    assert np.array_equal(win, R.canvas_f32(waves, nodes, nn, H_, W_, window=False))
    assert not ((win != canvas) & (margin >= R.NEAR_TIE)).any()


# ---------------------------------------------------------------------------------------------------------------- hash
def _hash_int(x):
    m = 0xffffffff
    x ^= x >> 16
    x = (x * 0x7feb352d) & m
    x ^= x >> 15
    x = (x * 0x846ca68b) & m
    x ^= x >> 16
    return x


def test_hash_known_answers():
    known = {0: 0, 1: 0x688990c0, 2: 0xd1132181, 12345: 0x912efcf7, 0x80000000: 0xcc4b4124, 0x9e3779b9: 0x01fce552,
             0xdeadbeef: 0xe628c683, 0xffffffff: 0x6768824a}
    xs = np.array(sorted(known), np.uint32)
    got = R.espi_hash(xs)
    assert got.dtype == np.uint32
    assert [int(v) for v in got] == [known[int(x)] for x in xs] == [_hash_int(int(x)) for x in xs]
    rs = np.random.RandomState(0)
    more = rs.randint(0, 2 ** 32, 1000, dtype=np.uint64).astype(np.uint32)
    assert [int(v) for v in R.espi_hash(more)] == [_hash_int(int(x)) for x in more]


def test_sensor_counter_chain_and_uniform_mapping():
    N, H_, W_, seed = 3, 5, 7, 0xfffffff0                    # a seed that wraps the 32-bit sum
    h1, h2, h3 = R.sensor_hashes(seed, N, H_, W_)
    m = 0xffffffff
    for f, y, x in ((0, 0, 0), (0, 0, 6), (0, 4, 6), (1, 0, 0), (2, 4, 6)):
        pix = (f * H_ + y) * W_ + x
        a = _hash_int((pix * 0x9e3779b9 + seed) & m)
        b = _hash_int(a ^ 0x85ebca6b)
        c = _hash_int((b + 0xc2b2ae35) & m)
        assert (int(h1[f, y, x]), int(h2[f, y, x]), int(h3[f, y, x])) == (a, b, c)
    assert len(np.unique(h1)) == h1.size                                        # no counter value twice in a launch
    mask, _, _ = R.sensor_ref(np.zeros((N, H_, W_), np.uint8), seed, H_, W_)
    assert np.array_equal(mask, ((h3 >> np.uint32(16)) & np.uint32(1)).astype(bool))
    ends = np.array([0, 0xff, 0x100, 0xffffffff], np.uint32)
    u1, u2 = R.uniforms(ends, ends)
    assert u1.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]            # (0, 1]: log(u1) is finite and <= 0
    assert u2.tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]             # [0, 1)
    _, noisy, n = R.sensor_ref(np.full((1, 1, 4), 128, np.uint8), 7, 1, 4)
    assert np.isfinite(n).all() and noisy.dtype == np.uint8 and (noisy >= 128).all()
