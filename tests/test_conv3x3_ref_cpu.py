"""tests/helpers/conv3x3_ref.py and the cases of tests/test_conv3x3_gpu.py, without a GPU: the tap-by-tap reference agrees
with the oracle convolution and its autograd (float64), forward and data gradient are adjoints exactly, the split mirror
gives the hand-computed slices, and every operand set the GPU tests draw is exact in fp32 (assert_exact_conv3x3)."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as T
from tests.helpers import conv3x3_ref as R
from tests.helpers import gemm_ref as G


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


@pytest.mark.parametrize("B,H,W", [(2, 3, 3), (1, 4, 6), (2, 7, 5)])
def test_reference_against_the_oracle(B, H, W):
    rs = np.random.RandomState(H * W)
    x, w = t64(rs.randn(B, H, W, 8), True), t64(rs.randn(3, 3, 8, 12), True)
    y = T.conv2d(x, w, 1, "valid")
    dy = rs.randn(*y.shape)
    y.backward(t64(dy))
    xn, wn = x.detach().numpy(), w.detach().numpy()
    assert np.allclose(R.fwd(xn, wn, np.float64), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.dgrad(dy, wn, np.float64), x.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.wgrad(xn, dy, np.float64), w.grad.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("geom", [(1, 3, 3), (3, 4, 5), (2, 3, 34)], ids=str)
def test_forward_and_data_gradient_are_adjoints(geom):
    """<y, dy> == <x, dx> == <w, dw>, exactly, in int64"""
    x, w, dy = R.draw(geom)
    a = int((R.fwd(x, w) * G.as_int(dy)).sum())
    assert a == int((G.as_int(x) * R.dgrad(dy, w)).sum()) == int((G.as_int(w) * R.wgrad(x, dy)).sum())
    assert a != 0


def test_split_mirror_against_hand_computed_values():
    # P = 1: one slice, one K tile.  2048: still one slice.  2049: two slabs, ceil(2049/2) = 1025 -> 1056.
    # 2244: 1122 -> 1152 (and 1092 = 34 * 32 + 4 left).  357604: 175 slices wanted, 170 allowed; 2103.6 -> 2104 -> 2112 = 66 * 32;
    # 169 * 2112 = 356928 < 357604: all 170 slices are in use, the last holds 676 pixels
    table = {(1, 3, 3): (1, 1, 32), (1, 34, 66): (2048, 1, 2048), (1, 5, 685): (2049, 2, 1056), (1, 35, 70): (2244, 2, 1152),
             (1, 600, 600): (357604, 170, 2112)}
    for geom, (P, ns, p_chunk) in table.items():
        assert R.pixels(*geom) == P
        assert R.split(*geom) == (ns, p_chunk), geom
        assert sum(R.slices(*geom)) == P and len(R.slices(*geom)) == ns
    assert R.wgrad_ws(1, 3, 3) == 18432 and R.wgrad_ws(1, 5, 685) == 2 * 18432 and R.wgrad_ws(*R.CAP_GEOMETRY) == 170 * 18432
    assert R.slices(*R.TWO_SLICES) == [1152, 1092] and R.slices(*R.CAP_GEOMETRY)[-1] == 676
    # rounding p_chunk up can empty the last slabs.  P = 170 * 2048 + 1: 2049 pixels per slab -> 2080, which 168 slices cover
    assert R.pixels(1, 3, 348163) == 348161 and R.split(1, 3, 348163) == (168, 2080) and R.wgrad_ws(1, 3, 348163) == 170 * 18432


def test_geometries_are_what_the_table_says():
    for (B, H, W) in R.GEOMETRIES:
        assert H >= 3 and W >= 3 and B >= 1
    assert R.pixels(1, 3, 3) == 1
    assert (2 * 1 * 32) % R.BK == 0 and R.pixels(2, 3, 34) == 64
    assert R.pixels(2, 10, 18) == 2 * R.BM_FWD and R.pixels(1, 3, 131) == R.BM_FWD + 1
    assert 1 * 8 * 16 == R.BM_DGRAD
    n = R.slices(*R.TWO_SLICES)
    tiles = [-(-v // R.BK) for v in n]
    assert tiles == [36, 35] and n[1] - 34 * R.BK == 4
    assert R.pixels(*R.CAP_GEOMETRY) > R.SLICE_CAP * R.SLICE_PIXELS
    assert R.pixels(3, 4, 5) < R.BK < R.pixels(40, 3, 3) and R.pixels(12, 4, 5) == 2 * R.BK + 8


@pytest.mark.parametrize("geom", list(R.GEOMETRIES) + [R.PROBE_GEOMETRY, R.CAP_GEOMETRY], ids=str)
def test_every_drawn_operand_set_is_exact(geom):
    x, w, dy = R.draw(geom)
    b = R.assert_exact_conv3x3(x, w, dy)
    assert 0 < max(b.values()) < R.LIMIT
    v = R.CAP_VALUE if geom == R.CAP_GEOMETRY else R.VALUE
    for a in (x, w, dy):                                      # the whole range is drawn, zero included
        assert a.dtype == np.float32 and set(np.unique(a)) == set(range(-v, v + 1))


def test_exactness_check_refuses_what_is_not_exact():
    x, w, dy = R.draw((1, 35, 70))
    with pytest.raises(AssertionError):
        R.assert_exact_conv3x3(x * 100, w, dy * 100)           # weight gradient: 2244 pixels of up to 300 * 300
    with pytest.raises(AssertionError):
        R.assert_exact_conv3x3(x * 1000, w * 1000, dy)
    with pytest.raises(ValueError):
        R.assert_exact_conv3x3(x + 0.5, w, dy)


def test_float32_tap_loop_equals_int64_under_the_condition():
    """the case above the slice cap takes its reference from the float32 tap loop: same integers as int64"""
    x, w, dy = R.draw(R.TWO_SLICES)
    R.assert_exact_conv3x3(x, w, dy)
    for got, want in ((R.wgrad(x, dy, np.float32), R.wgrad(x, dy)), (R.fwd(x, w, np.float32), R.fwd(x, w)),
                      (R.dgrad(dy, w, np.float32), R.dgrad(dy, w))):
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.astype(np.float64), want.astype(np.float64))


def test_probe_layouts_are_the_convolution_of_a_one_hot():
    B, H, W = R.PROBE_GEOMETRY
    x, w, dy = R.draw(R.PROBE_GEOMETRY)
    for (ih, iw) in R.probe_pixels(H, W):
        one = R.one_hot((B, H, W, R.CIN), (0, ih, iw), x[0, ih, iw] + (x[0, ih, iw] == 0))
        np.testing.assert_array_equal(R.fwd(one, w)[0], R.fwd_of_one_pixel(one[0, ih, iw], w, ih, iw, H, W))
    for (oh, ow) in R.probe_pixels(H - 2, W - 2):
        one = R.one_hot(dy.shape, (0, oh, ow), dy[0, oh, ow])
        np.testing.assert_array_equal(R.dgrad(one, w)[0], R.dgrad_of_one_pixel(dy[0, oh, ow], w, oh, ow, H, W))
        np.testing.assert_array_equal(R.wgrad(x, one), R.wgrad_of_one_pixel(x, dy[0, oh, ow], 0, oh, ow))
