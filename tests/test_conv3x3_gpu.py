"""The implicit-GEMM passes of block1_conv2 (csrc/conv_gemm.hip: spnet_conv3x3_fwd / _dgrad / _wgrad) against exact integer
sums (tests/helpers/conv3x3_ref.py), behind guards.

Operands are small integers and assert_exact_conv3x3 holds for every case (proved without a GPU by
tests/test_conv3x3_ref_cpu.py, and again here before anything is launched), so every summation order gives the same
integers: each case demands the int64 reference bit for bit.  Every device tensor sits at a 16-byte-aligned offset > 0 of
a larger allocation (dw_ref.place): inputs between NaN -- a read outside the tensor that reaches an output shows as NaN --
outputs and the workspace NaN inside, between sentinel bands that must come back untouched; the workspace holds exactly
spnet_conv3x3_wgrad_ws floats.  There is no tolerance in this file."""
import functools
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import conv3x3_ref as R
from tests.helpers import dw_ref as D
from tests.test_dwconv_gpu import Dev, work

CIN, COUT = R.CIN, R.COUT


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


out = work        # an output: NaN inside, the sentinel before and behind


@functools.lru_cache(maxsize=None)
def case(geom):
    """(x, w, dy) and the int64 results, computed once per geometry"""
    x, w, dy = R.draw(geom)
    R.assert_exact_conv3x3(x, w, dy)
    return x, w, dy, R.fwd(x, w), R.dgrad(dy, w), R.wgrad(x, dy)


def run_fwd(L, x, w, geom):
    B, H, W = geom
    xd, wd, y = Dev(x), Dev(w), out(R.pixels(*geom) * COUT)
    L.spnet_conv3x3_fwd(xd.ptr, wd.ptr, y.ptr, B, H, W, CIN, COUT, st())
    return y


def run_dgrad(L, dy, w, geom):
    B, H, W = geom
    dyd, wd, dx = Dev(dy), Dev(w), out(B * H * W * CIN)
    L.spnet_conv3x3_dgrad(dyd.ptr, wd.ptr, dx.ptr, B, H, W, CIN, COUT, st())
    return dx


def run_wgrad(L, x, dy, geom):
    """(dw, workspace): the workspace holds exactly what spnet_conv3x3_wgrad_ws asks for"""
    B, H, W = geom
    n = int(L.spnet_conv3x3_wgrad_ws(B, H, W, CIN, COUT))
    assert n == R.wgrad_ws(B, H, W)
    xd, dyd, dw, ws = Dev(x), Dev(dy), out(9 * CIN * COUT), work(n)
    L.spnet_conv3x3_wgrad(xd.ptr, dyd.ptr, dw.ptr, B, H, W, CIN, COUT, ws.ptr, n, st())
    return dw, ws


GEOMS = list(R.GEOMETRIES)


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_forward(L, geom):
    x, w, _, y, _, _ = case(geom)
    assert run_fwd(L, x, w, geom).check(y) == []


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_data_gradient(L, geom):
    _, w, dy, _, dx, _ = case(geom)
    assert run_dgrad(L, dy, w, geom).check(dx) == []


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_weight_gradient(L, geom):
    x, _, dy, _, _, dw = case(geom)
    if geom == R.TWO_SLICES:                                  # the case cannot silently stop covering what it is there for
        assert R.split(*geom) == (2, 1152) and R.slices(*geom) == [1152, 1092]
        assert -(-1092 // R.BK) == 35 and 1092 % R.BK == 4
    else:
        assert R.split(*geom)[0] == 1
    got, ws = run_wgrad(L, x, dy, geom)
    assert got.check(dw) == [] and ws.guards() == []
    again, ws2 = run_wgrad(L, x, dy, geom)
    assert np.array_equal(again.host().view(np.uint32), got.host().view(np.uint32))          # values and guards, bit for bit
    assert ws2.guards() == []


def test_weight_gradient_above_the_slice_cap(L):
    """P = 357604 > 170 * 2048: 170 slices of 2112 pixels (the last holds 676).  Operands in [-2, 2]; the reference is the
    helper's tap loop on float32 arrays, which gives the int64 integers under the exactness condition
    (tests/test_conv3x3_ref_cpu.py proves both for this draw and for the equivalence)."""
    geom = R.CAP_GEOMETRY
    assert R.split(*geom) == (170, 2112) and R.wgrad_ws(*geom) == 170 * 9 * CIN * COUT
    x, _, dy = R.draw(geom)
    assert 4 * R.pixels(*geom) < R.LIMIT and max(np.abs(x).max(), np.abs(dy).max()) == R.CAP_VALUE
    t0 = time.perf_counter()
    got, ws = run_wgrad(L, x, dy, geom)
    found = got.check(R.wgrad(x, dy, np.float32)) + ws.guards()
    print("conv3x3 wgrad above the slice cap: GPU run + float32 reference %.2f s" % (time.perf_counter() - t0))
    assert found == []


# ---- structural probes -------------------------------------------------------------------------------------------------------
def test_forward_of_a_single_input_pixel_is_its_nine_weights_mirrored(L):
    geom = R.PROBE_GEOMETRY
    B, H, W = geom
    x, w, _ = R.draw(geom)
    found = []
    for (ih, iw) in R.probe_pixels(H, W):
        v = x[0, ih, iw] + (x[0, ih, iw] == 0)                # no zero channel
        one = R.one_hot((B, H, W, CIN), (0, ih, iw), v)
        found += ["(%d, %d): %s" % (ih, iw, f) for f in run_fwd(L, one, w, geom).check(R.fwd_of_one_pixel(v, w, ih, iw, H, W))]
    assert found == []


def test_data_gradient_of_a_single_pixel_is_its_nine_weights(L):
    geom = R.PROBE_GEOMETRY
    B, H, W = geom
    _, w, dy = R.draw(geom)
    found = []
    for (oh, ow) in R.probe_pixels(H - 2, W - 2):
        g = dy[0, oh, ow] + (dy[0, oh, ow] == 0)
        one = R.one_hot(dy.shape, (0, oh, ow), g)
        found += ["(%d, %d): %s" % (oh, ow, f) for f in run_dgrad(L, one, w, geom).check(R.dgrad_of_one_pixel(g, w, oh, ow, H, W))]
    assert found == []


@pytest.mark.parametrize("geom,at", [((3, 4, 5), (2, 1, 2)), ((3, 4, 5), (1, 0, 0)), ((12, 4, 5), (11, 1, 2)), ((12, 4, 5), (5, 0, 2)),
                                     (R.TWO_SLICES, (0, 16, 64)), (R.TWO_SLICES, (0, 32, 67))],
                         ids=str)
def test_weight_gradient_of_a_single_pixel_is_its_window(L, geom, at):
    """dy zero but for one pixel: dw is that pixel's 3 x 3 x 32 window outer dy.  (3,4,5): the last pixel of the last image
    and the first of the middle one; (12,4,5): the last pixel, 71, in the third K tile, and pixel 32, the first of the second;
    (1,35,70): pixel 1152, the first of the second slice, and the very last, 2243."""
    x, _, dy = R.draw(geom)
    b, oh, ow = at
    if geom == R.TWO_SLICES:
        assert (oh * 68 + ow) in (1152, 2243)
    if geom == (12, 4, 5):
        assert ((b * 2 + oh) * 3 + ow) in (32, 71)
    g = dy[at] + (dy[at] == 0)
    one = R.one_hot(dy.shape, at, g)
    got, ws = run_wgrad(L, x, one, geom)
    assert got.check(R.wgrad_of_one_pixel(x, g, b, oh, ow)) == [] and ws.guards() == []


# ---- rejections --------------------------------------------------------------------------------------------------------------
def test_rejections_launch_nothing(L):
    """every argument set below is refused before anything is launched (hipErrorInvalidValue): valid, aligned pointers to
    tiny buffers, and the sentinel-filled buffer that stands for every output stays untouched.  The 32-bit rules are the
    ones stated above the entry points in csrc/conv_gemm.hip; each geometry is the first past its limit along one axis."""
    z = Dev(np.zeros(4096, np.float32))
    o = Dev(np.full(4096, D.SENTINEL, np.float32), D.SENTINEL)
    s = st()
    X, O = z.ptr, o.ptr
    B, H, W = 1, 5, 7
    big = 1 << 40                                              # a workspace size no rule below can find too small
    fw = lambda B=B, H=H, W=W, ci=CIN, co=COUT, x=X, w=X, y=O: L.spnet_conv3x3_fwd(x, w, y, B, H, W, ci, co, s)
    dg = lambda B=B, H=H, W=W, ci=CIN, co=COUT, dy=X, w=X, dx=O: L.spnet_conv3x3_dgrad(dy, w, dx, B, H, W, ci, co, s)
    wg = lambda B=B, H=H, W=W, ci=CIN, co=COUT, x=X, dy=X, dw=O, ws=O + 1024, n=big: L.spnet_conv3x3_wgrad(x, dy, dw, B, H, W, ci, co, ws, n, s)
    need = R.wgrad_ws(B, H, W)
    table = [
        # forward: x offsets, B*H*W*32 < 2^31
        ("fwd, B*H*W*32 = 2^31", lambda: fw(B=1, H=8192, W=8192)), ("fwd, B*H*W*32 = 2^31 by B", lambda: fw(B=1 << 19, H=8, W=16)),
        # dgrad: dy offsets, B*H*W*64 < 2^31
        ("dgrad, B*H*W*64 = 2^31", lambda: dg(B=1, H=4096, W=8192)), ("dgrad, B*H*W*64 = 2^31 by B", lambda: dg(B=1 << 18, H=8, W=16)),
        # wgrad, dy: (P + 128)*64 <= 2^31.  P = 2^25 exactly (P*64 = 2^31), and P = 2^25 - 127, the first past the limit
        ("wgrad, P*64 = 2^31", lambda: wg(B=2, H=4098, W=4098)), ("wgrad, (P + 128)*64 = 2^31 + 64", lambda: wg(B=5, H=31, W=231411)),
        # wgrad, x: (B + 1 + 127 / (OH*OW))*H*W*32 <= 2^31
        ("wgrad, (B + 1)*H*W*32 = 2^31 + 2^18", lambda: wg(B=1, H=4096, W=8193)),
        ("wgrad, (B + 128)*9*32 = 2^31 + 160", lambda: wg(B=7456413, H=3, W=3)),
    ]
    for name, f in (("fwd", fw), ("dgrad", dg), ("wgrad", wg)):
        table += [(name + ", cin 16", lambda f=f: f(ci=16)), (name + ", cout 32", lambda f=f: f(co=32)), (name + ", cin 64 cout 32", lambda f=f: f(ci=64, co=32)),
                  (name + ", H 2", lambda f=f: f(H=2)), (name + ", W 2", lambda f=f: f(W=2)), (name + ", B 0", lambda f=f: f(B=0)),
                  (name + ", B -1", lambda f=f: f(B=-1))]
    table += [("fwd, x at 4 bytes", lambda: fw(x=X + 4)), ("fwd, w at 4 bytes", lambda: fw(w=X + 4)), ("fwd, y at 4 bytes", lambda: fw(y=O + 4)),
              ("dgrad, dy at 4 bytes", lambda: dg(dy=X + 4)), ("dgrad, w at 4 bytes", lambda: dg(w=X + 4)), ("dgrad, dx at 4 bytes", lambda: dg(dx=O + 4)),
              ("wgrad, x at 4 bytes", lambda: wg(x=X + 4)), ("wgrad, dy at 4 bytes", lambda: wg(dy=X + 4)), ("wgrad, dw at 4 bytes", lambda: wg(dw=O + 4)),
              ("wgrad, workspace at 4 bytes", lambda: wg(ws=O + 1028)),
              ("wgrad, no workspace", lambda: wg(ws=None)), ("wgrad, workspace one float short", lambda: wg(n=need - 1)),
              ("wgrad, workspace of 0 floats", lambda: wg(n=0))]
    # what the table's names claim
    assert 2 * 4096 * 4096 * 64 == 1 << 31 and 3 * 4098 * 4098 * 32 < 1 << 31
    assert (5 * 29 * 231409 + 128) * 64 == (1 << 31) + 64 and 6 * 31 * 231411 * 32 < 1 << 31
    assert 2 * 4096 * 8193 * 32 == (1 << 31) + (1 << 18) and (4094 * 8191 + 128) * 64 < 1 << 31
    assert (7456413 + 128) * 288 == (1 << 31) + 160 and (7456412 + 128) * 288 < 1 << 31 and 7456413 * 288 < 1 << 31
    wrong = []
    for name, call in table:
        try:
            call()
            wrong.append(name + ": no HipError")
        except L.HipError as e:
            if not str(e).endswith("hipError_t 1"):             # hipErrorInvalidValue
                wrong.append(name + ": " + str(e))
        torch.cuda.synchronize()
        if o.check(np.full(o.n, D.SENTINEL)) != []:
            wrong.append(name + ": output written")
            break
    assert wrong == []
