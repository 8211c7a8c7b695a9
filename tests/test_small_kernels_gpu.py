"""The small kernels around the backbone, one by one through the C ABI: the fused stem head, block1_conv1, the grid-stride
trips of the elementwise stem convolutions, the ellipse loss, SelectiveSigmoid, decode, min/max + cutout + salt & pepper,
and dropout -- at the shapes that reach their loops, caps and edge branches.

Every output buffer is pre-filled with NaN (in-place cases with the input) and followed by a 4 KiB guard band that must
stay NaN.  Every comparison takes one of three forms, named in the comment next to it:
  (1) bit equality, where the code claims it or the operation is a copy / select;
  (2) exact-sum inputs: small integer-valued operands, every partial sum an integer below 2^24, so any summation order
      gives exactly the float64 result -- one dropped or doubled pixel among a million shows;
  (3) a forward-error bound against the float64 reference (tests/helpers/small_kernels_ref.py, oracle/): for a sum of n
      fp32 products |got - want| <= (n + 2) * 2^-24 * sum|terms|, sum|terms| from the same reference run on absolute
      values, n counted from the kernel's own chain of roundings.
expf / log1pf / atan2f results take the rtol / atol test_ellipse_loss and test_decode of test_kernels_gpu.py use."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import numpy_ref as R
from oracle import torch_ref as T
from tests.helpers import small_kernels_ref as S


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def st():
    return torch.cuda.current_stream().cuda_stream


def close(got, want, rtol, atol):
    np.testing.assert_allclose(got.detach().cpu().double().numpy(), np.asarray(want, np.float64), rtol=rtol, atol=atol)


NAN = float("nan")
U = 2.0 ** -24            # unit roundoff of fp32
GUARD = 1024              # floats behind every output: 4 KiB that must stay NaN
WS = 1024 * 1024          # workspace floats: >= 768 * 864 (block1_conv1 weight gradient), >= 512 * 81


def idev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def guarded(shape, init=None):
    """(buffer, view): `view` has `shape` and is NaN (or a copy of `init`), the GUARD floats behind it are NaN."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), NAN, device="cuda")
    view = buf[:n].view(shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def guard_untouched(buf):
    return bool(torch.isnan(buf[buf.numel() - GUARD:]).all())


def within(got, want, sum_abs, n, what, floor=0.0):
    """form (3): |got - want| <= (n + 2) * 2^-24 * sum|terms| (+ floor) elementwise (a NaN in `got` fails); prints the
    margin."""
    got = got.detach().double().cpu()
    want = torch.as_tensor(want, dtype=torch.float64).cpu().reshape(got.shape)
    bound = (n + 2) * U * torch.as_tensor(sum_abs, dtype=torch.float64).cpu().reshape(got.shape) + floor
    err = (got - want).abs()
    used = float((err / bound.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max()) if err.numel() else 0.0
    print("%s: largest error %.3e, largest share of the bound %.3f (n = %d)" % (what, float(err.nan_to_num(nan=float("inf")).max()), used, n))
    assert bool((err <= bound).all()), what


def ints(shape, lo, hi, seed):
    """integer-valued fp32 in [lo, hi], drawn on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()


# ============================================================================================ 1. stem head, forward
STEM_SHAPES = [(2, 8, 12), (1, 9, 11), (2, 2, 2), (1, 3, 5), (1, 331, 331)]


def _unfused_stem_head(L, xd, wd, B, H, W):
    """spnet_conv3x3_small (1 -> 3, 'same') + spnet_avgpool2_fwd, and spnet_avgpool2_fwd of the frame"""
    c = torch.full((B, H, W, 3), NAN, device="cuda")
    L.spnet_conv3x3_small(0, 1, 3, 1, 1, xd.data_ptr(), wd.data_ptr(), c.data_ptr(), B, H, W, None, 0, st())
    q1 = torch.full((B, H // 2, W // 2, 3), NAN, device="cuda")
    qx = torch.full((B, H // 2, W // 2), NAN, device="cuda")
    L.spnet_avgpool2_fwd(c.data_ptr(), q1.data_ptr(), B, H, W, 3, st())
    L.spnet_avgpool2_fwd(xd.data_ptr(), qx.data_ptr(), B, H, W, 1, st())
    return q1, qx


@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_stem_head_forward(L, B, H, W):
    """Odd H / W drop the last row / column (the 331 x 331 reference layout); (2,2,2) is one pooled pixel per frame whose
    whole window border is padding."""
    rs = np.random.RandomState(H * 7 + W)
    x, w = rs.randn(B, H, W).astype(np.float32), (rs.randn(3, 3, 1, 3) * 0.3).astype(np.float32)
    xd, wd = dev(x), dev(w)
    b1, p1 = guarded((B, H // 2, W // 2, 3))
    bx, px = guarded((B, H // 2, W // 2))
    L.spnet_stem_head(0, xd.data_ptr(), wd.data_ptr(), p1.data_ptr(), px.data_ptr(), B, H, W, None, 0, st())
    q1, qx = _unfused_stem_head(L, xd, wd, B, H, W)
    assert torch.equal(p1, q1) and torch.equal(px, qx)              # (1) the kernel's comment: the unfused pair's bits
    assert guard_untouched(b1) and guard_untouched(bx)
    xt, wt = torch.from_numpy(x), torch.from_numpy(w)
    r1, rx = S.stem_head_fwd(xt, wt)
    a1, ax = S.stem_head_fwd(xt.abs(), wt.abs())
    within(p1, r1, a1, 13, "p1")        # (3) 9 taps + 3 adds + 1 scale
    within(px, rx, ax, 4, "px")         # (3) 3 adds + 1 scale


def test_stem_head_forward_beyond_the_grid_cap(L):
    """3 x 850 x 850 = 2,167,500 pooled pixels > 8192 x 256 threads: the grid-stride loop makes a second trip."""
    B, H, W = 3, 1700, 1700
    assert B * (H // 2) * (W // 2) > 8192 * 256
    xd = ints((B, H, W), -2, 2, 1)
    wd = ints((3, 3, 1, 3), -8, 8, 2) / 8.0
    b1, p1 = guarded((B, H // 2, W // 2, 3))
    bx, px = guarded((B, H // 2, W // 2))
    L.spnet_stem_head(0, xd.data_ptr(), wd.data_ptr(), p1.data_ptr(), px.data_ptr(), B, H, W, None, 0, st())
    r1, rx = S.stem_head_fwd(xd, wd)
    # (2) |x| <= 2, |w| <= 1 in eighths: a conv output is a sum of 9 terms <= 2 (<= 18), a pooled cell <= 72 before the
    # exact * 0.25; everything a multiple of 1/32 far below 2^24 / 32
    assert torch.equal(p1.double(), r1) and torch.equal(px.double(), rx)
    assert guard_untouched(b1) and guard_untouched(bx)


# ============================================================================================ 2. stem head, weight gradient
@pytest.mark.parametrize("B,H,W", STEM_SHAPES)
def test_stem_head_weight_gradient(L, B, H, W):
    rs = np.random.RandomState(H * 5 + W)
    OH, OW = H // 2, W // 2
    x, dp = rs.randn(B, H, W).astype(np.float32), rs.randn(B, OH, OW, 3).astype(np.float32)
    xd, dpd = dev(x), dev(dp)
    ws = torch.empty(512 * 27, device="cuda")
    outs = []
    for _ in range(2):
        bw, dw = guarded((3, 3, 1, 3))
        L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, H, W, ws.data_ptr(), ws.numel(), st())
        assert guard_untouched(bw)
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])                            # (1) deterministic: two calls, the same bits
    xt, dpt = torch.from_numpy(x), torch.from_numpy(dp)
    within(outs[0], S.stem_head_wgrad(xt, dpt), S.stem_head_wgrad(xt.abs(), dpt.abs()), B * OH * OW, "dw")   # (3) n = pooled pixels


def test_stem_head_weight_gradient_beyond_the_parts_cap(L):
    """3 x 600 x 600 = 1,080,000 pooled pixels > 512 x 2048: the workgroup count is capped at 512 and every thread makes
    more than eight trips."""
    B, H, W = 3, 1200, 1200
    assert B * (H // 2) * (W // 2) > 512 * 2048
    xd = ints((B, H, W), -2, 2, 3)
    dpd = ints((B, H // 2, W // 2, 3), -1, 1, 4) * 4.0
    ws = torch.empty(512 * 27, device="cuda")
    outs = []
    for _ in range(2):
        bw, dw = guarded((3, 3, 1, 3))
        L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, H, W, ws.data_ptr(), ws.numel(), st())
        assert guard_untouched(bw)
        outs.append(dw)
    assert torch.equal(outs[0], outs[1])                            # (1)
    # (2) a term is (sum of four x, <= 8) * (0.25 * dp, in {-1, 0, 1}): the largest partial sum is 8 * 1,080,000 =
    # 8,640,000 < 2^24
    ref = S.stem_head_wgrad(xd, dpd)
    assert float(ref.abs().max()) > 0 and torch.equal(outs[0].double(), ref)


def test_stem_head_rejects(L):
    """Every refused call returns HipError and writes nothing."""
    B, H, W = 1, 331, 331                       # 27,225 pooled pixels -> 14 workgroups -> 378 workspace floats
    xd, dpd = ints((B, H, W), -2, 2, 5), ints((B, H // 2, W // 2, 3), -1, 1, 6)
    wd = ints((3, 3, 1, 3), -2, 2, 7)
    ws = torch.empty(512 * 27, device="cuda")
    bw, dw = guarded((3, 3, 1, 3))
    b1, p1 = guarded((B, H // 2, W // 2, 3))
    bx, px = guarded((B, H // 2, W // 2))
    with pytest.raises(L.HipError):             # workspace one float too small
        L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, H, W, ws.data_ptr(), 14 * 27 - 1, st())
    with pytest.raises(L.HipError):             # ... at a single workgroup
        L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, 1, 8, 12, ws.data_ptr(), 26, st())
    with pytest.raises(L.HipError):             # no workspace
        L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, H, W, None, 512 * 27, st())
    with pytest.raises(L.HipError):             # there is no data gradient
        L.spnet_stem_head(1, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, H, W, ws.data_ptr(), ws.numel(), st())
    with pytest.raises(L.HipError):             # forward without the skip output
        L.spnet_stem_head(0, xd.data_ptr(), wd.data_ptr(), p1.data_ptr(), None, B, H, W, None, 0, st())
    for h, w_ in ((1, 12), (12, 1)):            # nothing to pool
        with pytest.raises(L.HipError):
            L.spnet_stem_head(0, xd.data_ptr(), wd.data_ptr(), p1.data_ptr(), px.data_ptr(), B, h, w_, None, 0, st())
        with pytest.raises(L.HipError):
            L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, h, w_, ws.data_ptr(), ws.numel(), st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(bw).all()) and bool(torch.isnan(b1).all()) and bool(torch.isnan(bx).all())
    L.spnet_stem_head(2, xd.data_ptr(), dpd.data_ptr(), dw.data_ptr(), None, B, H, W, ws.data_ptr(), 14 * 27, st())   # exactly enough
    # (2) a term is (sum of four x, <= 8) * (0.25 * dp): in quarters, the largest partial sum is 8 * 27,225 < 2^24
    assert torch.equal(dw.double(), S.stem_head_wgrad(xd, dpd))


# ============================================================================================ 3. block1_conv1 (3 -> 32, stride 2, valid)
def _conv1_call(L, op, a, b, out, B, H, W, ws):
    L.spnet_conv3x3_small(op, 3, 32, 2, 0, a.data_ptr(), b.data_ptr(), out.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), st())


@pytest.mark.parametrize("B,H,W", [(2, 21, 29), (1, 165, 165), (2, 7, 67)])
def test_block1_conv1(L, B, H, W):
    """Odd widths: the last 2 x 2 block of a row of the data gradient is half outside (the scalar tail), and with
    (b*H + h) odd the six-float stores of the others start at an odd float offset.  165 is the plane the 331 layout
    feeds this layer; (2, 7, 67) has two tiles across and a last tile one output wide."""
    rs = np.random.RandomState(H + W)
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    xd, wd, dyd = dev(rs.randn(B, H, W, 3)), dev(rs.randn(3, 3, 3, 32) * 0.3), dev(rs.randn(B, OH, OW, 32))
    x = xd.cpu().double().requires_grad_(True)                      # float64 oracle on the fp32 values the device gets
    w, dy = wd.cpu().double(), dyd.cpu().double()
    y = T.conv2d(x, w, 2, "valid")
    y.backward(dy)
    xa = x.detach().abs().requires_grad_(True)                      # the same on absolute values: sum|terms|
    ya = T.conv2d(xa, w.abs(), 2, "valid")
    ya.backward(dy.abs())
    ws = torch.empty(WS, device="cuda")
    by, yd = guarded((B, OH, OW, 32))
    _conv1_call(L, 0, xd, wd, yd, B, H, W, ws)
    assert guard_untouched(by)
    within(yd, y.detach(), ya.detach(), 27, "y")                    # (3) 27 fmaf
    bx, dxd = guarded((B, H, W, 3))
    _conv1_call(L, 1, dyd, wd, dxd, B, H, W, ws)
    assert guard_untouched(bx)
    within(dxd, x.grad, xa.grad, 128, "dx")                         # (3) at most 4 taps x 32 channels reach a pixel
    # weight gradient (2): |x|, |dy| <= 2, a term <= 4, the largest partial sum 4 * B*OH*OW (<= 26,896 here)
    xi, dyi = ints((B, H, W, 3), -2, 2, 8), ints((B, OH, OW, 32), -2, 2, 9)
    wr = torch.zeros(3, 3, 3, 32, dtype=torch.float64, requires_grad=True)
    T.conv2d(xi.cpu().double(), wr, 2, "valid").backward(dyi.cpu().double())
    bw, dwd = guarded((3, 3, 3, 32))
    _conv1_call(L, 2, xi, dyi, dwd, B, H, W, ws)
    assert guard_untouched(bw)
    assert torch.equal(dwd.cpu().double(), wr.grad)


def test_block1_conv1_weight_gradient_walks_its_tiles(L):
    """4 x 25 x 8 = 800 tiles of 4 x 32 outputs > 768 workgroups: the first 32 workgroups take a second tile through the
    grid-stride loop (and its leading barrier)."""
    B, H, W = 4, 201, 513
    OH, OW = 100, 256
    assert B * ((OH + 3) // 4) * ((OW + 31) // 32) == 800
    xi, dyi = ints((B, H, W, 3), -2, 2, 10), ints((B, OH, OW, 32), -2, 2, 11)
    wr = torch.zeros(3, 3, 3, 32, dtype=torch.float64, requires_grad=True)
    T.conv2d(xi.cpu().double(), wr, 2, "valid").backward(dyi.cpu().double())
    ws = torch.empty(WS, device="cuda")
    outs = []
    for _ in range(2):
        bw, dwd = guarded((3, 3, 3, 32))
        _conv1_call(L, 2, xi, dyi, dwd, B, H, W, ws)
        assert guard_untouched(bw)
        outs.append(dwd)
    assert torch.equal(outs[0], outs[1])                            # (1)
    # (2) a term <= 4, 102,400 output pixels: the largest partial sum is 409,600 < 2^24
    assert torch.equal(outs[0].cpu().double(), wr.grad)
    with pytest.raises(L.HipError):                                 # 768 partial filters do not fit
        L.spnet_conv3x3_small(2, 3, 32, 2, 0, xi.data_ptr(), dyi.data_ptr(), outs[0].data_ptr(), B, H, W, ws.data_ptr(),
                              768 * 864 - 1, st())


# ============================================================================================ 4. the elementwise grid cap
@pytest.mark.parametrize("cin,B,H,W", [(1, 2, 1030, 1021), (3, 2, 1030, 1021), (3, 2, 2050, 2048)])
def test_stem_convs_beyond_the_grid_cap(L, cin, B, H, W):
    """spnet_ew_grid caps a grid at 8192 workgroups of 256: one thread per pixel makes a second trip above 2,097,152
    pixels (W % 4 != 0, and the 1 -> 3 layer at any width), the runs-of-four kernel (3 -> 3, W % 4 == 0) above four times
    as many."""
    per_thread = 4 if (cin == 3 and W % 4 == 0) else 1
    assert B * H * W > 8192 * 256 * per_thread
    wd = ints((3, 3, cin, 3), -2, 2, 12)
    # (2) |x|, |w| <= 2: an output is a sum of at most 27 terms <= 4
    xd = ints((B, H, W, cin), -2, 2, 13)
    by, yd = guarded((B, H, W, 3))
    L.spnet_conv3x3_small(0, cin, 3, 1, 1, xd.data_ptr(), wd.data_ptr(), yd.data_ptr(), B, H, W, None, 0, st())
    assert guard_untouched(by)
    assert torch.equal(yd.double(), S.conv3x3_same(xd, wd))
    del by, yd, xd
    dyd = ints((B, H, W, 3), -2, 2, 14)
    bx, dxd = guarded((B, H, W, cin))
    L.spnet_conv3x3_small(1, cin, 3, 1, 1, dyd.data_ptr(), wd.data_ptr(), dxd.data_ptr(), B, H, W, None, 0, st())
    assert guard_untouched(bx)
    assert torch.equal(dxd.double(), S.conv3x3_same_dgrad(dyd, wd))


# ============================================================================================ 5. ellipse loss
def _loss_inputs(B, ncols, seed, noobj="mixed"):
    rs = np.random.RandomState(seed)
    yt, yp = (rs.randn(B, ncols) * 0.5).astype(np.float32), (rs.randn(B, ncols) * 0.5).astype(np.float32)
    yt[:, 6::8] = {"mixed": (rs.rand(B, ncols // 8) < 0.5), "ones": 1.0, "zeros": 0.0}[noobj]
    return yt, yp


def _loss_grad_abs(yt, yp, loss_type):
    """R.loss_grad with every difference replaced by the sum of the absolute values of its operands: sum|terms| of (3)"""
    t, y = np.abs(yt.astype(np.float64)), np.abs(yp.astype(np.float64))
    B, n = y.shape
    o = np.repeat(1 + t[:, 6::8], 8, axis=1)
    d2 = np.repeat((t[:, 2::8] + t[:, 3::8]) ** 2, 8, axis=1)
    w = np.tile(np.array([R.L_CENTER, R.L_CENTER, R.L_SIZE, R.L_SIZE, R.L_ANGLE, R.L_ANGLE, 0.0, R.L_CLASS]), n // 8)[None, :] * o
    w[:, 4::8] *= d2[:, 4::8]
    w[:, 5::8] *= d2[:, 5::8]
    w[:, 6::8] = R.L_NOOBJ
    a = 2.0 * w * (t + y)
    if loss_type != "same":
        a[:, 6::8] = R.L_NOOBJ * (1.0 / (1.0 + np.exp(-yp[:, 6::8].astype(np.float64))) + t[:, 6::8])
    return a / (n * B)


def _run_loss(L, yt, yp, loss_type, with_grad=True):
    B, ncols = yt.shape
    ytd, ypd = dev(yt), dev(yp)
    bg, g = guarded((B, ncols))
    bp, parts = guarded((B, 5))
    bo, out = guarded((6,))
    L.spnet_ellipse_loss(ytd.data_ptr(), ypd.data_ptr(), g.data_ptr() if with_grad else None, parts.data_ptr(), out.data_ptr(),
                         B, ncols, 0 if loss_type == "same" else 1, st())
    assert guard_untouched(bp) and guard_untouched(bo)
    assert guard_untouched(bg) if with_grad else bool(torch.isnan(bg).all())     # grad == NULL: the stand-in stays NaN
    return out, g


def _check_loss(L, yt, yp, loss_type):
    out, g = _run_loss(L, yt, yp, loss_type)
    total, parts = R.loss_terms(yt, yp, loss_type)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(g).all())
    close(out[:5], parts, rtol=1e-5, atol=1e-9)                     # test_ellipse_loss's tolerance (expf / log1pf inside)
    close(out[5], total, rtol=1e-5, atol=1e-9)
    # (3) the longest chain of a gradient entry: the difference, 1 - noobj, a - b and its square, 1 / (ncols * B) (two
    # roundings), and four products -- or expf (two units), 1 + e, the division, the difference and three products
    # The relative model of (3) holds for normal numbers only: sigmoid(-90) = 8e-40 lies below the smallest normal fp32,
    # 2^-126 (expf(90) overflows and the quotient is 0), so that much absolute error is the format's own.
    within(g, R.loss_grad(yt, yp, loss_type), _loss_grad_abs(yt, yp, loss_type), 10, "grad", floor=2.0 ** -126)
    return out, g


@pytest.mark.parametrize("loss_type", ["same", "hybrid"])
@pytest.mark.parametrize("B", [1, 4, 65, 130])
@pytest.mark.parametrize("ncols", [8, 520, 576, 1024])
def test_ellipse_loss_shapes(L, B, ncols, loss_type):
    """B > 64: the finalize kernel's lanes take a second (130: third) sample; ncols 8 leaves 63 lanes idle, 520 = 65
    predictors gives lane 0 two and the others one, 1024 two each."""
    yt, yp = _loss_inputs(B, ncols, B + ncols)
    out, _ = _check_loss(L, yt, yp, loss_type)
    out2, _ = _run_loss(L, yt, yp, loss_type, with_grad=False)      # the models.py path
    assert torch.equal(out, out2)                                   # (1)


@pytest.mark.parametrize("loss_type", ["same", "hybrid"])
def test_ellipse_loss_without_objects_and_with_one_in_every_cell(L, loss_type):
    B, ncols = 5, 576
    yt, yp = _loss_inputs(B, ncols, 1, "ones")
    out, g = _check_loss(L, yt, yp, loss_type)
    objcols = torch.ones(ncols, dtype=torch.bool)
    objcols[6::8] = False
    assert bool((g[:, objcols.cuda()] == 0).all())                  # (1) 1 - noobj is exactly 0
    assert bool((out[[0, 1, 2, 4]] == 0).all()) and float(out[3]) == float(out[5])
    yt, yp = _loss_inputs(B, ncols, 2, "zeros")
    _check_loss(L, yt, yp, loss_type)


def test_ellipse_loss_hybrid_saturated_logits(L):
    """|z| of 20 and 90: expf(-|z|) vanishes against 1, expf(90) overflows to infinity inside the sigmoid."""
    B, ncols = 4, 576
    yt, yp = _loss_inputs(B, ncols, 3)
    z = np.array([-90.0, -20.0, 0.0, 20.0, 90.0], np.float32)
    yp[:, 6::8] = z[(np.arange(B)[:, None] * 3 + np.arange(ncols // 8)[None, :]) % 5]
    for col in range(5):                                            # each logit against both labels
        assert {0.0, 1.0} <= set(yt[:, 6::8][yp[:, 6::8] == z[col]].tolist())
    _check_loss(L, yt, yp, "hybrid")


def test_ellipse_loss_rejects(L):
    yt, yp = _loss_inputs(2, 16, 4)
    ytd, ypd = dev(yt), dev(yp)
    bp, parts = guarded((2, 5))
    bo, out = guarded((6,))
    with pytest.raises(L.HipError):
        L.spnet_ellipse_loss(ytd.data_ptr(), ypd.data_ptr(), None, parts.data_ptr(), out.data_ptr(), 2, 12, 0, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(bp).all()) and bool(torch.isnan(bo).all())


# ============================================================================================ 6. SelectiveSigmoid
@pytest.mark.parametrize("B,ncols,start,step", [(3, 576, 6, 8), (1, 7, 0, 1), (5, 576, 575, 8), (2, 20, 3, 7)])
def test_selective_sigmoid(L, B, ncols, start, step):
    rs = np.random.RandomState(ncols + start)
    y0 = (rs.randn(B, ncols) * 3).astype(np.float32)
    y0[0, start] = 100.0
    y0[B - 1, start + ((ncols - start - 1) // step) * step] = -100.0 if (B > 1 or ncols - start > step) else 100.0
    g0 = rs.randn(B, ncols).astype(np.float32)
    sel = np.zeros(ncols, bool)
    sel[start::step] = True
    by, y = guarded((B, ncols), dev(y0))
    L.spnet_selective_sigmoid(y.data_ptr(), None, B, ncols, start, step, 0, st())
    assert guard_untouched(by)
    yn = y.cpu().numpy()
    assert np.array_equal(yn[:, ~sel].view(np.uint32), y0[:, ~sel].view(np.uint32))       # (1) other columns untouched
    assert np.isfinite(yn).all() and yn[0, start] == 1.0
    close(y, S.selective_sigmoid_fwd(y0, start, step), rtol=1e-5, atol=1e-9)              # expf: test_ellipse_loss's
    # backward on the post-sigmoid output
    bg, g = guarded((B, ncols), dev(g0))
    L.spnet_selective_sigmoid(y.data_ptr(), g.data_ptr(), B, ncols, start, step, 1, st())
    assert guard_untouched(bg) and guard_untouched(by)
    assert torch.equal(y.cpu(), torch.from_numpy(yn))                                     # (1) y is only read
    gn = g.cpu().numpy()
    assert np.array_equal(gn[:, ~sel].view(np.uint32), g0[:, ~sel].view(np.uint32))       # (1)
    s64, a64 = yn.astype(np.float64), np.abs(g0.astype(np.float64))
    a64[:, sel] *= np.abs(s64[:, sel]) * (1.0 + np.abs(s64[:, sel]))
    within(g, S.selective_sigmoid_bwd(yn, g0, start, step), a64, 3, "grad")               # (3) 1 - s and two products
    assert np.isfinite(gn).all()


def test_selective_sigmoid_rejects(L):
    by, y = guarded((3, 576), dev(np.ones((3, 576))))
    bad = [(0, 576, 6, 8, 0), (3, 0, 6, 8, 0), (3, 576, -1, 8, 0), (3, 576, 576, 8, 0), (3, 576, 6, 0, 0), (3, 576, 6, -8, 0),
           (3, 576, 6, 8, 1)]                                       # (the last: backward without a gradient)
    for B, ncols, start, step, bwd in bad:
        with pytest.raises(L.HipError):
            L.spnet_selective_sigmoid(y.data_ptr(), None, B, ncols, start, step, bwd, st())
    torch.cuda.synchronize()
    assert bool((y == 1.0).all()) and guard_untouched(by)


# ============================================================================================ 7. decode
@pytest.mark.parametrize("sig", [0, 1])
def test_decode_on_the_branch_cut(L, sig):
    """(cos 2t, sin 2t) on the negative real axis (atan2f = +-pi: 90 degrees either way), at the origin (atan2f(0, 0) = 0
    -> 180), on the positive real axis (0 -> 180) and on the imaginary axis (45 / 135)."""
    B, ncols = 2, 576
    rs = np.random.RandomState(9)
    Yn = (rs.randn(B, ncols) * 0.5).astype(np.float32)
    pairs = [(1.0, 0.0), (-1.0, 0.0), (-1.0, -0.0), (0.0, 0.0), (0.0, 1.0), (0.0, -1.0)]
    expect = [180.0, 90.0, 90.0, 180.0, 45.0, 135.0]
    for r, p0 in ((0, 0), (1, 66)):
        for k, (c, s_) in enumerate(pairs):                         # ranges 2, means 0: v = 2 * yn exactly
            Yn[r, (p0 + k) * 8 + 4], Yn[r, (p0 + k) * 8 + 5] = np.float32(c / 2), np.float32(s_ / 2)
    gc = R.grid_constants()
    bo, out = guarded((B, ncols // 8, 7))
    ynd, md, rd = dev(Yn), dev(gc["means"]), dev(gc["ranges"])
    L.spnet_decode(ynd.data_ptr(), md.data_ptr(), rd.data_ptr(), out.data_ptr(), B, ncols, sig, st())
    assert guard_untouched(bo)
    want = R.decode(Yn, "hybrid" if sig else "same")
    o = out.cpu().numpy()
    ang = o[..., 4]
    assert (ang > 0).all() and (ang <= 180).all()
    np.testing.assert_allclose(ang, want[..., 4], rtol=0, atol=2e-4)                      # atan2f: test_decode's atol
    for r, p0 in ((0, 0), (1, 66)):
        np.testing.assert_allclose(ang[r, p0:p0 + 6], expect, rtol=0, atol=2e-4)
    # the affine columns (3): one product, one sum
    P = Yn.astype(np.float64).reshape(B, -1, 8)
    rg, mn = gc["ranges"].astype(np.float64).reshape(-1, 8), gc["means"].astype(np.float64).reshape(-1, 8)
    cols = [0, 1, 2, 3, 7] + ([] if sig else [6])
    within(out[..., [0, 1, 2, 3, 6] + ([] if sig else [5])], (P * rg + mn)[..., cols], (np.abs(P) * rg + np.abs(mn))[..., cols], 2, "affine")
    if sig:
        np.testing.assert_allclose(o[..., 5], want[..., 5], rtol=1e-5, atol=2e-4)         # expf: test_decode's


# ============================================================================================ 8. min / max, cutout, salt & pepper
FRAMES = [(1, 1), (5, 7), (64, 48), (384, 512)]
COUNTS = [1, 3, 70]


def _frames(N, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((N, H, W), device="cuda", generator=g) * 2 - 1


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("N", COUNTS)
def test_minmax(L, N, H, W):
    """Frames smaller than the 16 x 256 threads of the first stage leave workgroups (whole waves) without a pixel; 70
    frames need a second workgroup of the combine stage."""
    x = _frames(N, H, W, N + H)
    x[0, -1, -1] = 100.0                        # an extreme on the last pixel
    if N > 1:
        x[1, -1, -1] = -100.0
    bm, mm = guarded((N, 2))
    scratch = torch.full((N * 32,), NAN, device="cuda")
    L.spnet_minmax(x.data_ptr(), N, H * W, mm.data_ptr(), scratch.data_ptr(), st())
    assert guard_untouched(bm)
    xn = x.cpu().numpy().reshape(N, -1)
    assert np.array_equal(mm.cpu().numpy(), np.stack([xn.min(1), xn.max(1)], 1))          # (1) a selection
    assert float(mm[0, 1]) == 100.0 and (N == 1 or float(mm[1, 0]) == -100.0)


def _cutout_params(N, H, W, seed):
    rs = np.random.RandomState(seed)
    rects = np.zeros((N, 6, 4), np.int32)
    rects[..., 0], rects[..., 1] = rs.randint(0, H + 1, (N, 6)), rs.randint(0, H + 1, (N, 6))     # r1 < r0: empty
    rects[..., 2], rects[..., 3] = rs.randint(0, W + 1, (N, 6)), rs.randint(0, W + 1, (N, 6))
    vals = rs.randn(N, 6).astype(np.float32)
    nrect = np.array([6, 0, 3, 1, 2, 4, 5], np.int32)[np.arange(N) % 7]
    # frame 0 (six rectangles): the full frame, an empty one, two that overlap, two random
    rects[0, 0] = (0, H, 0, W)
    rects[0, 1] = (H // 2, H // 2, 0, W)
    rects[0, 2] = (0, H // 2 + 1, 0, W // 2 + 1)
    rects[0, 3] = (H // 4, H, W // 4, W)
    for n in range(N):                          # slots past nrect must be ignored: make them paint the whole frame
        rects[n, nrect[n]:] = (0, H, 0, W)
        vals[n, nrect[n]:] = 777.0
    return rects, vals, nrect


def _paint(frame, rects, vals, nrect):
    return S.paint_rects(frame.copy(), [tuple(rects[k]) + (vals[k],) for k in range(nrect)])


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("N", COUNTS)
def test_cutout(L, N, H, W):
    rects, vals, nrect = _cutout_params(N, H, W, N * 13 + H)
    rd, vd, nd = idev(rects), dev(vals), idev(nrect)
    n_src = N + 2
    src = _frames(n_src, H, W, N + W)
    sn = src.cpu().numpy()
    idx = np.random.RandomState(N).permutation(n_src)[:N].astype(np.int32)                # a permuted index ...
    if N >= 3:
        idx[2] = idx[0]                                                                   # ... with a repeat
    bd, dst = guarded((N, H, W))
    idxd = idev(idx)
    L.spnet_cutout(src.data_ptr(), idxd.data_ptr(), dst.data_ptr(), N, H, W, rd.data_ptr(), vd.data_ptr(), nd.data_ptr(), st())
    assert guard_untouched(bd)
    want = np.stack([_paint(sn[idx[n]], rects[n], vals[n], nrect[n]) for n in range(N)])
    assert np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))        # (1) a select
    assert torch.equal(src.cpu(), torch.from_numpy(sn))
    # in place, no index: how the single-frame API calls it
    bi, x = guarded((N, H, W), src[:N])
    L.spnet_cutout(x.data_ptr(), None, x.data_ptr(), N, H, W, rd.data_ptr(), vd.data_ptr(), nd.data_ptr(), st())
    assert guard_untouched(bi)
    want = np.stack([_paint(sn[n], rects[n], vals[n], nrect[n]) for n in range(N)])
    assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32))          # (1)


@pytest.mark.parametrize("H,W", FRAMES)
@pytest.mark.parametrize("N", COUNTS)
def test_saltpepper(L, N, H, W):
    """300 salt and 700 pepper points (more than one trip of the 256 threads each); the first ten pepper points sit on
    the first ten salt points (pepper must win), salt points 10..19 repeat 20..29; every second frame is switched off."""
    rs = np.random.RandomState(N * 7 + W)
    ns, npp = 300, 700
    coords = np.zeros((N, 2, ns + npp), np.int32)
    coords[:, 0], coords[:, 1] = rs.randint(0, H, (N, ns + npp)), rs.randint(0, W, (N, ns + npp))
    coords[:, :, 10:20] = coords[:, :, 20:30]
    coords[:, :, ns:ns + 10] = coords[:, :, :10]
    flag = (np.arange(N) % 2 == 0).astype(np.int32)
    x0 = _frames(N, H, W, N + 3 * W)
    xn = x0.cpu().numpy()
    mm = np.stack([xn.reshape(N, -1).min(1), xn.reshape(N, -1).max(1)], 1)
    bx, x = guarded((N, H, W), x0)
    cd, fd, mmd = idev(coords), idev(flag), dev(mm)
    L.spnet_saltpepper(x.data_ptr(), N, H, W, cd.data_ptr(), ns, npp, fd.data_ptr(), mmd.data_ptr(), st())
    assert guard_untouched(bx)
    want = xn.copy()
    for n in range(N):
        if flag[n]:
            S.paint_saltpepper(want[n], coords[n, 0, :ns], coords[n, 1, :ns], coords[n, 0, ns:], coords[n, 1, ns:], mm[n, 1], mm[n, 0])
    got = x.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))                      # (1) flag 0: untouched
    assert got[0, coords[0, 0, 0], coords[0, 1, 0]] == mm[0, 0]                           # pepper over salt


# ============================================================================================ 9. dropout
@pytest.mark.parametrize("n", [1, 255, 100003, 8192 * 256 + 257])
@pytest.mark.parametrize("rate", [0.0, 0.1, 0.5])
def test_dropout(L, n, rate):
    """The last n is 257 elements past the 8192 x 256 threads of the capped grid."""
    seed = 3000000019                           # above 2^31: the seed is unsigned
    g = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n, device="cuda", generator=g)
    by, y = guarded((n,))
    L.spnet_dropout(x.data_ptr(), y.data_ptr(), n, seed, rate, None, st())
    assert guard_untouched(by)
    keep = S.dropout_keep(n, seed, rate)
    xn, yn = x.cpu().numpy(), y.cpu().numpy()
    assert np.array_equal(yn != 0, keep & (xn != 0))                                      # (1) the documented mask, every index
    assert np.array_equal(yn, np.where(keep, xn * S.dropout_scale(rate), np.float32(0)))  # (1) survivors x * float32(1/(1-rate))
    if rate == 0.0:
        assert torch.equal(y, x)                                                          # (1) the identity
    bi, z = guarded((n,), x)                    # in place: the backward pass regenerates the mask over the gradient
    L.spnet_dropout(z.data_ptr(), z.data_ptr(), n, seed, rate, None, st())
    assert guard_untouched(bi) and torch.equal(z, y)                                      # (1)
    sd = torch.from_numpy(np.array([seed], np.uint32).view(np.int32)).cuda()
    bs, s = guarded((n,))
    L.spnet_dropout(x.data_ptr(), s.data_ptr(), n, 1, rate, sd.data_ptr(), st())            # the seed from device memory wins
    assert guard_untouched(bs) and torch.equal(s, y)                                      # (1)
    if n >= 255 and rate > 0:
        L.spnet_dropout(x.data_ptr(), s.data_ptr(), n, seed + 1, rate, None, st())
        assert not torch.equal(s, y)
        assert np.array_equal(s.cpu().numpy() != 0, S.dropout_keep(n, seed + 1, rate) & (xn != 0))
