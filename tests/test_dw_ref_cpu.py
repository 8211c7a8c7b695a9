"""tests/helpers/dw_ref.py and the tables of tests/test_dwconv_gpu.py / tests/test_pool_gpu.py, without a GPU: the reference
agrees with the oracle (float64 autograd, tie-free data) on one shape of every class, its tie rules give the answers
written out here, every table row is exact in fp32 (assert_exact), takes the path it is there for (the library's host-only
functions: no device is touched) and holds the ties it is there for."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as T
from tests.helpers import dw_ref as R
from tests import test_dwconv_gpu as G
from tests import test_pool_gpu as PG


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def rnd(shape, seed):
    return np.random.RandomState(seed).randn(*shape)


# ---- the reference against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("B,H,W,C", [(2, 1, 1, 4), (1, 2, 2, 4), (2, 3, 3, 8), (2, 4, 5, 4), (1, 9, 8, 8)])
def test_depthwise_forward_and_gradients_against_the_oracle(B, H, W, C, stride):
    x, w = t64(rnd((B, H, W, C), H), True), t64(rnd((3, 3, C), W), True)
    y = T.dwconv3x3(x, w, stride)
    dy = rnd(tuple(y.shape), C)
    (y * t64(dy)).sum().backward()
    xn, wn = x.detach().numpy(), w.detach().numpy()
    assert np.allclose(R.dw_fwd(xn, wn, stride), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.dw_bwd_data(dy, wn, H, W, stride), x.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.dw_bwd_weight(xn, dy, stride), w.grad.numpy(), rtol=1e-12, atol=1e-12)


# one shape of every class of the stride-1 tables: cfg 1, cfg 0 with ragged tiles, a plane shorter than the streaming rings
@pytest.mark.parametrize("k", range(len(G.OPTIONS)), ids=lambda k: G.OPTIONS[k][0])
@pytest.mark.parametrize("shape", [(2, 5, 7, 8), (2, 13, 17, 4), (1, 2, 7, 4)], ids=G.sid)
def test_fused_backward_against_the_oracle(shape, k):
    B, H, W, C = shape
    _, relu_in, add, affine, bn, bnx = G.OPTIONS[k]
    d = {n: rnd((B, H, W, C), i + H) for i, n in enumerate(("x", "dy", "add", "bn_x"))}
    d["w"] = rnd((3, 3, C), 11)
    for i, n in enumerate(("scale", "shift", "mean", "invstd")):
        d[n] = rnd((C,), 20 + i)
    d["invstd"] = np.abs(d["invstd"]) + 0.5
    ref = R.Fused(d["dy"], d["x"], d["w"], **G.option_args(d, G.OPTIONS[k]))
    x, w = t64(d["x"]), t64(d["w"], True)
    a = (x * t64(d["scale"]) + t64(d["shift"])) if affine else x
    a = a.clone().requires_grad_(True)
    y = T.dwconv3x3(torch.relu(a) if relu_in else a, w)
    loss = (y * t64(d["dy"])).sum()
    if add:
        loss = loss + (a * t64(d["add"])).sum()
    loss.backward()
    close = lambda p, q: np.allclose(p, q.detach().numpy() if torch.is_tensor(q) else q, rtol=1e-11, atol=1e-11)
    assert close(ref.y, y) and close(ref.dx, a.grad) and close(ref.dw, w.grad)
    for regions in (R.tiled_regions(B, H, W), R.stream_regions(B, H, W, 0), R.stream_regions(B, H, W, 1), R.stream_regions(B, H, W, 5)):
        # the regions tile the tensor: the partial rows add up to the whole sums
        cover = np.zeros((B, H, W), int)
        for b, h0, h1, w0, w1 in regions:
            cover[b, h0:h1, w0:w1] += 1
        assert (cover == 1).all()
        assert close(ref.weight_rows(regions).sum(0).reshape(3, 3, C), w.grad)
        if bn:
            pre = d["bn_x"] if bnx else d["x"]
            xhat = (pre - d["mean"]) * d["invstd"]
            g = a.grad.numpy()
            rows = ref.bn_rows(regions)
            assert close(rows[:, 0].sum(0), g.sum((0, 1, 2))) and close(rows[:, 1].sum(0), (g * xhat).sum((0, 1, 2)))


@pytest.mark.parametrize("same", [1, 0])
@pytest.mark.parametrize("B,H,W,C", [(2, 3, 3, 4), (1, 4, 5, 8), (2, 7, 6, 4), (1, 5, 4, 4)])
def test_maxpool_against_the_oracle(B, H, W, C, same):
    x, res = rnd((B, H, W, C), H + W), None
    x_ss = np.concatenate([rnd((C,), 1) + 3, rnd((C,), 2)])
    r_ss = np.concatenate([rnd((C,), 3), rnd((C,), 4)])
    v = t64(x * x_ss[:C] + x_ss[C:], True)
    y = T.maxpool3x3s2_same(v) if same else T.maxpool3x3s2_valid(v)
    res = rnd(tuple(y.shape), 5)
    dy = rnd(tuple(y.shape), 6)
    (y * t64(dy)).sum().backward()
    y_ref, taps = R.maxpool_fwd(x, bool(same), res, x_ss, r_ss)
    assert np.allclose(y_ref, y.detach().numpy() + res * r_ss[:C] + r_ss[C:], rtol=1e-12, atol=1e-12)
    dx = R.maxpool_bwd(dy, taps, H, W, bool(same))
    assert np.allclose(dx, v.grad.numpy(), rtol=1e-12, atol=1e-12)
    yp, mean, invstd = rnd((B, H, W, C), 7), rnd((C,), 8), np.abs(rnd((C,), 9)) + 0.5
    for rows in (1, 2, 3):
        part = R.maxpool_bn_rows(dx, yp, mean, invstd, rows)
        assert np.allclose(part[:, 0].sum(0), dx.sum((0, 1, 2))) and np.allclose(part[:, 1].sum(0), (dx * (yp - mean) * invstd).sum((0, 1, 2)))


@pytest.mark.parametrize("B,H,W,C", [(2, 1, 1, 4), (1, 2, 3, 3), (2, 5, 8, 1), (1, 3, 5, 4)])
def test_average_pools_against_the_oracle(B, H, W, C):
    x = t64(rnd((B, H, W, C), H * W), True)
    y3 = T.avgpool3x3s1_same(x)
    dy3 = rnd((B, H, W, C), 3)
    (y3 * t64(dy3)).sum().backward()
    assert np.allclose(R.avgpool3_fwd(x.detach().numpy())[0], y3.detach().numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(R.avgpool3_bwd(dy3), x.grad.numpy(), rtol=1e-12, atol=1e-12)
    if H >= 2 and W >= 2:
        x.grad = None
        y2 = T.avgpool2(x)
        dy2 = rnd(tuple(y2.shape), 4)
        (y2 * t64(dy2)).sum().backward()
        assert np.allclose(R.avgpool2_fwd(x.detach().numpy()), y2.detach().numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(R.avgpool2_bwd(dy2, H, W), x.grad.numpy(), rtol=1e-12, atol=1e-12)
    else:
        assert R.avgpool2_fwd(x.detach().numpy()).size == 0 and not R.avgpool2_bwd(np.zeros((B, H // 2, W // 2, C)), H, W).any()


# ---- the tie rules, on cases whose answers are written out -------------------------------------------------------------------
def test_first_maximum_wins_on_a_3x3_image():
    """SAME on 3x3: pad 1 in front, windows (oh, ow) see rows 2*oh-1 .. 2*oh+1.  Channel 0 is constant: every window takes
    its FIRST in-image tap.  Channel 1 holds its maximum at the four pixels (1..2, 1..2): every window's first maximum in
    row-major order is pixel (1, 1), which collects all four gradients."""
    x = np.zeros((1, 3, 3, 4))
    x[0, 1:, 1:, 1] = 5
    x[..., 2:] = x[..., :2]
    y, taps = R.maxpool_fwd(x)
    assert taps[0, :, :, 0].tolist() == [[4, 3], [1, 0]] and taps[0, :, :, 1].tolist() == [[8, 6], [2, 0]]
    assert y[0, :, :, 0].tolist() == [[0, 0], [0, 0]] and y[0, :, :, 1].tolist() == [[5, 5], [5, 5]]
    assert R.pack_taps(taps).tolist() == [0x08040804, 0x06030603, 0x02010201, 0]
    dx = R.maxpool_bwd(np.ones((1, 2, 2, 4)), taps, 3, 3)
    assert dx[0, :, :, 0].tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 0]] and dx[0, :, :, 1].tolist() == [[0, 0, 0], [0, 4, 0], [0, 0, 0]]
    # VALID: one window over the whole image, no padding: tap 0 for the constant channel, tap 4 = pixel (1, 1) for the other
    yv, tv = R.maxpool_fwd(x, same=False)
    assert tv[0, 0, 0].tolist() == [0, 4, 0, 4] and yv[0, 0, 0].tolist() == [0, 5, 0, 5]


def test_first_maximum_wins_on_a_2x2_image():
    """SAME on 2x2: no padding in front, one window with the taps (kh, kw) in {0, 1}^2"""
    x = np.zeros((1, 2, 2, 4))
    x[0, :, :, 1] = [[1, 3], [2, 0]]
    x[0, :, :, 2] = [[-2, -2], [-1, -1]]
    x[0, :, :, 3] = [[2, 2], [2, 2]]
    y, taps = R.maxpool_fwd(x)
    assert taps[0, 0, 0].tolist() == [0, 1, 3, 0] and y[0, 0, 0].tolist() == [0, 3, -1, 2]
    dx = R.maxpool_bwd(np.full((1, 1, 1, 4), 2.0), taps, 2, 2)
    assert dx[0, :, :, 1].tolist() == [[0, 2], [0, 0]] and dx[0, :, :, 2].tolist() == [[0, 0], [2, 0]]
    assert R.tie_share(x) == 0.75 and R.tie_share(x[..., 2:3]) == 1.0


def test_relu_mask_is_strict_at_zero():
    """a == 0 after the affine: relu(a) == 0 AND no gradient passes (a > 0 is false); `add` still does"""
    x = np.array([0.0, 1, -1, 3]).reshape(1, 1, 1, 4)
    w = np.zeros((3, 3, 4))
    w[1, 1] = 2
    f = R.Fused(np.ones((1, 1, 1, 4)), x, w, relu_in=1, add=np.full((1, 1, 1, 4), 5.0), scale=np.ones(4), shift=np.array([0.0, -1, 1, -2]),
                mean=np.array([1.0, 1, 1, 1]), invstd=np.array([0.5, 0.5, 2, 2]))
    assert f.a.ravel().tolist() == [0, 0, 0, 1] and f.y.ravel().tolist() == [0, 0, 0, 2]
    assert f.dx.ravel().tolist() == [5, 5, 5, 7] and f.dw[1, 1].tolist() == [0, 0, 0, 1] and not f.dw[0].any()
    rows = f.bn_rows([(0, 0, 1, 0, 1)])
    assert rows[0, 0].tolist() == [5, 5, 5, 7] and rows[0, 1].tolist() == [-2.5, 0, -20, 28]
    g = R.Fused(np.ones((1, 1, 1, 4)), x, w, relu_in=0, scale=np.ones(4), shift=np.array([0.0, -1, 1, -2]))
    assert g.dx.ravel().tolist() == [2, 2, 2, 2]


def test_partial_row_regions_are_the_documented_ones():
    assert R.tiled_regions(1, 13, 17) == [(0, 0, 12, 0, 16), (0, 0, 12, 16, 17), (0, 12, 13, 0, 16), (0, 12, 13, 16, 17)]
    assert R.tiled_regions(2, 6, 8) == [(0, 0, 6, 0, 8), (1, 0, 6, 0, 8)] and R.tiled_cfg(6, 8) == 1 and R.tiled_cfg(7, 1) == 0 and R.tiled_cfg(1, 9) == 0
    assert R.stream_regions(1, 5, 9, 2) == [(0, 0, 2, 0, 8), (0, 0, 2, 8, 9), (0, 2, 4, 0, 8), (0, 2, 4, 8, 9), (0, 4, 5, 0, 8), (0, 4, 5, 8, 9)]
    assert R.stream_regions(1, 5, 9, 0) == R.stream_regions(1, 5, 9, 8) == [(0, 0, 5, 0, 8), (0, 0, 5, 8, 9)]


def test_assert_exact_rejects_what_is_not_exact():
    x = np.full((1, 64, 64, 4), 64.0)
    with pytest.raises(AssertionError):
        R.assert_exact_dw(x, x, np.ones((3, 3, 4)))                # 4096 pixels * 2^12 = 2^24 in the weight sums
    R.assert_exact_dw(x[:, :63], x[:, :63], np.ones((3, 3, 4)))
    with pytest.raises(ValueError):
        R.assert_exact_dw(x + 0.5, x, np.ones((3, 3, 4)))
    with pytest.raises(ValueError):
        R.assert_exact_dw(x[:, :8], x[:, :8], np.ones((3, 3, 4)), mean=np.zeros(4), invstd=np.full(4, 0.3))
    with pytest.raises(AssertionError):                             # the half-integers of xhat cost one bit
        R.assert_exact_dw(x[:, :32], x[:, :32], np.zeros((3, 3, 4)), add=x[:, :32] * 32, mean=np.zeros(4), invstd=np.full(4, 0.5))
    with pytest.raises(AssertionError):
        R.assert_exact_pool(np.full((1, 2, 2, 4), 2.0 ** 23), np.ones((1, 1, 1, 4)), residual=np.full((1, 1, 1, 4), 2.0 ** 23))


def test_guard_checkers_find_stray_writes():
    want = np.arange(12.0)
    buf, off = R.place(np.full(12, R.SENTINEL), R.SENTINEL)
    assert off == R.FRONT and off % 4 == 0 and off > 0
    buf[off:off + 12] = want
    assert R.check_placed(buf, want) == []
    for at in (off - 1, off + 12, 0, buf.size - 1):
        bad = buf.copy()
        bad[at] = 0
        assert R.check_placed(bad, want) and R.check_guards(bad, 12)
    bad = buf.copy()
    bad[off + 3] = np.nan
    assert R.check_placed(bad, want) and R.check_guards(bad, 12) == []
    # planes: the matrix in the high plane, zeros elsewhere
    Rr, K = 19, 36
    ps = R.plane_elems(Rr, K)
    assert ps == 2 * 2 * 512 and np.unique(R.x3_offsets(Rr, K)).size == Rr * K and R.x3_offsets(Rr, K).max() < ps
    m = R.ints((Rr, K), -200, 200, 1)
    words = np.full(8 + 3 * ps + 8, 0x40E0, np.uint16)
    words[8:8 + 3 * ps] = 0
    words[8 + R.x3_offsets(Rr, K)] = (m.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    assert R.check_planes(words, m, 8, 8, 0x40E0) == []
    pad = np.setdiff1d(np.arange(ps), R.x3_offsets(Rr, K).ravel())
    for at in (8 + pad[0], 8 + ps + 5, 8 + 2 * ps + 7, 3, 8 + 3 * ps + 1, 8 + R.x3_offsets(Rr, K)[18, 35]):
        bad = words.copy()
        bad[at] = 0x3F80
        assert R.check_planes(bad, m, 8, 8, 0x40E0), at


# ---- every table row: exact, on its path, with its ties ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from spnet_amd import _lib
    return _lib


def test_stride1_rows_are_exact_and_hold_zeros_behind_the_affine():
    for shape in G.ALL:
        d = G.case(shape)
        for n in ("x", "dy", "add", "bn_x", "w", "shift", "mean"):
            assert np.abs(d[n]).max() <= 2 and np.array_equal(d[n], np.rint(d[n]))
        assert set(np.unique(d["scale"])) <= {-2.0, -1.0, 1.0, 2.0} and set(np.unique(d["invstd"])) <= {0.5, 1.0, 2.0}
        for k in range(len(G.OPTIONS)):
            ref = G.fused(shape, k)                                         # (runs assert_exact_dw)
            assert np.abs(ref.y).max() < 256
        assert R.zero_share(G.fused(shape, 4).a) >= 0.05, shape             # the affine is on: a == 0 is a real case


def test_stride1_rows_take_their_paths(lib):
    for table, cfg in ((G.CFG1, 1), (G.CFG0, 0)):
        for B, H, W, C in table:
            c, th, tw, cc, nth, ntw, chunks = R.tiled_geom(H, W, C)
            assert c == cfg == R.tiled_cfg(H, W)
            rows = int(lib.spnet_dwconv3x3_tiled_rows(B, H, W, C))
            assert rows == B * nth * ntw == len(R.tiled_regions(B, H, W))
            assert int(lib.spnet_dwconv3x3_tiled_bwd_ws(B, H, W, C)) == (rows + 32) * 9 * C
    chunks = lambda s: R.tiled_geom(*s[1:])[6]
    assert chunks((2, 3, 4, 516)) == 9 and 516 % 64 and chunks((2, 13, 17, 260)) == 9 and 260 % 32       # XCD remap from 8 chunks on
    assert R.tiled_geom(13, 17, 36)[4:6] == (2, 2) and 13 % 12 == 1 and 17 % 16 == 1 and 36 % 32 == 4
    assert R.tiled_geom(12, 16, 32)[4:] == (1, 1, 1)
    odd_wave_counts = set()
    for shape in G.STREAM:
        B, H, W, C = shape
        for backward in (True, False):
            values = G.rps_values(shape, backward)
            assert len({R.stream_geom(B, H, W, C, r, backward)[3] for r in values}) == len(values)
            assert {R.stream_geom(B, H, W, C, r, backward)[3] for r in (0, 1, 2, 3, 5, H, H + 3)} == {R.stream_geom(B, H, W, C, r, backward)[3] for r in values}
        for rps in G.rps_values(shape, True):
            strips, cchunks, segs, per, waves = R.stream_geom(B, H, W, C, rps)
            rows = int(lib.spnet_dwconv3x3_stream_rows(B, H, W, C, rps))
            assert rows == B * segs * strips == len(R.stream_regions(B, H, W, rps)) and waves == rows * cchunks
            assert int(lib.spnet_dwconv3x3_stream_bwd_ws(B, H, W, C, rps)) == (rows + 32) * 9 * C
            if waves % 4:
                odd_wave_counts.add((shape, per))
        if H > 1:
            assert 1 in [R.stream_geom(B, H, W, C, r)[3] for r in G.rps_values(shape, True)]              # a one-row segment
    assert len([1 for s, _ in odd_wave_counts if s == (3, 5, 17, 36)]) >= 3
    assert any(H < 3 for _, H, _, _ in G.STREAM) and {1, 7, 9} <= {W for _, _, W, _ in G.STREAM}         # shorter than both rings


def test_strided_rows_are_exact_and_sized_by_their_row_counts(lib):
    pads = set()
    for stride in (1, 2):
        for H, W in G.STRIDED_HW:
            pads |= {(stride, R.same_geom(H, stride)[1]), (stride, R.same_geom(W, stride)[1])}
            for C in G.STRIDED_C:
                for B in G.STRIDED_B:
                    G.strided_draw(B, H, W, C, stride, G.strided_seed(B, H, W, C, stride))
                    OH, OW = R.same_geom(H, stride)[0], R.same_geom(W, stride)[0]
                    assert int(lib.spnet_dwconv3x3_strided_ws(B, H, W, C, stride)) == R.strided_rows(B, OH, OW, C) * 9 * C
    assert pads == {(1, 1), (2, 0), (2, 1)}
    B, H, W, C, stride = G.ROW_CAP
    x, dy, w = G.strided_draw(B, H, W, C, stride, G.ROW_CAP_SEED, v=1)
    assert np.abs(x).max() == 1 and np.abs(dy).max() == 1
    assert int(lib.spnet_dwconv3x3_strided_ws(B, H, W, C, stride)) == 256 * 9 * C and R.chan_lanes(C // 4) == 8
    assert int(lib.spnet_dwconv3x3_strided_ws(1, 255, 256, C, 1)) == 255 * 9 * C                           # one row short of the cap


def test_pool_rows_are_exact_and_full_of_ties(lib):
    for same, hw, cbs in ((True, PG.SAME_HW, [(c, b) for c in PG.SAME_C for b in PG.SAME_B]), (False, PG.VALID_HW, PG.VALID_CB)):
        for H, W in hw:
            for C, B in cbs:
                for kind in ("ints", "const", "affine") if same else ("ints", "const"):
                    x, x_ss, res, r_ss = PG.pool_data(kind, B, H, W, C, same)
                    assert np.abs(x).max() <= 2
                    R.assert_exact_pool(x, np.full((1, 1, 1, C), 2.0), res, x_ss, r_ss)
                    share = R.tie_share(x * x_ss[:C] + x_ss[C:] if x_ss is not None else x, same)
                    assert share >= (1.0 if kind == "const" else 0.25), (kind, B, H, W, C, share)
    for B, H, W, C in PG.BNSUMS_SHAPES:
        assert R.tie_share(R.draw_pool(B, H, W, C, PG.pool_seed(B, H, W, C))) >= 0.25
        for m in PG.BNSUMS_MAX_ROWS + (0, 2, 5):
            rows = int(lib.spnet_maxpool3x3s2_bwd_rows(B, H, W, C, m))
            assert rows == R.pool_bwd_rows(B, H, W, m) and 1 <= rows <= max(m, 1)
    assert [int(lib.spnet_maxpool3x3s2_bwd_rows(*s, 128)) for s in PG.BNSUMS_SHAPES] == [3, 6, 1]
