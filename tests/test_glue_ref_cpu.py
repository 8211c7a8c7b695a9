"""tests/helpers/glue_ref.py and the tables of tests/test_irv2_glue_gpu.py / tests/test_densenet_glue_gpu.py, without a GPU:
the references agree with an independent formulation (the oracle's float64 convolution and autograd, bn_ref.backward_saved,
gemm_ref.patch_matrix), every table row is exact in fp32 (its assert_exact_*), takes the path it is there for (the library's
host-only functions: no device is touched) and holds the zeros it is there for."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as T
from tests.helpers import bn_ref as BN
from tests.helpers import gemm_ref as G
from tests.helpers import glue_ref as R
from tests import test_densenet_glue_gpu as DG
from tests import test_irv2_glue_gpu as IG


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def rnd(shape, seed):
    return np.random.RandomState(seed).randn(*shape)


@pytest.fixture(scope="module")
def lib():
    from spnet_amd import _lib
    return _lib


# ---- the references against independent formulations -------------------------------------------------------------------------
@pytest.mark.parametrize("KH,KW,s", IG.TAPS)
def test_patch_matrix_and_adjoint_against_the_oracle(KH, KW, s):
    for B, H, W, C, _, _, _, same in IG.patch_cases(KH, KW, s):
        C = 4
        xi = R.ramp((B, H, W, C)).astype(np.int64)
        assert np.array_equal(R.patch_matrix(xi, KH, KW, s, same), G.patch_matrix(xi, KH, KW, s, same))
        x, w = t64(rnd((B, H, W, C), H), True), t64(rnd((KH, KW, C, 3), W))
        y = T.conv2d_general(x, w, s, "same" if same else "valid")
        col = R.patch_matrix(x.detach().numpy(), KH, KW, s, same)
        assert np.allclose(col @ w.numpy().reshape(-1, 3), y.detach().numpy().reshape(-1, 3), rtol=1e-12, atol=1e-12)
        dy = rnd(tuple(y.shape), 3)
        (y * t64(dy)).sum().backward()
        dcol = dy.reshape(-1, 3) @ w.numpy().reshape(-1, 3).T
        assert np.allclose(R.patch_adjoint(dcol, B, H, W, C, KH, KW, s, same), x.grad.numpy(), rtol=1e-12, atol=1e-12)
        # <col, dcol> == <x, adjoint(dcol)> in exact integers
        di = R.ints(col.shape, 5).astype(np.int64)
        assert int((R.patch_matrix(xi, KH, KW, s, same) * di).sum()) == int((xi * R.patch_adjoint(di, B, H, W, C, KH, KW, s, same)).sum())


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 2, 6), (1, 7, 8), (2, 13, 6)])
def test_conv7_against_the_oracle(B, H, W):
    x, w, dy = DG.conv7_case(B, H, W)
    xt, wt = t64(x, True), t64(w, True)
    y = T.conv2d_general(torch.nn.functional.pad(xt, (0, 0, 3, 3, 3, 3)), wt, 2, "valid")
    assert tuple(y.shape[1:3]) == (R.conv7_out(H), R.conv7_out(W))
    (y * t64(dy)).sum().backward()
    assert np.array_equal(R.conv7_fwd(x, w), y.detach().numpy())
    assert np.array_equal(R.conv7_dgrad(dy, w, H, W), xt.grad.numpy()) and np.array_equal(R.conv7_wgrad(x, dy), wt.grad.numpy())
    # the scatter forms of the two cap cases == the full convolutions
    pts = [(B - 1, H - 1, W - 1, 2, 3), (0, 0, 0, 0, -2), (0, H // 2, W // 2, 1, 1)]
    xs = np.zeros_like(x)
    for b, h, ww, ci, v in pts:
        xs[b, h, ww, ci] += v
    assert np.array_equal(R.conv7_fwd_scatter(pts, w, B, H, W), R.conv7_fwd(xs, w))
    OH, OW = R.conv7_out(H), R.conv7_out(W)
    pts = [(B - 1, OH - 1, OW - 1, 63, 3), (0, 0, 0, 0, -2), (0, OH // 2, OW // 2, 5, 1)]
    ds = np.zeros_like(dy)
    for b, oh, ow, co, v in pts:
        ds[b, oh, ow, co] += v
    assert np.array_equal(R.conv7_dgrad_scatter(pts, w, B, H, W), R.conv7_dgrad(ds, w, H, W))


@pytest.mark.parametrize("M,C", [(1, 4), (33, 8), (126, 4), (129, 8)])
def test_batchnorm_sums_and_producer_finalize_against_backward_saved(M, C):
    """sum g, sum g*xhat of both partial-row layouts add up to dbeta, dgamma of the closed form; with one consumer,
    u = gamma*dbeta and v = gamma*dgamma, the producer finalize is its dx"""
    x, dz = rnd((M, C), 1), rnd((M, C), 2)
    gamma, beta, mean, invstd = rnd((C,), 3), rnd((C,), 4), rnd((C,), 5), np.abs(rnd((C,), 6)) + 0.5
    for relu in (0, 1):
        ref = BN.backward_saved(x, dz, gamma, beta, mean, invstd, relu)
        scale, shift = gamma * invstd, beta - mean * gamma * invstd
        g, Gm, part = R.dense_consumer_bwd(dz, x, scale, shift, mean, invstd, gamma, relu, np.zeros((M, C)))
        assert part.shape == (R.dense_rows(M), 2, C)
        assert np.allclose(g, ref["g"].numpy()) and np.allclose(part[:, 0].sum(0), ref["dbeta"].numpy()) and np.allclose(part[:, 1].sum(0), ref["dgamma"].numpy())
        y = ref["out_pre"].numpy()                       # the bnsums producers mask with the layer's OUTPUT y = relu(pre)
        for rows in (1, 2, R.grad_bnsums_rows(M, 512)):
            p2 = R.bn_rows(R.relu_mask(dz, np.maximum(y, 0), relu), x, mean, invstd, rows)
            assert np.allclose(p2[:, 0].sum(0), ref["dbeta"].numpy()) and np.allclose(p2[:, 1].sum(0), ref["dgamma"].numpy())
        dx = R.dense_producer_fin(Gm, gamma * part[:, 0].sum(0), gamma * part[:, 1].sum(0), x, mean, invstd, M)
        assert np.allclose(dx, ref["dx"].numpy(), rtol=1e-10, atol=1e-10)
        # the fp32 finalize: its double sum, cast and fmaf stay within two roundings of float64
        dgamma, dbeta, u, v = R.dense_consumer_fin(part, gamma, np.zeros(C), np.zeros(C))
        assert np.allclose(dbeta, ref["dbeta"].numpy(), rtol=1e-6, atol=1e-6) and np.allclose(v, np.float32(gamma) * dgamma, rtol=1e-6, atol=1e-7)


def test_partial_row_layouts_are_the_documented_ones():
    g = np.arange(1.0, 101.0).reshape(100, 1) * np.ones((1, 4))
    z = np.zeros(4)
    rows = R.bn_rows(g, np.zeros((100, 4)), z, z + 1, 2)          # pixels 0..31 and 64..95 | 32..63 and 96..99
    assert rows[0, 0, 0] == sum(range(1, 33)) + sum(range(65, 97)) and rows[1, 0, 0] == sum(range(33, 65)) + sum(range(97, 101))
    slabs = R.dense_colsums(g)
    assert slabs.shape == (2, 2, 4) and slabs[0, 0, 0] == sum(range(1, 65)) and slabs[1, 0, 0] == sum(range(65, 101)) and slabs[1, 1, 0] == sum(k * k for k in range(65, 101))


def test_elementwise_references_and_their_zero_rules():
    y = np.array([0.0, -0.0, 1.0, -1.0])
    g = np.array([2.0, 3.0, -1.0, 5.0])
    assert R.relu_mask(g, y, 1).tolist() == [0, 0, -1, 0] and R.relu_mask(g, y, 0).tolist() == g.tolist()
    dx, dup = R.resadd_bwd(y, g, 0.17, 1)
    assert dx.dtype == np.float32 and dup.dtype == np.float32 and dup[2] == np.float32(0.17) * np.float32(-1)
    x, up = np.array([1.0, -1.0, -0.0, 2.0]), np.array([-4.0, 8.0, -0.0, 4.0])
    assert R.resadd(x, up, 0.25, 0, exact=True).tolist() == [0, 1, 0, 3] and R.resadd(x, up, 0.25, 1, exact=True).tolist() == [0, 1, 0, 3]
    a = R.resadd(x, up, 0.17, 0)
    exact = x.astype(np.float64) + np.float64(np.float32(0.17)) * up                      # (a 48-bit product + x: exact in float64 here)
    assert a.dtype == np.float32 and np.array_equal(a, exact.astype(np.float32))
    with pytest.raises(AssertionError):
        R.resadd(x, up, 0.17, 0, exact=True)
    assert R.copy_cols(np.ones((2, 4)), 2 * np.ones((2, 4)), 1).tolist() == [[3.0] * 4] * 2 and R.copy_cols(np.ones((2, 4)), 2 * np.ones((2, 4)), 0).tolist() == [[2.0] * 4] * 2
    p = R.pad_nhwc(R.ramp((1, 2, 2, 4)), 1, 0, 2, 1)
    assert p.shape == (1, 3, 5, 4) and not p[:, 0].any() and not p[:, :, :2].any() and not p[:, :, 4:].any()
    assert np.array_equal(R.pad_nhwc(p, 1, 0, 2, 1, backward=True), R.ramp((1, 2, 2, 4)))
    d = R.copy_cols_batched(6, 3, [np.ones((3, 2)), 2 * np.ones((1, 4))])
    assert d[:, :2].tolist() == [[1, 1]] * 3 and d[0, 2:].tolist() == [2] * 4 and (d[1:, 2:] == R.SENTINEL).all()


def test_dense_coeffs_follows_finalize_bits():
    """training: scale, shift and the moving update of bn_ref.finalize_bits on the same batch statistics"""
    C, M = 9, 37
    rs = np.random.RandomState(0)
    s = rs.randn(C) * M
    q = s * s / M + (rs.rand(C) + 0.5) * M                      # a variance between 0.5 and 1.5: never clamped
    gamma, beta, mm, mv = (rs.randn(C).astype(np.float32) for _ in range(4))
    mean, invstd, scale, shift, nmm, nmv = BN.finalize_bits(s, q, M, gamma, beta, 1e-3, 0.99, mm, np.abs(mv))
    var = BN.fma64(-(s / M), s / M, q / M)
    bvar = (var * (M / (M - 1.0))).astype(np.float32)
    coef, mm2, mv2 = R.dense_coeffs(C, C + 3, gamma, beta, mean, invstd, mean, bvar, mm, np.abs(mv), 1e-3, 0.99, 1)
    assert np.array_equal(coef[:C], scale) and np.array_equal(coef[2 * (C + 3):2 * (C + 3) + C], shift) and not coef[C:2 * (C + 3)].any()
    assert np.array_equal(mm2, nmm) and np.array_equal(mv2, nmv)
    coef0, mm0, mv0 = R.dense_coeffs(C, C + 3, gamma, beta, None, None, None, None, mm, np.abs(mv) + 1, 1e-3, 0.99, 0)
    want = gamma / np.sqrt(np.abs(mv).astype(np.float64) + 1 + 1e-3)
    assert np.allclose(coef0[:C], want, rtol=1e-6) and np.array_equal(mm0, mm)


def test_assert_exact_rejects_what_is_not_exact():
    with pytest.raises(AssertionError):
        R.assert_exact_patches(x=np.full((1, 1, 1, 4), 2.0 ** 24))
    with pytest.raises(AssertionError):
        R.assert_exact_patches(dcol=np.full((1, 36), 2.0 ** 21), taps=9)
    with pytest.raises(ValueError):
        R.assert_exact_patches(x=np.full((1, 1, 1, 4), 0.5))
    big = np.full((4096, 4), 2.0 ** 11)
    with pytest.raises(AssertionError):
        R.assert_exact_bnsums(big, np.ones((4096, 4)), np.ones(4), np.ones(4))
    with pytest.raises(ValueError):
        R.assert_exact_bnsums(np.ones((2, 4)), np.ones((2, 4)), np.ones(4), np.full(4, 0.3))
    with pytest.raises(AssertionError):
        R.assert_exact_dense(np.full((4097, 4), 64.0))
    with pytest.raises(AssertionError):
        R.assert_exact_producer_fin(np.ones((3, 4)), np.ones(4), np.ones(4), np.ones((3, 4)), np.ones(4), np.ones(4), 3)
    with pytest.raises(AssertionError):
        R.assert_exact_conv7(bound=2.0 ** 24)
    with pytest.raises(AssertionError):
        R.assert_exact_elementwise((np.full(4, 2.0 ** 23), np.full(4, 2.0 ** 23)))


# ---- every table row: exact, on its path, with its zeros -----------------------------------------------------------------------
def test_patch_rows_take_their_paths():
    assert [R.unrolled(*t) for t in IG.TAPS] == [True] * 6 + [False] * 4
    for KH, KW, s in IG.TAPS:
        cases = IG.patch_cases(KH, KW, s)
        assert {c[3] for c in cases} == set(IG.CHANNELS) and {c[-1] for c in cases} == {0, 1}
        for B, H, W, C, _, _, _, same in cases:
            OH, OW, pt, pl = G.conv_geometry(H, W, KH, KW, s, same)
            assert OH >= 1 and OW >= 1
            R.assert_exact_patches(x=R.ramp((B, H, W, C)))
        assert any(c[-1] and (c[1] < KH or c[2] < KW) for c in cases) or (KH, KW) == (1, 1)       # SAME on an image smaller than the window
        assert any(not c[-1] and c[1] == KH for c in cases) and any(not c[-1] and c[2] == KW for c in cases)
        if s == 2:                                           # an odd total padding (one more row behind than in front) and an even one
            total = lambda n, k: max((-(-n // 2) - 1) * 2 + k - n, 0)
            assert {total(c[1], KH) % 2 for c in cases if c[-1]} == {0, 1} and {total(c[2], KW) % 2 for c in cases if c[-1]} == {0, 1}
    B, H, W, C, KH, KW, s, same = IG.PATCH_CAP
    assert B * H * W * KH * KW * (C // 4) > R.EW_CAP_ITEMS and B * H * W * C < R.LIMIT
    # the short-image refusals: floor division gives no output where truncation gives one
    for _, H, W in IG.SHORT:
        OH, OW, _, _ = G.conv_geometry(H, W, 3, 3, 2, 0)
        assert min(OH, OW) == 0 and int((H - 3) / 2) + 1 >= 1 and int((W - 3) / 2) + 1 >= 1


def test_bnsums_rows_are_exact_on_their_paths_and_full_of_zeros(lib):
    assert {(kh, kw) for kh, kw, s, same in IG.BN_TAPS if R.unrolled(kh, kw, s) and same} == set(R.UNROLLED_TAPS)
    assert {(kh, kw) for kh, kw, s, same in IG.BN_TAPS if R.unrolled(kh, kw, s) and not same} == set(R.UNROLLED_TAPS)
    assert [t for t in IG.BN_TAPS if not R.unrolled(*t[:3])] == [(3, 3, 2, 0), (3, 3, 2, 1), (1, 1, 1, 1)]
    pixels, channels = set(), set()
    for KH, KW, s, same in IG.BN_TAPS:
        cases = IG.bn_cases(KH, KW, s, same)
        if not same:
            assert any(G.conv_geometry(H, W, KH, KW, s, 0)[0] == 1 for _, H, W, _ in cases)
        if s == 2 and same:
            assert {H % 2 for _, H, _, _ in cases} == {0, 1}
        for B, H, W, C in cases:
            d = IG.bn_case(B, H, W, C, KH, KW, s, same)                 # (runs the assert_exact_* of the case)
            npix = B * H * W
            if npix > 4:
                assert R.zero_share(d["y"]) >= 0.1, (B, H, W, C)
            assert (d["y"] == 0).any()
            pixels.add(npix)
            channels.add(C)
            full = int(lib.spnet_grad_bnsums_rows(npix, IG.BN_MAX_ROWS))
            assert full == R.grad_bnsums_rows(npix, IG.BN_MAX_ROWS) == -(-npix // 32)
            assert IG.rows_to_run(None, npix) == IG.rows_to_run(lib, npix) and IG.rows_to_run(None, npix)[-1] == full
    assert {1, 31, 32, 33, 126} <= pixels and channels == set(IG.BN_CHANNELS)
    assert IG.rows_to_run(None, 126) == [1, 2, 4] and 126 > 2 * 32                 # the pixel loop strides for rows 1 and 2
    assert [(C // 4 + R.BN_QUADS - 1) // R.BN_QUADS for C in IG.BN_CHANNELS] == [1, 1, 2, 3]
    for m in (0, 1, 3, 512):
        for npix in (0, 1, 32, 33, 100000):
            assert int(lib.spnet_grad_bnsums_rows(npix, m)) == R.grad_bnsums_rows(npix, m)
    for C in IG.BN_CHANNELS:
        for M in IG.COLS_M:
            d = IG.cols_case(M, C)
            assert M < 8 or R.zero_share(d["y"]) >= 0.1


def test_copy_and_resadd_rows():
    for rows, cols, lds, ldd in IG.COPY_CASES + [IG.COPY_CAP]:
        assert lds != ldd and lds >= cols and ldd >= cols + 4 and (lds == cols or lds == cols + 4)
    assert any(r == 1 for r, _, _, _ in IG.COPY_CASES) and any(c == 4 for _, c, _, _ in IG.COPY_CASES)
    assert any((r * c // 4) % 256 for r, c, _, _ in IG.COPY_CASES)
    rows, cols, _, _ = IG.COPY_CAP
    assert rows * (cols // 4) > R.EW_CAP_ITEMS
    sizes = [r * c for r, c, _ in IG.BATCHED_JOBS]
    assert max(sizes) // 4 > R.BATCHED_CAP_ITEMS and min(sizes) == 4 and sorted(sizes)[1] * 100 < max(sizes)
    assert IG.RESADD_CAP_N // 4 > R.EW_CAP_ITEMS and 4 in IG.RESADD_N
    for n in IG.RESADD_N:
        for relu in (0, 1):
            x, up = IG.resadd_operands(n, IG.seed_of(n, relu), True)
            R.assert_exact_elementwise((x, up), unit=0.25)
            s = x + 0.25 * up
            assert R.zero_share(s) >= 0.1 and np.signbit(x[0]) and np.signbit(up[0])
            y = R.draw_y((n,), IG.seed_of(n, relu, 3))
            assert R.zero_share(y) >= 0.1 and np.signbit(y[1]) and not np.signbit(y[0])


def test_dense_rows_are_exact_and_land_on_zero(lib):
    assert [(C // 4 + R.DN_QUADS - 1) // R.DN_QUADS for C in DG.SUM_C] == [1, 1, 1, 2] and [C // 4 for C in DG.SUM_C] == [1, 63, 64, 65]
    for M in DG.SUM_M + (0, 128, 98304):
        assert int(lib.spnet_dense_rows(M)) == R.dense_rows(M)
    assert [R.dense_rows(M) for M in DG.SUM_M] == [1, 1, 1, 1, 1, 1, 2, 3]
    for c in DG.SUM_C:
        for M in DG.SUM_M:
            d = DG.dense_case(M, c)                                        # (runs assert_exact_dense)
            if M * c >= 64:
                assert R.zero_share(d["x"] * d["scale"] + d["shift"]) >= 0.1, (M, c)
            assert set(np.unique(d["invstd"])) <= {0.5, 1.0, 2.0} and np.abs(d["x"]).max() <= 3
    for M, C in DG.APPLY_CASES:
        x, scale, shift = R.draw_affine(R.ints((M, C), DG.seed_of(M, C, 2)), DG.seed_of(M, C, 2) + 1)
        R.assert_exact_dense(x, scale, shift)
        assert R.zero_share(x * scale + shift) >= 0.1
    M, C = DG.APPLY_CAP
    assert M * (C // 4) > R.APPLY_CAP_ITEMS
    for M, c0, c1 in DG.PRODUCER_EXACT:
        d, r = DG.producer_case(M, c0, c1)
        R.assert_exact_producer_fin(r["G"], r["u"], r["v"], r["x"], r["mean"], r["invstd"], M)
        assert c0 > 0 and np.isnan(d["G"][:, :c0]).all() and not np.isnan(r["G"]).any()
    assert all(M & (M - 1) for M, _, _ in DG.PRODUCER_BOUND)
    assert {(c + 7) // 8 for c in DG.FIN_C} == {1, 2} and {min(P, 32) for P in DG.FIN_P} == {1, 31, 32}


def test_conv7_rows_are_exact_and_sized_by_the_library(lib):
    for B, H, W in DG.CONV7_CASES + [DG.CONV7_WGRAD_SLABS, DG.CONV7_FWD_CAP, DG.CONV7_DGRAD_CAP, (16, 384, 512), (64, 768, 1024)]:
        assert int(lib.spnet_dense_conv7_ws(B, H, W)) == R.conv7_ws(B, H, W)
    assert R.conv7_slabs(64, 768, 1024) == R.CONV7_MAX_SLABS
    assert {v for _, H, W in DG.CONV7_CASES for v in (H, W)} == {1, 2, 6, 7, 8, 13} and {B for B, _, _ in DG.CONV7_CASES} == {1, 2, 3}
    for case in DG.CONV7_CASES + [DG.CONV7_WGRAD_SLABS]:
        DG.conv7_case(*case)                                               # (runs assert_exact_conv7)
    B, H, W = DG.CONV7_WGRAD_SLABS
    npix = B * R.conv7_out(H) * R.conv7_out(W)
    assert R.conv7_slabs(B, H, W) == 2 and npix > R.CONV7_SLAB_PIXELS and (-(-npix // 2)) % R.CONV7_STEP
    B, H, W = DG.CONV7_FWD_CAP
    assert B * R.conv7_out(H) * R.conv7_out(W) > R.CONV7_FWD_CAP_PIXELS
    assert all(0 <= h < H and 0 <= w < W for _, h, w, _, _ in DG.conv7_fwd_cap_points(H, W))
    B, H, W = DG.CONV7_DGRAD_CAP
    assert B * H * W > R.CONV7_DGRAD_CAP_PIXELS
    assert all(0 <= oh < R.conv7_out(H) and 0 <= ow < R.conv7_out(W) for _, oh, ow, _, _ in DG.conv7_dgrad_cap_points(H, W))
    for Bp, Hp, Wp, C, pt, pb, pl, pr in DG.PAD_CASES:
        assert C in (4, 12)
    assert any(p[4:] == (0, 0, 0, 0) for p in DG.PAD_CASES) and any(p[4] > p[1] and p[6] > p[2] for p in DG.PAD_CASES)
    assert any(p[4] != p[5] and p[6] != p[7] for p in DG.PAD_CASES)
