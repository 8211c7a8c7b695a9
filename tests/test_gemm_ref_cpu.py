"""tests/helpers/gemm_ref.py and the tables of tests/test_gemm_gpu.py, without a GPU: the checker finds what a subtly wrong
strided GEMM does (numpy models of a correct kernel and of eight broken ones), assert_exact rejects operands that are not
exact, the patch-matrix restatement agrees with the oracle's convolution, and spnet_gemm_plan (host only) confirms that
every row of the GPU tables takes the path it is there for.  At the end: the multi-piece operands of
tests/test_gemm_x3_gpu.py -- the six-term model of a bf16x3 kernel equals the int64 product on every one of them, and a
dropped or doubled term, or swapped middle and low planes, does not."""
import ctypes

import numpy as np
import pytest

from tests.helpers import gemm_ref as R
from tests import test_gemm_gpu as G


# ---- a numpy model of the forward-form kernel on flat buffers, with switchable defects --------------------------------------
def model_gemm(a, oa, lda, b, ob, ldb, c, oc, ldc, M, N, K, bug=None):
    """c[oc + m*ldc + n] = sum_k a[oa + m*lda + k] * b[ob + k*ldb + n] as the kernel addresses its operands"""
    rows = np.arange(M)
    if bug == "clamp off by one":
        rows = np.minimum(rows, M - 2)
    kk = K
    if bug == "drops the last reduction step":
        kk = K - 1
    if bug == "drops the last 4 of a ragged K":
        kk = K - 4 if K % 32 else K
    if bug == "reads column K of A":
        kk = K + 1
    A = a[oa + rows[:, None] * lda + np.arange(kk)[None, :]].astype(np.float64)
    B = b[ob + np.minimum(np.arange(kk), K - 1)[:, None] * ldb + np.arange(N)[None, :]].astype(np.float64)
    C = (A @ B).astype(np.float32)
    ncol, nrow = N, M
    if bug == "writes 4 columns past N":
        C = np.concatenate([C, C[:, -4:]], 1)
        ncol = N + 4
    if bug == "writes a row past M":
        C = np.concatenate([C, C[-1:]], 0)
        nrow = M + 1
    c[oc + np.arange(nrow)[:, None] * ldc + np.arange(ncol)[None, :]] = C


def model_reduce(ws, nslab, M, N, out, oc, ldc, bug=None):
    s = ws[:nslab * M * N].reshape(nslab, M, N).astype(np.float64).sum(0).astype(np.float32)
    ld = N if bug == "reduces with ldc = N" else ldc
    out[oc + np.arange(M)[:, None] * ld + np.arange(N)[None, :]] = s


def strided_case(M=70, N=72, K=36, seed=0):
    A, B = R.int_operands((M, K), -2, 2, seed), R.int_operands((K, N), -2, 2, seed + 1)
    R.assert_exact(R.as_int(A), R.as_int(B))
    a, oa = R.embed(A, K + 4)
    b, ob = R.embed(B, N + 20)
    c, oc = R.embed(np.full((M, N), R.SENTINEL, np.float32), N + 4, poison=R.SENTINEL)
    return A, B, (a.ravel(), oa, K + 4), (b.ravel(), ob, N + 20), (c.ravel(), oc, N + 4)


GEMM_BUGS = ["drops the last reduction step", "drops the last 4 of a ragged K", "clamp off by one", "writes 4 columns past N",
             "writes a row past M", "reads column K of A"]


def test_checker_passes_a_correct_strided_gemm():
    A, B, (a, oa, lda), (b, ob, ldb), (c, oc, ldc) = strided_case()
    model_gemm(a, oa, lda, b, ob, ldb, c, oc, ldc, 70, 72, 36)
    assert R.check_output(c, R.product(A, B, "fwd"), ldc) == []


@pytest.mark.parametrize("bug", GEMM_BUGS)
def test_checker_catches_a_broken_strided_gemm(bug):
    A, B, (a, oa, lda), (b, ob, ldb), (c, oc, ldc) = strided_case()
    model_gemm(a, oa, lda, b, ob, ldb, c, oc, ldc, 70, 72, 36, bug)
    found = R.check_output(c, R.product(A, B, "fwd"), ldc)
    assert found, bug
    kind = "gap/guard overwritten" if "writes" in bug else "block differs"
    assert any(f.startswith(kind) for f in found), found
    if bug == "reads column K of A":
        assert any("nan" in f for f in found), found


def test_checker_catches_a_slab_reduce_that_ignores_ldc():
    M, N, nslab = 37, 68, 5
    slabs = R.int_operands((nslab, M, N), -8, 8, 3)
    want = R.as_int(slabs).sum(0)
    for bug in (None, "reduces with ldc = N"):
        c, oc = R.embed(np.full((M, N), R.SENTINEL, np.float32), N + 4, poison=R.SENTINEL)
        model_reduce(slabs.ravel(), nslab, M, N, c.ravel(), oc, N + 4, bug)
        found = R.check_output(c, want, N + 4)
        assert bool(found) == bool(bug), (bug, found)


def test_checker_catches_a_missing_statistics_row():
    M, N, bm = 70, 72, 32
    C = R.product(R.int_operands((M, 36), -2, 2, 5), R.int_operands((36, N), -2, 2, 6), "fwd")
    R.assert_exact_stats(C, bm)
    want = R.col_stats(C, bm)
    assert want.shape == (3, 2, N) and np.array_equal(want[2, 0], C[64:].sum(0)) and np.array_equal(want[:, 1].sum(0), (C * C).sum(0))
    total = 4
    good = np.full(total * 2 * N, R.SENTINEL, np.float32)
    good[:want.size] = want.ravel()
    assert R.check_dense(good, want, (total - 3) * 2 * N) == []
    short = good.copy()
    short[2 * 2 * N:3 * 2 * N] = R.SENTINEL                   # the last statistics row was never written
    assert R.check_dense(short, want, (total - 3) * 2 * N)
    long = good.copy()
    long[want.size] = 0.0                                     # a write behind row stat_rows
    assert R.check_dense(long, want, (total - 3) * 2 * N)
    swapped = good.copy().reshape(total, 2, N)
    swapped[[0, 1]] = swapped[[1, 0]]                         # right in total, wrong row by row
    assert R.check_dense(swapped, want, (total - 3) * 2 * N)


def test_assert_exact_rejects_operands_over_the_bound():
    A, B = np.full((4, 1024), 128, np.float32), np.full((1024, 4), 128, np.float32)      # 1024 * 2^14 = 2^24
    assert R.exact_bound(A, B) == 2 ** 24
    with pytest.raises(AssertionError):
        R.assert_exact(A, B)
    R.assert_exact(A[:, :1023], B[:1023])
    with pytest.raises(AssertionError):
        R.assert_exact(A[:, :600], B[:600], extra=2)
    with pytest.raises(AssertionError):
        R.assert_exact_stats(np.full((64, 4), 512, np.int64), 64)      # 64 * 2^18
    R.assert_exact_stats(np.full((63, 4), 512, np.int64), 64)
    with pytest.raises(ValueError):
        R.assert_exact(A + 0.5, B)
    with pytest.raises(ValueError):
        R.embed(A, 1028, col0=2)
    assert float(R.int_operands((50, 50), -2, 2, 0, density=0.1).astype(bool).mean()) < 0.2


@pytest.mark.parametrize("KH,KW,stride,same,B,H,W", [(3, 3, 2, 1, 2, 5, 7), (1, 7, 1, 1, 1, 3, 4), (3, 3, 2, 0, 2, 6, 7), (7, 1, 1, 1, 1, 5, 2)])
def test_patch_matrix_against_the_oracle_convolution(KH, KW, stride, same, B, H, W):
    """a cross-check of the reference only: float64, integer data, so the two must agree exactly"""
    import torch
    from oracle import torch_ref as T
    C, Cout = 4, 3
    x = R.int_operands((B, H, W, C), -3, 3, KH + W).astype(np.float64)
    w = R.int_operands((KH, KW, C, Cout), -3, 3, KW + H).astype(np.float64)
    want = T.conv2d_general(torch.from_numpy(x), torch.from_numpy(w), stride, "same" if same else "valid").numpy()
    OH, OW, _, _ = R.conv_geometry(H, W, KH, KW, stride, same)
    got = (R.patch_matrix(x, KH, KW, stride, same) @ w.reshape(KH * KW * C, Cout)).reshape(B, OH, OW, Cout)
    assert want.shape == got.shape and np.array_equal(got, want)


# ---- the GPU tables take the paths they are written for (csrc/gemm_plan.h through spnet_gemm_plan: host only) ---------------
FORM, TILE, BM, BN, NSPLIT, KCHUNK, KSLICES, PIPE, TO_WS, STAT_ROWS = range(10)


def plan_of(form, M, N, K, tile, split=1, ws=0, colstats=0, batch=0, xf=0, accumulate=0, conv=0):
    from spnet_amd import _lib
    am, bmaj = R.FORMS[form]
    plan = (ctypes.c_int * 10)(*([-7] * 10))
    _lib.spnet_gemm_plan(am, bmaj, M, N, K, split, 1 if ws else 0, ws, colstats, 1 if batch else 0, batch, xf, accumulate, conv,
                         tile, ctypes.addressof(plan))
    return list(plan)


def on_its_path(p, form, tile, M, N, K, nsplit=1):
    assert p[FORM] == {"fwd": 0, "dgrad": 1, "wgrad": 2}[form]
    if tile:
        assert p[TILE] == tile
    assert (p[BM], p[BN]) == G.TILES[p[TILE]]
    assert p[NSPLIT] == nsplit and p[TO_WS] == (nsplit > 1) and p[STAT_ROWS] == -(-M // p[BM])
    return p


def test_tile_table_is_the_library_s():
    for t, (bm, bn) in G.TILES.items():
        p = plan_of("fwd", 256, 256, 64, t)
        assert (p[TILE], p[BM], p[BN]) == (t, bm, bn)


def test_gpu_tables_take_their_named_paths():
    seen_pipe = set()
    for form, tile, M, N, K in G.PLAIN:
        p = on_its_path(plan_of(form, M, N, K, tile), form, tile, M, N, K)
        # 33 K tiles: the pipelined main loop wherever the tile has one (the 128x128 tile has none); shorter K: never
        assert p[PIPE] == (K >= G.LONG_K and p[TILE] != 1), (form, tile, M, N, K)
        if p[PIPE]:
            seen_pipe.add((form, p[TILE]))
    assert seen_pipe >= {(f, t) for f in ("fwd", "dgrad", "wgrad") for t in range(2, 11)}
    for form, tile, split, M, N, K in G.SPLIT:
        p = on_its_path(plan_of(form, M, N, K, tile, split=split, ws=split * M * N), form, tile, M, N, K, nsplit=split)
        assert p[TO_WS] == 1 and p[NSPLIT] > 1 and (p[NSPLIT] - 1) * p[KCHUNK] < K <= p[NSPLIT] * p[KCHUNK] and K % p[KCHUNK]
    for form, tile, M, N, K in G.ACCUMULATE:
        p = on_its_path(plan_of(form, M, N, K, tile, accumulate=1), form, tile, M, N, K)
        assert p[PIPE] == (K >= G.LONG_K and p[TILE] != 1)
    for form, tile, M, N, K in G.COLSTATS:
        p = on_its_path(plan_of(form, M, N, K, tile, colstats=1), form, tile, M, N, K)
        assert p[PIPE] == (K >= G.LONG_K and p[TILE] != 1) and p[STAT_ROWS] == (2 if M > p[BM] else 1)      # one ragged row group | a full one and one of a single row
    for tile, M, N, K in G.BATCHED:
        on_its_path(plan_of("wgrad", M, N, K, tile, batch=3), "wgrad", tile, M, N, K)
    for tile, ks, M, N, K in G.BATCHED_SPLIT:
        p = on_its_path(plan_of("wgrad", M, N, K, tile, split=ks, ws=3 * ks * M * N, batch=3), "wgrad", tile, M, N, K, nsplit=ks)
        assert p[KSLICES] == ks and p[TO_WS] == 1
    for xf, table in ((1, G.BNBLEND), (2, G.BNRELU)):
        for tile, M, N, K, _ in table:
            p = on_its_path(plan_of("fwd", M, N, K, tile, xf=xf), "fwd", tile, M, N, K)
            assert p[PIPE] == 0
    for tile, cout, (KH, KW, stride, same), (Bn, H, W) in G.CONV:
        OH, OW, _, _ = R.conv_geometry(H, W, KH, KW, stride, same)
        if OH >= 1 and OW >= 1:
            on_its_path(plan_of("fwd", Bn * OH * OW, cout, KH * KW * G.CONV_C, tile, conv=1), "fwd", tile, Bn * OH * OW, cout, KH * KW * G.CONV_C)
    assert sum(1 for _, _, (KH, KW, s, same), (_, H, W) in G.CONV if min(R.conv_geometry(H, W, KH, KW, s, same)[:2]) < 1) == 8
    for tile, M, N, K in G.NONFINITE:
        on_its_path(plan_of("fwd", M, N, K, tile, colstats=1), "fwd", tile, M, N, K)


def test_gpu_table_operands_are_exact():
    """the draws of the plain / split / accumulate / statistics / batched tables, as the GPU tests make them (those assert
    the same before they launch; the remaining tables do so there as well)"""
    for base, table in ((0, G.PLAIN), (100, G.SPLIT), (200, G.ACCUMULATE), (400, G.COLSTATS)):
        for i, row in enumerate(table):
            form, (M, N, K) = row[0], row[-3:]
            A, B = G.draw(form, M, N, K, base + i)
            assert R.as_int(A).min() >= -2 and R.as_int(A).max() <= 2 and (K < G.LONG_K or np.abs(A).max() <= 1)
            R.assert_exact(*R.logical(A, B, form), extra=2)
            if table is G.COLSTATS:
                R.assert_exact_stats(R.product(A, B, form), G.TILES[row[1]][0])
    for base, table in ((500, G.BATCHED), (600, G.BATCHED_SPLIT)):
        for i, row in enumerate(table):
            G.batch_operands(*row[-3:], base + i)


# ---- the bf16x3 operands of tests/test_gemm_x3_gpu.py: what a subtly wrong six-term kernel would do to them ------------------
from tests import test_gemm_x3_gpu as X


def x3_sets():
    """(name, A [M][K], B [K][N], row group) of every plain GEMM operand set the GPU file launches"""
    for i, (s, swap) in enumerate(X.GEMM):
        yield ("gemm %dx%dx%d swap %d" % (X.X3_SHAPES[s] + (swap,)),) + X.gemm_case(i) + (96,)
    for i, (M, c, nb) in enumerate(X.WGRAD):
        for b in range(nb):
            z, dy = X.wgrad_case(i, b)
            yield ("wgrad M %d %dx%d problem %d of %d" % ((M,) + X.WGRAD_CH[c] + (b, nb)), z.T, dy, 96)


def knock_outs(A, B, finish=None):
    """{term: (share of outputs the model without it gets wrong, share with the term doubled)}; finish: the epilogue
    between the GEMM and the compared output"""
    pa, pb = R.bf16x3_pieces(A), R.bf16x3_pieces(B)
    finish = finish or (lambda y: y)
    want = finish(R.as_int(A) @ R.as_int(B))
    return {t: tuple(float((finish(R.x3_model(pa, pb, {t: f})) != want).mean()) for f in (0, 2)) for t in R.X3_TERMS}


def test_bf16_rounding_and_pieces():
    x = np.array([1.0, 257.0, 259.0, 261.0, -257.0, 262657.0, 3.1415927, 1e-3, -7.25e5, 0.0], np.float32)
    # 257 = 0x101 lies halfway between 256 and 258 (8 significand bits): ties go to the even one, 259 to 260
    assert R.bf16_rne(x)[:5].tolist() == [1.0, 256.0, 260.0, 260.0, -256.0]
    p = R.bf16x3_pieces(x)
    assert p[:, 5].tolist() == [262144.0, 512.0, 1.0] and np.array_equal(p.sum(0), x.astype(np.float64))
    assert np.array_equal(R.bf16_rne(p.astype(np.float32)), p.astype(np.float32))          # every piece is a bf16
    f = X.full_mantissa((64, 64), 1)
    q = R.bf16x3_pieces(f)
    assert (q[2] != 0).mean() > 0.9 and (f < 0).any() and (f > 0).any() and np.abs(f).max() / np.abs(f).min() > 2.0 ** 30
    assert (np.abs(q[1]) <= np.abs(q[0]) * 2.0 ** -8).all() and (np.abs(q[2]) <= np.abs(q[0]) * 2.0 ** -16).all()
    with pytest.raises(ValueError):
        R.bf16x3_pieces(np.array([0.1]))                       # not a float32
    with pytest.raises(ValueError):
        R.bf16_rne(np.array([np.inf], np.float32))


def test_x3_operands_make_the_six_term_model_exact():
    """every operand set of the GPU file: exact in fp32, the six-term model is the int64 product, the three dropped terms
    are identically zero, and the operands do hold three-piece and two-piece values"""
    sets = [(n, A, B) for n, A, B, _ in x3_sets()] + [("stats %d" % s,) + X.stats_case(s) for s in range(len(X.X3_SHAPES))]
    sets += [("dwfwd %d" % i,) + X.DwFwd(i).operands() for i in range(len(X.DWFWD))]
    sets += [("dwbwd %d" % i,) + X.DwBwd(i).operands() for i in range(len(X.DWBWD))]
    for name, A, B in sets:
        assert np.abs(A).max() < 2 ** 19 and np.abs(B).max() < 2 ** 19, name
        R.assert_exact(R.as_int(A), R.as_int(B))
        pa, pb = R.bf16x3_pieces(A), R.bf16x3_pieces(B)
        assert np.array_equal(R.x3_model(pa, pb), R.as_int(A) @ R.as_int(B)), name
        for t in R.X3_DROPPED:
            assert not R.x3_term(pa, pb, *t).any(), (name, t)
        if not name.startswith("stats"):
            assert (pa[2] != 0).any() and (pb[2] != 0).any() and ((pa[1] != 0) & (pa[2] == 0)).any(), name
    for s in range(len(X.X3_SHAPES)):
        A, B = X.stats_case(s)
        R.assert_exact_stats(R.as_int(A) @ R.as_int(B), X.X3_BM)
    for i in range(len(X.DWFWD)):
        X.DwFwd(i).assert_exact()
    for i in range(len(X.DWBWD)):
        X.DwBwd(i).assert_exact()


def test_x3_every_knock_out_shows_in_half_of_the_outputs():
    """a kernel that drops or doubles one of its six products gets at least half of the outputs of every plain GEMM case
    wrong -- a property of the operands, which is what makes the GPU comparison a test of all six"""
    for name, A, B, _ in x3_sets():
        for t, (gone, twice) in knock_outs(A, B).items():
            assert gone >= 0.5 and twice >= 0.5, (name, R.X3_TERM_NAMES[t], gone, twice)


def test_x3_knock_outs_show_in_the_last_row_group_and_the_last_k_step():
    """... in the rows past the last multiple of 96 and of 16 alone, and with nothing but the last K step of 32 (the ragged
    one, where there is one) contributing"""
    for name, A, B, bm in x3_sets():
        M, K = A.shape
        for g in (bm, 16):
            r0 = (M - 1) // g * g
            for t, (gone, twice) in knock_outs(A[r0:], B).items():
                assert gone > 0 and twice > 0, (name, "rows from %d" % r0, R.X3_TERM_NAMES[t])
        k0 = (K - 1) // 32 * 32
        for t, (gone, twice) in knock_outs(A[:, k0:], B[k0:]).items():
            assert gone > 0 and twice > 0, (name, "k from %d" % k0, R.X3_TERM_NAMES[t])


def test_x3_swapped_planes_show():
    """reading the low plane for the middle one (and the reverse), of either operand, changes the result"""
    for name, A, B, _ in x3_sets():
        pa, pb = R.bf16x3_pieces(A), R.bf16x3_pieces(B)
        want = R.as_int(A) @ R.as_int(B)
        assert float((R.x3_model(pa[[0, 2, 1]], pb) != want).mean()) >= 0.5, name
        assert float((R.x3_model(pa, pb[[0, 2, 1]]) != want).mean()) >= 0.5, name


def test_x3_statistics_sets_hold_the_two_piece_terms():
    for s in range(len(X.X3_SHAPES)):
        A, B = X.stats_case(s)
        ko = knock_outs(A, B)
        for t in ((0, 0), (0, 1), (1, 0)):
            assert ko[t][0] > 0 and ko[t][1] > 0, (s, R.X3_TERM_NAMES[t])
        stat = lambda y: R.col_stats(y, X.X3_BM)
        for t in ((0, 1), (1, 0)):
            assert knock_outs(A, B, stat)[t][0] > 0, (s, R.X3_TERM_NAMES[t])


def test_x3_knock_outs_reach_every_tile_of_the_fused_kernels():
    """the fused cases are sparse in multi-piece values (sums over a tile's 192 pixels have to stay exact), so a knock-out
    changes fewer outputs there; but each of the six changes the compared output in every 192-row tile and every block of
    96 output channels, the ragged last ones included"""
    cases = [("dwfwd %d" % i, X.DwFwd(i), lambda c, y: c.finish(y)) for i in range(len(X.DWFWD))]
    cases += [("dwbwd %d" % i, X.DwBwd(i), lambda c, y: c.finish(y)[0]) for i in range(len(X.DWBWD))]
    for name, c, fin in cases:
        A, B = c.operands()
        pa, pb = R.bf16x3_pieces(A), R.bf16x3_pieces(B)
        want = fin(c, R.as_int(A) @ R.as_int(B))
        for t in R.X3_TERMS:
            diff = fin(c, R.x3_model(pa, pb, {t: 0})) != want
            for r0 in range(0, diff.shape[0], X.FB_BM):
                for c0 in range(0, diff.shape[1], 96):
                    assert diff[r0:r0 + X.FB_BM, c0:c0 + 96].any(), (name, R.X3_TERM_NAMES[t], r0, c0)
    c = X.DwBwd(1)
    A, B = c.operands()
    pa, pb = R.bf16x3_pieces(A), R.bf16x3_pieces(B)
    _, dw, bn = c.finish(R.as_int(A) @ R.as_int(B))
    for t in R.X3_TERMS:                                       # the summed partial rows notice as well
        _, dw1, bn1 = c.finish(R.x3_model(pa, pb, {t: 0}))
        assert (dw1 != dw).any() and (bn1 != bn).any(), R.X3_TERM_NAMES[t]
