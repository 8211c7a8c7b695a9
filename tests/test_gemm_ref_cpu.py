"""tests/helpers/gemm_ref.py and the tables of tests/test_gemm_gpu.py, without a GPU: the checker finds what a subtly wrong
strided GEMM does (numpy models of a correct kernel and of eight broken ones), assert_exact rejects operands that are not
exact, the patch-matrix restatement agrees with the oracle's convolution, and spnet_gemm_plan (host only) confirms that
every row of the GPU tables takes the path it is there for."""
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
