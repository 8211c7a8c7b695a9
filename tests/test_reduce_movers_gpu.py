"""The row reductions of csrc/dwconv.hip (spnet_reduce_rows, _ws, _batched) and the movers of csrc/gemm.hip
(spnet_transpose_batched, spnet_gather_s2, spnet_scatter_add_s2) against tests/helpers/movers_ref.py, behind guards.

Reductions add integers, so the fp32 sum is the integer sum in any order; copies are compared on the int32 view.  Every
output sits between (and is filled with) the sentinel, the scratch of the two-pass path is exactly 32 * L floats of NaN.
There is no tolerance in this file: every assertion is an equality or an empty list of findings."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import movers_ref as R
from tests.helpers.dw_ref import SENTINEL
from tests.test_dwconv_gpu import Dev, out, st, tag, work
from tests.test_irv2_glue_gpu import run_refusals


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def bits_findings(d, want_bits, name):
    found = d.guards()
    got = d.head(d.n).view(np.int32)
    bad = np.flatnonzero(got != np.asarray(want_bits, np.int32).ravel())
    if bad.size:
        found.append("%d elements differ, first at %d" % (bad.size, bad[0]))
    return tag(found, name)


def jobs_table(rows):
    return torch.tensor(rows, dtype=torch.int64, device="cuda")


# ---- reductions --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lc", R.COLS)
def test_reduce_rows_every_path(L, Lc):
    found = []
    for P in R.ROWS:
        for kind in ("ones", "ints"):
            x = R.reduce_data(P, Lc, kind)
            want = x.astype(np.float64).sum(axis=0)
            src = Dev(x)
            o1, o2, o3, o4, scratch = out(Lc), out(Lc), out(Lc), out(Lc), work(32 * Lc)
            L.spnet_reduce_rows(src.ptr, P, Lc, o1.ptr, st())
            L.spnet_reduce_rows_ws(src.ptr, P, Lc, o2.ptr, scratch.ptr, 32 * Lc, st())
            L.spnet_reduce_rows_ws(src.ptr, P, Lc, o3.ptr, None, 0, st())
            jobs = jobs_table([[src.ptr, o4.ptr, P, Lc]])
            L.spnet_reduce_rows_batched(jobs.data_ptr(), 1, Lc, st())
            torch.cuda.synchronize()
            for name, o in (("reduce_rows", o1), ("reduce_rows_ws", o2), ("reduce_rows_ws without scratch", o3), ("reduce_rows_batched", o4)):
                found += tag(o.check(want), "%s P %d %s" % (name, P, kind))
            found += tag(scratch.guards(), "scratch P %d" % P)
            written = ~np.isnan(scratch.head(32 * Lc))
            if written.any() != R.takes_two_passes(P, True) or (written.any() and not written.all()):
                found.append("scratch P %d: %d of %d floats written" % (P, written.sum(), written.size))
    assert found == []


def test_reduce_rows_batched_mixed_jobs_side_by_side(L):
    found = []
    for kind in ("ones", "ints"):
        data = [R.reduce_data(P, Lj, kind) for P, Lj in R.BATCH_JOBS]
        srcs = [Dev(x) for x in data]
        total = sum(Lj for _, Lj in R.BATCH_JOBS)
        dst = out(total)
        rows, at = [], 0
        for (P, Lj), s in zip(R.BATCH_JOBS, srcs):
            rows.append([s.ptr, dst.ptr + 4 * at, P, Lj])
            at += Lj
        jobs = jobs_table(rows)
        L.spnet_reduce_rows_batched(jobs.data_ptr(), len(rows), max(Lj for _, Lj in R.BATCH_JOBS), st())
        torch.cuda.synchronize()
        found += tag(dst.check(np.concatenate([x.astype(np.float64).sum(axis=0) for x in data])), kind)
    assert found == []


# ---- transpose ---------------------------------------------------------------------------------------------------------------
def test_transpose_batched_mixed_shapes(L):
    srcs = [R.as_floats(R.payload_bits(r * c, 17 * k)).reshape(r, c) for k, (r, c) in enumerate(R.TRANSPOSE_JOBS)]
    devs = [Dev(x) for x in srcs]
    dst = out(sum(x.size for x in srcs))
    rows, at = [], 0
    for x, d in zip(srcs, devs):
        rows.append([d.ptr, dst.ptr + 4 * at, x.shape[0], x.shape[1]])
        at += x.size
    jobs = jobs_table(rows)
    L.spnet_transpose_batched(jobs.data_ptr(), len(rows), 65, 65, st())
    torch.cuda.synchronize()
    want = np.concatenate([np.ascontiguousarray(x.T).view(np.int32).ravel() for x in srcs])
    assert bits_findings(dst, want, "transposes") == []


# ---- stride-2 gather / scatter -----------------------------------------------------------------------------------------------
def s2_findings(L, shape, seed):
    B, H, W, C = shape
    x = R.as_floats(R.payload_bits(B * H * W * C, seed)).reshape(B, H, W, C)
    want = R.gather_s2(x)
    src, xs = Dev(x), out(want.size)
    L.spnet_gather_s2(src.ptr, xs.ptr, B, H, W, C, st())
    dxs, dx, want_dx = R.scatter_case(B, H, W, C, seed)
    up, acc = Dev(dxs), Dev(dx, SENTINEL)
    L.spnet_scatter_add_s2(up.ptr, acc.ptr, B, H, W, C, st())
    torch.cuda.synchronize()
    return bits_findings(xs, want.view(np.int32), "gather %r" % (shape,)) + bits_findings(acc, want_dx, "scatter %r" % (shape,))


def test_gather_and_scatter_s2(L):
    found = []
    for k, shape in enumerate(R.S2_SHAPES):
        found += s2_findings(L, shape, 3 + k)
    assert found == []


def test_gather_and_scatter_s2_past_the_grid_cap(L):
    assert s2_findings(L, R.S2_CAP, 1) == []


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_reduce_and_mover_refusals_launch_nothing(L):
    """z: 16384 zeros behind every input, o / o2: 8192 sentinels behind every output -- more than any of these calls would
    touch if it were NOT refused (the shapes offered stay below 64 x 40 and 1 x 4 x 4 x 8).  The table of 65536 jobs holds
    valid one-element jobs."""
    z, o, o2 = Dev(np.zeros(16384, np.float32)), out(8192), out(8192)
    s = st()
    rr = lambda i=z.ptr, P=64, Lc=40, d=o.ptr: L.spnet_reduce_rows(i, P, Lc, d, s)
    ws = lambda i=z.ptr, P=200, Lc=40, d=o.ptr, sc=o2.ptr, n=32 * 40: L.spnet_reduce_rows_ws(i, P, Lc, d, sc, n, s)
    many = jobs_table([[z.ptr, o2.ptr, 1, 1]] * 65536)
    one = jobs_table([[z.ptr, o.ptr, 4, 4]])
    rb = lambda j=one.data_ptr(), n=1, m=4: L.spnet_reduce_rows_batched(j, n, m, s)
    tb = lambda j=one.data_ptr(), n=1, r=4, c=4: L.spnet_transpose_batched(j, n, r, c, s)
    ga = lambda x=z.ptr, d=o.ptr, g=(1, 4, 4, 8): L.spnet_gather_s2(x, d, *g, s)
    sc = lambda x=z.ptr, d=o.ptr, g=(1, 4, 4, 8): L.spnet_scatter_add_s2(x, d, *g, s)
    table = [("reduce_rows, in NULL", lambda: rr(i=None)), ("reduce_rows, out NULL", lambda: rr(d=None)),
             ("reduce_rows_ws, in NULL", lambda: ws(i=None)), ("reduce_rows_ws, out NULL", lambda: ws(d=None)),
             ("reduce_rows_ws, scratch one float short", lambda: ws(n=32 * 40 - 1)), ("reduce_rows_ws, scratch_floats -1", lambda: ws(n=-1)),
             ("reduce_rows_ws, scratch NULL with 1280 floats", lambda: ws(sc=None)), ("reduce_rows_ws, scratch NULL with -1 floats", lambda: ws(sc=None, n=-1)),
             ("reduce_rows_batched, jobs NULL", lambda: rb(j=None)), ("reduce_rows_batched, njobs 0", lambda: rb(n=0)),
             ("reduce_rows_batched, njobs -1", lambda: rb(n=-1)), ("reduce_rows_batched, max_L 0", lambda: rb(m=0)),
             ("reduce_rows_batched, max_L -1", lambda: rb(m=-1)), ("reduce_rows_batched, njobs 65536", lambda: rb(j=many.data_ptr(), n=65536, m=1)),
             ("transpose_batched, jobs NULL", lambda: tb(j=None)), ("transpose_batched, njobs 0", lambda: tb(n=0)),
             ("transpose_batched, max_rows 0", lambda: tb(r=0)), ("transpose_batched, max_cols 0", lambda: tb(c=0)),
             ("transpose_batched, max_rows -1", lambda: tb(r=-1)), ("transpose_batched, max_cols -1", lambda: tb(c=-1)),
             ("transpose_batched, njobs 65536", lambda: tb(j=many.data_ptr(), n=65536, r=1, c=1)),
             ("transpose_batched, max_rows 65535 * 32 + 1", lambda: tb(r=65535 * 32 + 1))]
    for bad in (0, -1):
        table += [("reduce_rows, P %d" % bad, lambda bad=bad: rr(P=bad)), ("reduce_rows, L %d" % bad, lambda bad=bad: rr(Lc=bad)),
                  ("reduce_rows_ws, P %d" % bad, lambda bad=bad: ws(P=bad)), ("reduce_rows_ws, L %d" % bad, lambda bad=bad: ws(Lc=bad))]
    for name, call in (("gather_s2", ga), ("scatter_add_s2", sc)):
        table += [(name + ", source NULL", lambda call=call: call(x=None)), (name + ", destination NULL", lambda call=call: call(d=None))]
        for k, what in enumerate("BHW"):
            for bad in (0, -1):
                g = (1, 4, 4, 8)[:k] + (bad,) + (1, 4, 4, 8)[k + 1:]
                table.append(("%s, %s %d" % (name, what, bad), lambda call=call, g=g: call(g=g)))
        for bad in (0, -4, 2, 6):
            table.append(("%s, C %d" % (name, bad), lambda call=call, bad=bad: call(g=(1, 4, 4, bad))))
    assert run_refusals(L, table, (o, o2)) == []
    # valid calls afterwards still give the right answers
    x = R.reduce_data(200, 40, "ints")
    src, dst, scratch = Dev(x), out(40), work(32 * 40)
    L.spnet_reduce_rows_ws(src.ptr, 200, 40, dst.ptr, scratch.ptr, 32 * 40, s)
    torch.cuda.synchronize()
    assert dst.check(x.astype(np.float64).sum(axis=0)) == []
    assert s2_findings(L, (1, 4, 4, 8), 9) == []
