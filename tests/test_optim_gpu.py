"""The fused Adam + l2 step (csrc/optim.hip: spnet_adam_step, spnet_adam_part, spnet_adam_l2_sum, spnet_adam_parts) against
tests/helpers/optim_ref.py, bit for bit and behind guards.

The inputs are built so that every intermediate is an fp32 number (proved per case by tests/test_optim_ref_cpu.py), so p, m,
v, every sq_partial[b] and l2_loss_out[0] are demanded on their int32 views; g must come back unchanged; every tensor sits
between guard floats.  There is no tolerance in this file."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import optim_ref as R
from tests.test_dwconv_gpu import Dev, out, st, tag
from tests.test_irv2_glue_gpu import run_refusals
from tests.helpers.dw_ref import SENTINEL


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


HYPER = (R.BETA1, R.BETA2, R.EPS, R.L2, R.GRAD_SCALE)


def same_bits(d, want, name):
    """findings about a guarded tensor: the guards, then the int32 view of its contents"""
    found = d.guards()
    got, want = R.bits(d.head(d.n)), R.bits(want)
    bad = np.flatnonzero(got != want)
    if bad.size:
        found.append("%d elements differ, first at %d: %#x, expected %#x" % (bad.size, bad[0], got[bad[0]] & 0xFFFFFFFF, want[bad[0]] & 0xFFFFFFFF))
    return tag(found, name)


class Step:
    """the device side of one case: p, m, v between sentinels, g and the mask between NaN, the step size in device memory"""

    def __init__(self, inp):
        self.inp = inp
        self.p, self.m, self.v = (Dev(inp[k], SENTINEL) for k in "pmv")
        self.g = Dev(inp["g"])
        self.g0 = self.g.host().view(np.int32).copy()
        self.mask = None if inp["mask"] is None else Dev(inp["mask"])
        self.lr = None if inp["lr_dev"] is None else torch.full((1,), inp["lr_dev"], device="cuda")

    def args(self, lo, n, l2_n):
        q = lambda d: d.ptr + 4 * lo
        return (q(self.p), q(self.g), q(self.m), q(self.v), n, l2_n, self.inp["lr_arg"]) + HYPER + (None if self.mask is None else q(self.mask),)

    def lr_ptr(self):
        return None if self.lr is None else self.lr.data_ptr()

    def findings(self, want, sq, l2):
        torch.cuda.synchronize()
        found = []
        for k, d in (("p", self.p), ("m", self.m), ("v", self.v), ("sq_partial", sq), ("l2_loss_out", l2)):
            found += same_bits(d, want["l2_loss"] if d is l2 else want[k], k)
        if not np.array_equal(self.g.host().view(np.int32), self.g0):
            found.append("g was written")
        return found


def step_findings(L, case):
    inp = R.inputs(*case)
    want = R.adam(inp)
    s, sq, l2 = Step(inp), out(R.parts(inp["n"])), out(1)
    L.spnet_adam_step(*s.args(0, inp["n"], inp["l2_n"]), sq.ptr, l2.ptr, s.lr_ptr(), st())
    return tag(s.findings(want, sq, l2), "n %d l2_n %d mask %s lr from %s" % (case[0], case[1], case[2], "device" if case[3] else "argument"))


@pytest.mark.parametrize("n", R.SIZES)
def test_adam_step(L, n):
    found = []
    for case in R.cases():
        if case[0] == n:
            found += step_findings(L, case)
    assert found == []


@pytest.mark.parametrize("n", (1028, R.SIZES[-1]))
def test_adam_part_over_ranges_and_l2_sum(L, n):
    found = []
    for k, cuts in enumerate(((4,), (n - 4,), (4, n - 4))):
        for l2n in ((3, n - 1), (5, n + 7), (n, 2))[k][:2 if n == 1028 else 1]:        # one prefix per cut at the large size
            inp = R.inputs(n, l2n, "checkered", True)
            want = R.adam_in_ranges(inp, cuts)
            s, sq, l2 = Step(inp), out(want["sq_partial"].size), out(1)
            at = 0
            for lo, hi in R.ranges(n, cuts):
                L.spnet_adam_part(*s.args(lo, hi - lo, R.range_l2(l2n, lo, hi)), sq.ptr + 4 * at, s.lr_ptr(), st())
                at += int(L.spnet_adam_parts(hi - lo))
            assert at == sq.n
            L.spnet_adam_l2_sum(sq.ptr, at, R.L2, l2.ptr, st())
            found += tag(s.findings(want, sq, l2), "cuts %r l2_n %d" % (cuts, l2n))
    assert found == []


def test_adam_parts(L):
    sizes = (0, 3, 4, 1020, 1024, 1028, 2048 * 1024 - 4, 2048 * 1024, 2048 * 1024 + 4, 1 << 40)
    assert [int(L.spnet_adam_parts(n)) for n in sizes] == [R.parts(n) for n in sizes]
    assert int(L.spnet_adam_parts(3)) == 0 and int(L.spnet_adam_parts(1 << 40)) == 2048


@pytest.mark.parametrize("count", R.L2_SUM_COUNTS)
def test_adam_l2_sum(L, count):
    part = R.l2_sum_partials(count)
    src = Dev(part)
    found = []
    for l2 in (0.25, 1e-4):
        dst = out(1)
        L.spnet_adam_l2_sum(src.ptr, count, l2, dst.ptr, st())
        torch.cuda.synchronize()
        found += same_bits(dst, R.l2_sum(part, l2), "l2 %g" % l2)
    assert found == []


def test_adam_refusals_launch_nothing(L):
    """every tensor is 1028 elements behind its pointer and the partials 2048, more than any of these calls would touch if it
    were not refused (the sizes offered are at most 1026); the count above the cap reads from a buffer of that many floats"""
    n = 1028
    inp = R.inputs(n, n)
    s, sq, l2 = Step(inp), out(R.ADAM_BLOCKS), out(1)
    ptrs = s.args(0, n, n)[:4]
    tail = s.args(0, n, n)[6:]

    def step(p=ptrs, n=n, l2_n=n):
        return L.spnet_adam_step(*p, n, l2_n, *tail, sq.ptr, l2.ptr, None, st())

    def part(p=ptrs, n=n, l2_n=n):
        return L.spnet_adam_part(*p, n, l2_n, *tail, sq.ptr, None, st())

    many = Dev(np.zeros(R.L2_SUM_MAX + 1, np.float32))
    table = []
    for k, name in enumerate("pgmv"):
        null = ptrs[:k] + (None,) + ptrs[k + 1:]
        table += [("adam_step, %s NULL" % name, lambda null=null: step(p=null)), ("adam_part, %s NULL" % name, lambda null=null: part(p=null))]
    for bad in (-4, -1, 1, 2, 3, 6, 1026):
        table.append(("adam_step, n %d" % bad, lambda bad=bad: step(n=bad, l2_n=0)))
    for bad in (-4, 0, 3, 6, 1026):
        table.append(("adam_part, n %d" % bad, lambda bad=bad: part(n=bad, l2_n=0)))
    table += [("adam_l2_sum, partials NULL", lambda: L.spnet_adam_l2_sum(None, 4, R.L2, l2.ptr, st())),
              ("adam_l2_sum, out NULL", lambda: L.spnet_adam_l2_sum(sq.ptr, 4, R.L2, None, st())),
              ("adam_l2_sum, count 0", lambda: L.spnet_adam_l2_sum(sq.ptr, 0, R.L2, l2.ptr, st())),
              ("adam_l2_sum, count -1", lambda: L.spnet_adam_l2_sum(sq.ptr, -1, R.L2, l2.ptr, st())),
              ("adam_l2_sum, count above the cap", lambda: L.spnet_adam_l2_sum(many.ptr, R.L2_SUM_MAX + 1, R.L2, l2.ptr, st()))]
    wrong = run_refusals(L, table, (sq, l2))
    for k, d in (("p", s.p), ("m", s.m), ("v", s.v)):
        wrong += same_bits(d, inp[k], k + " after the refusals")
    assert wrong == []
    # n == 0 is an empty step, not a refusal: nothing moves, the penalty is 0
    L.spnet_adam_step(*ptrs, 0, 0, *tail, sq.ptr, l2.ptr, None, st())
    torch.cuda.synchronize()
    assert same_bits(l2, np.float32(0.0), "l2 of an empty step") == [] and same_bits(s.p, inp["p"], "p of an empty step") == []
    # and a valid call afterwards gives the right answer
    sq, l2 = out(R.parts(n)), out(1)
    L.spnet_adam_step(*s.args(0, n, n), sq.ptr, l2.ptr, None, st())
    assert s.findings(R.adam(inp), sq, l2) == []
