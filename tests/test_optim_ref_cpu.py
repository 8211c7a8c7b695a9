"""The case table of tests/test_optim_gpu.py, proved on the CPU (tests/helpers/optim_ref.py): every intermediate of every
case is an fp32 number, so the kernel's result does not depend on contraction or order; the sums of squares are exact; and
each planted defect changes at least one output of the table.  No GPU."""
import numpy as np
import pytest

from tests.helpers import optim_ref as R

SMALL_CASES = [c for c in R.cases() if c[0] in R.SMALL]
LARGE_CASES = [c for c in R.cases() if c[0] not in R.SMALL]


def test_the_table_holds_what_the_issue_lists():
    t = R.cases()
    assert {c[0] for c in t} == set(R.SIZES) and R.SIZES[-1] > R.ADAM_BLOCKS * 256 * 4          # the second sweep runs
    for n in R.SIZES:
        assert {c[1] for c in t if c[0] == n} == {0, 1, 2, 3, 5, n - 1, n, n + 7}
        assert {c[2] for c in t if c[0] == n} == set(R.MASKS) and {c[3] for c in t if c[0] == n} == {False, True}
    chk = R.mask_of("checkered", 20).reshape(5, 4)
    assert all(any(row[k] == 0 and row.sum() == 3 for row in chk) for k in range(4))            # each lane frozen alone
    assert R.LR_ARG != R.LR_DEV


def test_every_small_case_is_exact_in_fp32():
    for c in SMALL_CASES:
        R.adam(R.inputs(*c), check=True)


@pytest.mark.parametrize("case", LARGE_CASES, ids=lambda c: "n%d-l2n%d-%s-%s" % (c[0], c[1], c[2], "dev" if c[3] else "arg"))
def test_every_large_case_is_exact_in_fp32(case):
    got = R.adam(R.inputs(*case), check=True)
    assert got["sq_partial"].size == R.ADAM_BLOCKS
    if case[1] >= case[0] and case[0] > R.ADAM_BLOCKS * 1024:
        # the second sweep: workgroup 0 also holds the items 2048 * 256 .. of the tail, workgroup 2 does not
        p = R.inputs(*case)["p"].astype(np.float64)
        assert got["sq_partial"][0] == (p[:1024] ** 2).sum() + (p[R.ADAM_BLOCKS * 1024:R.ADAM_BLOCKS * 1024 + 1024] ** 2).sum()
        assert got["sq_partial"][2] == (p[2048:3072] ** 2).sum()


def test_the_update_moves_every_output_and_eps_matters():
    inp = R.inputs(1028, 1028)
    got = R.adam(inp, check=True)
    assert (got["m"] != inp["m"]).mean() > 0.5 and (got["v"] != inp["v"]).mean() > 0.5 and (got["p"] != inp["p"]).mean() > 0.5
    assert set(np.sqrt(got["v"]).tolist()) == {1.0, 3.0, 7.0}
    assert got["l2_loss"] == np.float32(R.L2 * (inp["p"].astype(np.float64) ** 2).sum())


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_table_notices_the_planted_defect(defect):
    hits = [c for c in SMALL_CASES if R.outputs_differ(R.adam(R.inputs(*c)), R.adam(R.inputs(*c), defect=defect))]
    assert hits, defect
    print(defect, "-> %d of %d small cases differ, first %r" % (len(hits), len(SMALL_CASES), hits[0]))


def test_frozen_elements_keep_their_bits_and_still_count():
    inp = R.inputs(1028, 1028, "checkered")
    got, free = R.adam(inp), R.adam(R.inputs(1028, 1028, "none"))
    frozen = inp["mask"] == 0
    for k in "pmv":
        assert np.array_equal(R.bits(got[k])[frozen], R.bits(inp[k])[frozen])
        assert np.array_equal(got[k][~frozen], free[k][~frozen])
    assert np.array_equal(got["sq_partial"], free["sq_partial"])


def test_ranges_restate_the_whole_step():
    for n in (1028, 2048 * 1024 + 4 * 257):
        for cuts in ((4,), (n - 4,), (4, n - 4)):
            for l2n in (3, 5, n - 1, n + 7):
                got = R.adam_in_ranges(R.inputs(n, l2n, "checkered", True), cuts)
                assert got["sq_partial"].size == sum(R.parts(hi - lo) for lo, hi in R.ranges(n, cuts))
    assert [R.parts(n) for n in (0, 3, 4, 1024, 1028, 2048 * 1024, 2048 * 1024 + 4, 1 << 40)] == [0, 0, 1, 1, 2, 2048, 2048, 2048]


def test_l2_sum_partials_are_exact_in_double_only():
    for count in R.L2_SUM_COUNTS:
        part = R.l2_sum_partials(count)
        assert np.array_equal(part, np.round(part)) and part.astype(np.float64).sum() < 2.0 ** 53
    big = R.l2_sum_partials(4096)
    assert big.astype(np.float64).sum() > 2.0 ** 24                     # an fp32 accumulation would round
    assert float(R.l2_sum(big, 0.25)) == float(np.float32(big.astype(np.float64).sum() * 0.25))
