"""The case tables of tests/test_reduce_movers_gpu.py, proved on the CPU (tests/helpers/movers_ref.py): the reduction operands
are exact in fp32 in any order, the restated row assignment is the plain column sum, each planted defect changes a result of
the table, and the mover tables hold the payloads and shapes they are there for.  No GPU."""
import numpy as np
import pytest

from tests.helpers import movers_ref as R

PATHS = [(P, L, two) for P in R.ROWS for L in R.COLS for two in (False, True) if not two or P > R.TWO_PASS_ROWS]


def test_the_reduction_table_is_exact_and_the_model_is_the_column_sum():
    assert 128 in R.ROWS and 129 in R.ROWS and {15, 16, 17} <= set(R.COLS)
    for P, L, two in PATHS:
        for kind in ("ones", "ints"):
            x = R.reduce_data(P, L, kind)
            R.assert_exact(x)
            want = x.astype(np.float64).sum(axis=0)
            assert np.array_equal(R.reduce_model(x, two), want)
            if kind == "ones":
                assert (want == P).all()
            else:
                assert np.abs(x).max() == 7 or P * L < 20
    for P, L in R.BATCH_JOBS:
        R.assert_exact(R.reduce_data(P, L, "ints"))
    Ls = [L for _, L in R.BATCH_JOBS]
    assert 1 in Ls and min(Ls) < max(Ls) == 40 and {P for P, _ in R.BATCH_JOBS} == set(R.ROWS)
    assert R.takes_two_passes(129, True) and not R.takes_two_passes(128, True) and not R.takes_two_passes(129, False)


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_the_reduction_table_notices_the_planted_defect(defect):
    hits = {}
    for kind in ("ones", "ints"):
        hits[kind] = [(P, L, two) for P, L, two in PATHS
                      if not np.array_equal(R.reduce_model(R.reduce_data(P, L, kind), two, defect), R.reduce_data(P, L, kind).astype(np.float64).sum(axis=0))]
    assert hits["ones"] and hits["ints"], defect
    print(defect, "-> ones: %d of %d paths, first %r" % (len(hits["ones"]), len(PATHS), hits["ones"][0]))


def test_the_mover_tables():
    assert max(r for r, _ in R.TRANSPOSE_JOBS) == 65 == max(c for _, c in R.TRANSPOSE_JOBS) and (65, 65) not in R.TRANSPOSE_JOBS
    assert len(R.TRANSPOSE_JOBS) == 24
    b = R.payload_bits(4096, 5)
    f = R.as_floats(b)
    assert np.isnan(f).sum() > 1000 and (b == np.int32(-2 ** 31)).sum() > 100 and len(set(b[np.isnan(f)].tolist())) > 1000
    assert np.array_equal(R.as_floats(b).view(np.int32), b)
    B, H, W, C = R.S2_CAP
    assert B * ((H + 1) // 2) * ((W + 1) // 2) * (C // 4) > R.EW_CAP_ITEMS and B * H * W * C * 4 < 136e6
    assert len(R.S2_SHAPES) == 64
    for shape in R.S2_SHAPES[:8] + R.S2_SHAPES[-8:]:
        dxs, dx, want = R.scatter_case(*shape, 3)
        odd = np.ones(dx.shape, bool)
        odd[:, ::2, ::2, :] = False
        assert np.isnan(dx[odd]).all() and np.array_equal(want[odd], dx.view(np.int32)[odd])
        assert np.array_equal(R.as_floats(want)[~odd], (dx[~odd].astype(np.float64) + dxs.ravel()).astype(np.float32))
        assert R.gather_s2(dx).shape == dxs.shape
