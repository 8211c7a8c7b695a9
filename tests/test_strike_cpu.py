"""The strike rule's host path (spnet_amd/fake_espi.py strike_params_host, strike_rows) against the Python-integer oracle
(tests/helpers/track_score_ref.py strike) and the properties the rule promises: bit equality, no tolerance."""
import numpy as np
import pytest

from spnet_amd import fake_espi as F
from spnet_amd import tracks as TK
from tests.helpers import track_score_ref as R


def assert_equals_oracle(got, want):
    waves, nodes, nnode, ident = got
    assert waves.dtype == np.float32 and nodes.dtype == np.float32 and nnode.dtype == np.int32 and ident.dtype == np.int32
    assert np.array_equal(waves, np.asarray(want[0], np.float32).reshape(-1, 5))
    assert np.array_equal(nodes, np.asarray(want[1], np.float32).reshape(-1, 7, 8))
    assert np.array_equal(nnode, np.asarray(want[2], np.int32)) and np.array_equal(ident, np.asarray(want[3], np.int32).reshape(-1, 7))


def hostile_base():
    waves0, nodes0, nnode0 = R.base_params(4, 2)
    nodes0[0, 0, 7] = 0                                        # the struck note is the second slot
    nodes0[1, :, 5] = (np.nan, -3, 300, 0, 1e9, 2.5, np.inf)    # ring counts outside 0 .. 255
    nnode0[:] = (7, 9, -2, 3)
    nodes0[:, :, 7] = np.where(nodes0[:, :, 0] > 0, nodes0[:, :, 7], 1)
    return waves0, nodes0, nnode0


@pytest.mark.parametrize("T,J,seed,first", [(1, 0, 0, 0), (2, 8, 1, 0), (9, 3, 0xFFFFFFFF, 5), (16, 8, 7, 306783370)])
def test_s1_host_equals_the_oracle(T, J, seed, first):
    for base in (R.base_params(5, 11), hostile_base()):
        assert_equals_oracle(F.strike_params_host(*base, T, seed, J, first), R.strike(*base, T, seed, J, first))


def test_s2_T_4096_on_one_sequence():
    base = R.base_params(1, 4)
    got = F.strike_params_host(*base, 4096, 3, 8)
    frames = [(0, t) for t in list(range(0, 4096, 97)) + [4095]]
    want = R.strike(*base, 4096, 3, 8, 0, frames)
    idx = [t for _, t in frames]
    assert_equals_oracle(tuple(a[idx] for a in got), want)
    assert got[3][0].max() > 0 and (got[1][..., 5].max(0) == base[1][0, :, 5] * (base[1][0, :, 7] != 0)).all()   # the peak is R


def test_s3_presence_is_one_run_and_J0_rows_do_not_move():
    base = R.base_params(6, 8)
    T = 24
    _, nodes, nnode, ident = F.strike_params_host(*base, T, 5, 0)
    nodes, ident = nodes.reshape(6, T, 7, 8), ident.reshape(6, T, 7)
    seen = 0
    for s in range(6):
        first_valid = True
        for j in range(7):
            p = np.flatnonzero(ident[s, :, j])
            if j >= base[2][s]:
                assert p.size == 0
                continue
            if first_valid:                                    # the struck note: there from frame 0, at its full count
                assert p[0] == 0 and nodes[s, 0, j, 5] == base[1][s, j, 5]
                first_valid = False
            if p.size == 0:
                continue
            seen += 1
            assert (np.diff(p) == 1).all(), "presence is not contiguous"
            assert (ident[s, p, j] == 1 + 7 * s + j).all()
            run = nodes[s, p, j]
            assert (run[:, [0, 1, 2, 3, 4, 6, 7]] == base[1][s, j, [0, 1, 2, 3, 4, 6, 7]]).all()
            r = run[:, 5]
            k = int(np.argmax(r))
            assert (np.diff(r[:k + 1]) >= 0).all() and (np.diff(r[k:]) <= 0).all() and r.min() >= 1 and r.max() <= base[1][s, j, 5]
            assert (nodes[s, :, j][ident[s, :, j] == 0] == 0).all()
    assert seen > 12
    # jitter moves the centres by at most J and nothing else
    _, nj, _, ij = F.strike_params_host(*base, T, 5, 8)
    nj = nj.reshape(6, T, 7, 8)
    assert np.array_equal(ij.reshape(6, T, 7), ident) and np.array_equal(nj[..., 2:], nodes[..., 2:])
    d = (nj[..., :2] - nodes[..., :2])[ident > 0]
    assert np.abs(d).max() == 8 and (d == np.rint(d)).all() and len(np.unique(d)) == 17


def test_s4_a_frame_depends_on_seed_sequence_and_time_only():
    base = R.base_params(7, 3)
    T = 6
    whole = F.strike_params_host(*base, T, 21, 4)
    for lo, hi in ((0, 1), (1, 4), (4, 7), (6, 7)):            # any split into calls, first_sequence moving along
        part = F.strike_params_host(*(a[lo:hi] for a in base), T, 21, 4, first_sequence=lo)
        for w, p in zip(whole, part):
            assert np.array_equal(w[lo * T:hi * T], p)
    other = F.strike_params_host(*base, T, 22, 4)
    assert not np.array_equal(other[1], whole[1])
    shifted = F.strike_params_host(*base, T, 21, 4, first_sequence=1)
    assert not np.array_equal(shifted[1], whole[1])
    empty = F.strike_params_host(base[0][:0], base[1][:0], base[2][:0], T)
    assert [a.shape for a in empty] == [(0, 5), (0, 7, 8), (0,), (0, 7)]


@pytest.mark.parametrize("kw", [dict(T=0), dict(T=4097), dict(jitter=-1), dict(jitter=9), dict(first_sequence=-1),
                                dict(first_sequence=(1 << 31) // 7)])
def test_s5_argument_errors(kw):
    base = R.base_params(2, 3)
    args = dict(T=4, seed=0, jitter=0, first_sequence=0)
    args.update(kw)
    with pytest.raises(ValueError):
        F.strike_params_host(*base, **args)


def test_s6_rows_are_compacted_with_their_identities_and_round_trip(tmp_path):
    base = hostile_base()
    T = 10
    _, nodes, nnode, ident = F.strike_params_host(*base, T, 2, 1)
    rows, count, idc = F.strike_rows(nodes, nnode, ident)
    assert rows.dtype == np.float64 and rows.shape == (4 * T, 7, 6) and count.dtype == np.int32 and idc.dtype == np.int32
    holes = 0
    for n in range(4 * T):
        keep = [j for j in range(7) if ident[n, j] > 0]
        holes += keep != list(range(len(keep)))
        assert count[n] == len(keep) and idc[n].tolist() == [int(ident[n, j]) for j in keep] + [0] * (7 - len(keep))
        assert np.array_equal(rows[n, :len(keep)], nodes[n, keep, :6].astype(np.float64)) and (rows[n, len(keep):] == 0).all()
    assert holes > 0, "no frame needed compaction"
    # through the CSV files the loaders read and the truth table
    names = ["steelpan_%07d.png" % n for n in range(T)]
    table = TK.write_truth_tracks(str(tmp_path / "truth_tracks.csv"), rows[:T], idc[:T], names)
    assert TK.read_truth_tracks(str(tmp_path / "truth_tracks.csv")) == table
    r2, c2, i2 = TK.truth_arrays(table, names=names)
    K = r2.shape[1]
    assert np.array_equal(c2, count[:T]) and np.array_equal(i2, idc[:T, :K]) and np.array_equal(r2, rows[:T, :K])
    first = {}
    for rec in table:
        assert rec[3] == rec[0] - first.setdefault(rec[2], rec[0]) and rec[1] == names[rec[0]]
    for n in range(T):
        text = F.rows_to_csv([tuple(r) for r in rows[n, :count[n]].astype(np.int64).tolist()])
        back = [tuple(float(v) for v in line.split(",")) for line in text.splitlines()]
        assert back == ([tuple(r) for r in rows[n, :count[n]].tolist()] if count[n] else [(0.0,) * 6])
