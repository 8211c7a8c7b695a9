"""csrc/tracks.hip through spnet_amd/tracks.py and through the raw entry points against the Python-integer oracle
(tests/helpers/tracks_ref.py): exact equality of area, every inter of every pass, next, prev, track and age on the whole
case table.  No tolerance appears anywhere.  The cases' angles pass mask_ref.assert_trig_safe (tests/test_tracks_cpu.py
checks the table; the tests here check what they build themselves).

Shapes are the smallest at which the kernels can still go wrong: 48 x 80, 17 x 70 and 33 x 130 (interior, edge and partial
tiles of the 64 x 16 tiling, up to 3 x 3 tiles), 16 x 64 (exactly one tile); N 1, 2, 3, 9, 33 (a non-power of two for the
pointer jumping) and 40; K 4, 72 and 128 (the whole LDS table, both halves of the 128-bit sets); gaps 1 .. 4."""
import os

import numpy as np
import pytest
import torch

from spnet_amd import masks as MK
from spnet_amd import tracks as TK
from tests.helpers import mask_ref as MR
from tests.helpers import tracks_ref as R
from tests.test_tracks_cpu import _grids, assert_equals_oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = "hipError_t 1$"           # hipErrorInvalidValue
CASES = list(range(len(R.cases())))
IDS = [c.name for c in R.cases()]
GUARD, PATTERN, CANARY = 8, 0x5A5A5A5A, 0x7E7E7E7E


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _dev(case):
    return (torch.from_numpy(np.ascontiguousarray(case.rows, np.float64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(case.count, np.int32)).cuda())


class Guarded:
    """An int32 device array of n elements with GUARD canary words before and after it, pre-filled with a pattern."""

    def __init__(self, n, fill=PATTERN):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.buf[GUARD:GUARD + n] = fill
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self, shape):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + self.n:] == CANARY).all(), "a canary was overwritten"
        return h[GUARD:GUARD + self.n].reshape(shape).copy()


def _raw(case, pairs_per_chunk=None):
    """The four entry points as link_tracks_device calls them, into guarded, pre-filled arrays; (track, age, next, prev,
    area, {d: inter}).  Checks the canaries and that every element of area, inter, track and age was written."""
    from spnet_amd import _lib as L
    rows, count = _dev(case)
    N, K = case.rows.shape[:2]
    st = L.current_stream()
    area, track, age = Guarded(N * K), Guarded(N * K), Guarded(N * K)
    nxt, prv = Guarded(N * K, -1), Guarded(N * K, -1)
    rp, cp = rows.data_ptr(), count.data_ptr()
    L.spnet_track_area(rp, cp, N, K, case.H, case.W, area.ptr, st)
    inters = {}
    for d in range(1, case.G + 1):
        per = pairs_per_chunk or max(N - d, 1)
        got = []
        for t0 in range(0, max(N - d, 0), per):
            n = min(per, N - d - t0)
            inter = Guarded(n * K * K)
            L.spnet_track_overlap(rp, cp, N, K, case.H, case.W, t0, n, d, inter.ptr, st)
            L.spnet_track_link(inter.ptr, area.ptr, rp, cp, N, K, t0, n, d, case.iou_q, nxt.ptr, prv.ptr, st)
            got.append(inter.host((n, K, K)))
        inters[d] = np.concatenate(got) if got else np.zeros((0, K, K), np.int32)
    ws_bytes = L.spnet_track_rank_ws(N, K)
    assert ws_bytes == 16 * N * K
    ws = Guarded(ws_bytes // 4)
    L.spnet_track_rank(prv.ptr, rp, cp, N, K, track.ptr, age.ptr, ws.ptr, st)
    ws.host((-1,))                                              # the canaries around the workspace
    out = tuple(g.host((N, K)) for g in (track, age, nxt, prv, area))
    for name, a in zip(("track", "age", "area"), (out[0], out[1], out[4])):
        assert (a != PATTERN).all(), name + " has unwritten elements"
    assert all((i != PATTERN).all() for i in inters.values()), "inter has unwritten elements"
    return out + (inters,)


@pytest.mark.parametrize("index", CASES, ids=IDS)
def test_g1_entry_points_equal_the_oracle(index):
    _need_gpu()
    case = R.cases()[index]
    got = _raw(case)
    assert_equals_oracle(got[:5], R.oracle(index), case, got[5])


@pytest.mark.parametrize("index", CASES, ids=IDS)
def test_g2_link_tracks_device_equals_the_oracle(index):
    _need_gpu()
    case = R.cases()[index]
    rows, count = _dev(case)
    got = TK.link_tracks_device(rows, count, case.H, case.W, iou=case.iou_q / 1024.0, max_gap=case.G, return_inter=True)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got[:5])
    assert_equals_oracle([t.cpu().numpy() for t in got[:5]], R.oracle(index), case, {d: v.cpu().numpy() for d, v in got[5].items()})


@pytest.mark.parametrize("name", ["seeded flicker, gap 4", "72 rows a frame, gap 3", "one chain through 33 frames",
                                  "128 rows piled on one tile"])
def test_g3_one_pair_a_chunk_and_a_second_run_give_the_same_tensors(name):
    _need_gpu()
    case = R.case_named(name)
    rows, count = _dev(case)
    kw = dict(H=case.H, W=case.W, iou=case.iou_q / 1024.0, max_gap=case.G)
    whole = TK.link_tracks_device(rows, count, **kw)
    again = TK.link_tracks_device(rows, count, **kw)
    single = TK.link_tracks_device(rows, count, ws_bytes=1, **kw)
    host = TK.link_tracks_host(case.rows, case.count, **kw)
    for a, b, c, h in zip(whole, again, single, host):
        assert torch.equal(a, b) and torch.equal(a, c) and np.array_equal(a.cpu().numpy(), h)
    got = _raw(case, pairs_per_chunk=1)                          # the raw calls, one pair a launch, guarded
    assert_equals_oracle(got[:5], R.oracle(IDS.index(name)), case, got[5])


def test_g4_host_input_and_empty_input():
    _need_gpu()
    case = R.case_named("two that cross")
    want = R.oracle(IDS.index(case.name))
    got = TK.link_tracks_device(case.rows, case.count, case.H, case.W, iou=case.iou_q / 1024.0, max_gap=case.G)
    assert_equals_oracle([t.cpu().numpy() for t in got], want, case)
    labels = [[tuple(r) for r in case.rows[t, :case.count[t]]] for t in range(case.rows.shape[0])]
    got = TK.link_tracks_device(labels, None, case.H, case.W, iou=case.iou_q / 1024.0, max_gap=case.G)
    assert np.array_equal(got[0].cpu().numpy()[:, :4], want.track) and got[0].shape[1] >= 4
    empty = TK.link_tracks_device(torch.zeros((0, 4, 6), dtype=torch.float64, device="cuda"), None, 8, 8, return_inter=True)
    assert all(tuple(t.shape) == (0, 4) for t in empty[:5]) and tuple(empty[5][1].shape) == (0, 4, 4)
    with pytest.raises(TypeError):
        TK.link_tracks_device(torch.zeros((2, 4, 6), dtype=torch.float32, device="cuda"), None, 8, 8)
    with pytest.raises(ValueError):
        TK.link_tracks_device(torch.zeros((2, 4, 6), dtype=torch.float64, device="cuda"), None, 8, 8, max_gap=9)


def test_g5_tracks_from_predictions_equals_the_oracle_on_prediction_rows():
    """Hand-built de-normalised grids, no model: 72 predictors a frame, four of them alive, on a 384 x 512 frame cut to its
    upper left 200 x 330 for the oracle's sake (brute force over every pixel)."""
    _need_gpu()
    H, W, G = 200, 330, 2
    Y = _grids(4, 1)
    Y.reshape(4, 72, 8)[:, 40, 0] -= 200.0                       # bring the third ellipse into the cut frame
    Y.reshape(4, 72, 8)[:, 40, 1] -= 150.0
    rows = MK.prediction_rows(Y)
    MR.assert_trig_safe(rows[..., 4])
    want = R.link(rows, np.full(4, 72), H, W, G, 256)
    assert want.live.sum() == 15 and (want.next >= 0).sum() >= 10 and want.age.max() == 3
    for Yin in (Y, torch.from_numpy(Y).cuda()):
        got = TK.tracks_from_predictions(Yin, H, W, iou=0.25, max_gap=G)
        assert got[0].is_cuda and tuple(got[0].shape) == (4, 72, 6)
        for t in range(4):                                       # the rows quantise to the same integers
            for k in np.flatnonzero(want.live[t]):
                assert MR.quantise(got[0][t, k].cpu().numpy())[:6] == MR.quantise(rows[t, k])[:6]
        case = R.Case("predictions", H, W, 72, G, 256, rows, np.full(4, 72))
        assert_equals_oracle([t.cpu().numpy() for t in got[1:]], want, case)
    host = TK.tracks_from_predictions(Y, H, W, iou=0.25, max_gap=G, host=True)
    assert all(np.array_equal(h, g.cpu().numpy()) for h, g in zip(host[1:], got[1:]))


def test_g6_invalid_arguments_write_nothing():
    _need_gpu()
    from spnet_amd import _lib as L
    N, K, H, W = 3, 4, 16, 64
    case = R.Case("valid", H, W, K, 1, 256, *R.pack([[(20, 8, 6, 4, 0, 1)]] * N, K))
    rows, count = _dev(case)
    st = L.current_stream()
    r, c = rows.data_ptr(), count.data_ptr()
    out = {k: Guarded(N * K * K) for k in ("area", "inter", "next", "prev", "track", "age", "ws")}
    a, i, nx, pv, tr, ag, ws = (out[k].ptr for k in ("area", "inter", "next", "prev", "track", "age", "ws"))
    bad_area = [(None, c, N, K, H, W, a), (r, None, N, K, H, W, a), (r, c, N, K, H, W, None), (r, c, -1, K, H, W, a),
                (r, c, N, 0, H, W, a), (r, c, N, 129, H, W, a), (r, c, N, K, 0, W, a), (r, c, N, K, H, 0, a),
                (r, c, N, K, 16385, W, a), (r, c, N, K, H, 16385, a), (r + 4, c, N, K, H, W, a), (r, c + 2, N, K, H, W, a),
                (r, c, N, K, H, W, a + 2), (r, c, 1 << 24, 128, H, W, a)]
    bad_overlap = [(None, c, N, K, H, W, 0, 2, 1, i), (r, None, N, K, H, W, 0, 2, 1, i), (r, c, N, K, H, W, 0, 2, 1, None),
                   (r, c, N, K, H, W, 0, 2, 0, i), (r, c, N, K, H, W, 0, 2, 9, i), (r, c, N, K, H, W, -1, 2, 1, i),
                   (r, c, N, K, H, W, 0, -1, 1, i), (r, c, N, K, H, W, 0, 3, 1, i), (r, c, N, K, H, W, 1, 2, 1, i),
                   (r, c, N, K, H, W, 0, 2, 2, i), (r, c, N, K, H, W, 2147483647, 2, 1, i), (r, c, N, 129, H, W, 0, 2, 1, i),
                   (r, c, N, K, 0, W, 0, 2, 1, i), (r, c, N, K, H, W, 0, 2, 1, i + 2), (r + 4, c, N, K, H, W, 0, 2, 1, i)]
    bad_link = [(None, a, r, c, N, K, 0, 2, 1, 256, nx, pv), (i, None, r, c, N, K, 0, 2, 1, 256, nx, pv),
                (i, a, None, c, N, K, 0, 2, 1, 256, nx, pv), (i, a, r, None, N, K, 0, 2, 1, 256, nx, pv),
                (i, a, r, c, N, K, 0, 2, 1, 256, None, pv), (i, a, r, c, N, K, 0, 2, 1, 256, nx, None),
                (i, a, r, c, N, K, 0, 2, 1, 0, nx, pv), (i, a, r, c, N, K, 0, 2, 1, 1025, nx, pv),
                (i, a, r, c, N, K, 0, 3, 1, 256, nx, pv), (i, a, r, c, N, K, 0, 2, 9, 256, nx, pv),
                (i, a, r, c, N, 0, 0, 2, 1, 256, nx, pv), (i, a, r, c, N, K, 0, 2, 1, 256, nx + 2, pv),
                (i + 2, a, r, c, N, K, 0, 2, 1, 256, nx, pv), (i, a, r, c, N, K, 0, 2, 1, 256, nx, pv + 1)]
    bad_rank = [(None, r, c, N, K, tr, ag, ws), (pv, None, c, N, K, tr, ag, ws), (pv, r, None, N, K, tr, ag, ws),
                (pv, r, c, N, K, None, ag, ws), (pv, r, c, N, K, tr, None, ws), (pv, r, c, N, K, tr, ag, None),
                (pv, r, c, -1, K, tr, ag, ws), (pv, r, c, N, 129, tr, ag, ws), (pv, r, c, N, K, tr + 2, ag, ws),
                (pv, r, c, N, K, tr, ag, ws + 1), (pv + 2, r, c, N, K, tr, ag, ws)]
    for fn, table in ((L.spnet_track_area, bad_area), (L.spnet_track_overlap, bad_overlap), (L.spnet_track_link, bad_link),
                      (L.spnet_track_rank, bad_rank)):
        for args in table:
            with pytest.raises(L.HipError, match=INVALID):
                fn(*args, st)
    assert L.spnet_track_rank_ws(1 << 24, 128) == -1 and L.spnet_track_rank_ws(2, 0) == -1 and L.spnet_track_rank_ws(0, 4) == 16
    torch.cuda.synchronize()
    for g in out.values():
        assert (g.host((-1,)) == PATTERN).all()
    got = _raw(case)                                             # the same arguments, valid: one track through the frames
    assert got[0][:, 0].tolist() == [1, 1, 1] and got[1][:, 0].tolist() == [0, 1, 2]


def test_g7_predict_network_writes_both_tables(tmp_path):
    """predict_network(tracks=PATH) with a freshly initialised model on four small fake-ESPI frames: both CSV files exist,
    their rows are detections of hawley_spnet.csv's frames, and a run without tracks writes byte-identical other outputs."""
    _need_gpu()
    import predict_spnet
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    data = tmp_path / "frames"
    F.write_dataset(str(data) + "/", 4, seed=6)
    names = sorted(p for p in os.listdir(data) if p.endswith(".png"))
    saved = cf.model_type
    try:
        cf.model_type = 'monolithic'
        model = M.Model((331, 331, 1), Y0size=576, seed=8)
        plain, tracked = str(tmp_path / "plain") + "/", str(tmp_path / "tracked") + "/"
        predict_spnet.predict_network(datapath=str(data), log_dir=plain, batch_size=4, model=model)
        path = str(tmp_path / "out" / "tracks.csv")
        os.makedirs(os.path.dirname(path))
        predict_spnet.predict_network(datapath=str(data), log_dir=tracked, batch_size=4, model=model, tracks=path,
                                      track_iou=0.25, track_gap=2, track_min_len=1)
    finally:
        cf.model_type = saved
    assert sorted(os.listdir(plain)) == sorted(os.listdir(tracked)) and "hawley_spnet.csv" in os.listdir(plain)
    for f in os.listdir(plain):
        assert open(plain + f, "rb").read() == open(tracked + f, "rb").read(), f
    table = [l.split(",") for l in open(path).read().splitlines()]
    summary = [l.split(",") for l in open(TK.summary_path(path)).read().splitlines()]
    assert tuple(table[0]) == TK.TABLE_FIELDS and tuple(summary[0]) == TK.SUMMARY_FIELDS
    hawley = [l.split(",") for l in open(plain + "hawley_spnet.csv").read().splitlines()]
    drawn = {(h[2], int(h[0]), int(h[1])) for h in hawley}      # (file, cx, cy) as cleanup_antinode_vars rounds them
    assert {h[2] for h in hawley} == set(names)
    n_of = {}
    for frame, name, track, age, cx, cy, a, b, angle, rings in table[1:]:
        assert name == names[int(frame)] and int(track) >= 1 and 0 <= int(age) <= int(frame)
        n_of[track] = n_of.get(track, 0) + 1
        # a tracked detection with rings above 0 and whole-number axes above 0 is a row of hawley_spnet.csv
        if float(rings) > 0 and round(float(a)) >= 0 and round(float(b)) >= 0:
            assert (name, int(round(float(cx))), int(round(float(cy)))) in drawn, (name, cx, cy)
    assert [s[0] for s in summary[1:]] == sorted(n_of, key=int) and all(int(s[3]) == n_of[s[0]] for s in summary[1:])
    assert all(int(s[1]) <= int(s[6]) <= int(s[2]) for s in summary[1:])
