"""csrc/track_score.hip through the raw entry points and through spnet_amd/tracks.py against the sets-and-fractions oracle
(tests/helpers/track_score_ref.py) and the host rule: exact integer equality on the whole case table.

Shapes are the smallest at which the tiling can go wrong: 16 x 64 (exactly one 64 x 16 tile), 17 x 65 (one row and one
column into the next tiles), 48 x 130 and 48 x 80 (interior, edge and partial tiles); N 1, 2, 3, 5, 6 and 9; Kt and Kp of 1, 2,
4, 7 and 128 with Kt != Kp in both orders (128: the whole LDS table, both halves of the 128-bit sets); M 1, 2, 7 and 65,536
(the last on two frames)."""
import numpy as np
import pytest
import torch

from spnet_amd import fake_espi as F
from spnet_amd import tracks as TK
from tests.helpers import track_score_ref as R
from tests.test_track_score_cpu import assert_equals_oracle, host

pytestmark = pytest.mark.gpu
INVALID = "hipError_t 1$"           # hipErrorInvalidValue
CASES = list(range(len(R.cases())))
IDS = [c.name for c in R.cases()]
GUARD, PATTERN, CANARY = 8, 0x5A5A5A5A, 0x7E7E7E7E


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


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


def _dev(case):
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    i = lambda a: torch.from_numpy(np.ascontiguousarray(np.clip(a, -2 ** 31, 2 ** 31 - 1), np.int32)).cuda()
    return f(case.rows_t), i(case.count_t), i(case.ident), f(case.rows_p), i(case.count_p), i(case.track)


def _raw(case, frames_per_chunk=None):
    """Both entry points as score_tracks_device calls them, into guarded, pre-filled arrays.  Checks the canaries (the
    workspaces' too) and that every output element was written."""
    from spnet_amd import _lib as L
    rt, ct, idt, rp, cp, tr = _dev(case)
    N, Kt, Kp, M = case.rows_t.shape[0], case.rows_t.shape[1], case.rows_p.shape[1], case.M
    st = L.current_stream()
    match, counts, stats = Guarded(N * Kt), Guarded(N * 3), Guarded((M + 1) * 5)
    per = frames_per_chunk or max(N, 1)
    for n0 in range(0, N, per):
        n = min(per, N - n0)
        nbytes = L.spnet_track_match_ws(n, Kt, Kp)
        assert nbytes == 4 * n * (Kt * Kp + Kt + Kp)
        ws = Guarded(nbytes // 4)
        L.spnet_track_match(rt[n0:].data_ptr(), ct[n0:].data_ptr(), idt[n0:].data_ptr(), Kt, rp[n0:].data_ptr(), cp[n0:].data_ptr(),
                            tr[n0:].data_ptr(), Kp, n, case.H, case.W, case.iou_q, M, ws.ptr, match.ptr + 4 * n0 * Kt,
                            counts.ptr + 12 * n0, st)
        ws.host((-1,))
    nbytes = L.spnet_track_ident_ws(N, Kt, M)
    assert nbytes == 4 * (N * Kt + 2 * (M + 1))
    ws = Guarded(nbytes // 4)
    L.spnet_track_ident(rt.data_ptr(), ct.data_ptr(), idt.data_ptr(), match.ptr, tr.data_ptr(), N, Kt, Kp, M, ws.ptr, stats.ptr, st)
    ws.host((-1,))
    out = match.host((N, Kt)), counts.host((N, 3)), stats.host((M + 1, 5))
    assert all((a != PATTERN).all() for a in out), "an output has unwritten elements"
    return out


@pytest.mark.parametrize("index", CASES, ids=IDS)
def test_g1_entry_points_equal_the_oracle(index):
    _need_gpu()
    case = R.cases()[index]
    assert_equals_oracle(_raw(case), R.oracle(index), case)


@pytest.mark.parametrize("index", CASES, ids=IDS)
def test_g2_score_tracks_device_equals_the_oracle_and_the_host(index):
    _need_gpu()
    case = R.cases()[index]
    got = TK.score_tracks_device(*_dev(case), case.H, case.W, iou=case.iou_q / 1024.0, M=case.M)
    assert all(t.is_cuda and t.dtype == torch.int32 for t in got)
    got = [t.cpu().numpy() for t in got]
    assert_equals_oracle(got, R.oracle(index), case)
    assert all(np.array_equal(g, h) for g, h in zip(got, host(case)))
    a = TK.track_score(*got, case.rows_t, case.rows_p, ident=case.ident)
    b = TK.track_score(*host(case), case.rows_t, case.rows_p, ident=case.ident)
    assert a == b and repr(a) == repr(b)


@pytest.mark.parametrize("name", ["seeded, Kt 7, Kp 128", "an identity switch", "count above K and below 0",
                                  "seeded, Kt 128, Kp 7, M 65536"])
def test_g3_one_frame_a_chunk_and_a_second_run_give_the_same_tensors(name):
    _need_gpu()
    case = R.case_named(name)
    args = _dev(case)
    kw = dict(H=case.H, W=case.W, iou=case.iou_q / 1024.0, M=case.M)
    whole = TK.score_tracks_device(*args, **kw)
    again = TK.score_tracks_device(*args, **kw)
    single = TK.score_tracks_device(*args, ws_bytes=1, **kw)
    for a, b, c in zip(whole, again, single):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert_equals_oracle(_raw(case, frames_per_chunk=1), R.oracle(IDS.index(name)), case)
    if case.rows_t.shape[0] > 2:
        assert_equals_oracle(_raw(case, frames_per_chunk=2), R.oracle(IDS.index(name)), case)


def test_g4_no_frames_and_default_arguments():
    _need_gpu()
    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    rt, rp = (torch.zeros((0, K, 6), dtype=torch.float64, device="cuda") for K in (3, 5))
    m, fc, st = TK.score_tracks_device(rt, z(0), z(0, 3), rp, None, z(0, 5), 8, 8, M=4)
    assert tuple(m.shape) == (0, 3) and tuple(fc.shape) == (0, 3)
    assert st.cpu().numpy().tolist() == [[0] * 5] + [[0, 0, 0, 0, -1]] * 4
    case = R.case_named("an identity switch")
    rt, ct, idt, rp, cp, tr = _dev(case)
    # the raw entry points with N == 0 (valid pointers, canaries around every output): success, nothing written
    from spnet_amd import _lib as L
    out = {k: Guarded(64) for k in ("ws", "match", "counts", "stats")}
    L.spnet_track_match(rt.data_ptr(), ct.data_ptr(), idt.data_ptr(), 4, rp.data_ptr(), cp.data_ptr(), tr.data_ptr(), 4, 0,
                        case.H, case.W, 256, 2, out["ws"].ptr, out["match"].ptr, out["counts"].ptr, L.current_stream())
    torch.cuda.synchronize()
    assert all((out[k].host((-1,)) == PATTERN).all() for k in ("ws", "match", "counts"))
    L.spnet_track_ident(rt.data_ptr(), ct.data_ptr(), idt.data_ptr(), out["match"].ptr, tr.data_ptr(), 0, 4, 4, 2, out["ws"].ptr,
                        out["stats"].ptr, L.current_stream())
    assert out["stats"].host((-1,))[:15].tolist() == [0] * 5 + [0, 0, 0, 0, -1] * 2
    assert (out["stats"].host((-1,))[15:] == PATTERN).all() and (out["match"].host((-1,)) == PATTERN).all()
    got = TK.score_tracks_device(rt, ct, idt, rp, None, tr, case.H, case.W)       # M: the largest ident; count_p: every row
    want = TK.score_tracks_host(case.rows_t, case.count_t, case.ident, case.rows_p, np.full(5, 4), case.track, case.H, case.W)
    assert all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(got, want)) and got[2].shape[0] == 3
    with pytest.raises(TypeError):
        TK.score_tracks_device(rt.float(), ct, idt, rp, cp, tr, case.H, case.W)
    with pytest.raises(ValueError):
        TK.score_tracks_device(rt, ct, idt, rp, cp, tr, case.H, case.W, M=65537)


def test_g5_invalid_arguments_write_nothing():
    _need_gpu()
    from spnet_amd import _lib as L
    case = R.case_named("Kt 2, Kp 7")
    rt_, ct_, id_, rp_, cp_, tr_ = _dev(case)
    rt, ct, idt, rp, cp, tr = (a.data_ptr() for a in (rt_, ct_, id_, rp_, cp_, tr_))
    N, Kt, Kp, H, W, q, M = 2, 2, 7, case.H, case.W, 256, 7
    out = {k: Guarded(4096) for k in ("ws", "match", "counts", "stats")}
    ws, m, fc, s = (out[k].ptr for k in ("ws", "match", "counts", "stats"))
    st = L.current_stream()
    good = [rt, ct, idt, Kt, rp, cp, tr, Kp, N, H, W, q, M, ws, m, fc]
    bad_match = []
    for pos in (0, 1, 2, 4, 5, 6, 13, 14, 15):                   # every pointer: NULL, then misaligned
        bad_match.append(good[:pos] + [None] + good[pos + 1:])
        bad_match.append(good[:pos] + [good[pos] + (4 if pos in (0, 4) else 2)] + good[pos + 1:])
    for pos, values in ((3, (0, 129)), (7, (0, 129)), (8, (-1,)), (9, (0, 16385)), (10, (0, 16385)), (11, (0, 1025)),
                        (12, (0, -1, 65537))):
        bad_match += [good[:pos] + [v] + good[pos + 1:] for v in values]
    bad_match.append([rt, ct, idt, 128, rp, cp, tr, 128, 1 << 17, H, W, q, M, ws, m, fc])           # N * Kt * Kp > 2^31 - 2
    bad_match.append([rt, ct, idt, 128, rp, cp, tr, 1, 1 << 24, H, W, q, M, ws, m, fc])             # N * Kt > 2^31 - 2
    good = [rt, ct, idt, m, tr, N, Kt, Kp, M, ws, s]
    bad_ident = []
    for pos in (0, 1, 2, 3, 4, 9, 10):
        bad_ident.append(good[:pos] + [None] + good[pos + 1:])
        bad_ident.append(good[:pos] + [good[pos] + (4 if pos == 0 else 2)] + good[pos + 1:])
    for pos, values in ((5, (-1, 1 << 30)), (6, (0, 129)), (7, (0, 129)), (8, (0, 65537))):
        bad_ident += [good[:pos] + [v] + good[pos + 1:] for v in values]
    for fn, table in ((L.spnet_track_match, bad_match), (L.spnet_track_ident, bad_ident)):
        for args in table:
            with pytest.raises(L.HipError, match=INVALID):
                fn(*args, st)
    assert L.spnet_track_match_ws(1 << 17, 128, 128) == -1 and L.spnet_track_match_ws(2, 0, 4) == -1
    assert L.spnet_track_match_ws(0, 4, 4) == 4 and L.spnet_track_ident_ws(2, 4, 65537) == -1
    assert L.spnet_track_ident_ws(0, 4, 1) == 16
    torch.cuda.synchronize()
    for g in out.values():
        assert (g.host((-1,)) == PATTERN).all()
    assert_equals_oracle(_raw(case), R.oracle(IDS.index(case.name)), case)      # the same arguments, valid


def test_g6_strike_movie_linked_and_scored_equals_the_host_path():
    """The real path end to end: generate_strike_device -> link_tracks_device on the truth rows -> score_tracks_device,
    against link_tracks_host -> score_tracks_host on the rows read back: every array and the dictionary, bit for bit."""
    _need_gpu()
    X, (rows, count), ident = F.generate_strike_device(2, 8, seed=4, jitter=2, size=(96, 128))
    assert tuple(X.shape) == (16, 96, 128, 1) and tuple(rows.shape) == (16, 7, 6) and tuple(ident.shape) == (16, 7)
    track = TK.link_tracks_device(rows, count, F.IM_H, F.IM_W, iou=0.25, max_gap=1)[0]
    got = TK.score_tracks_device(rows, count, ident, rows, count, track, F.IM_H, F.IM_W, iou=0.25)
    r, c, i = rows.cpu().numpy(), count.cpu().numpy(), ident.cpu().numpy()
    track_h = TK.link_tracks_host(r, c, F.IM_H, F.IM_W, iou=0.25, max_gap=1)[0]
    want = TK.score_tracks_host(r, c, i, r, c, track_h, F.IM_H, F.IM_W, iou=0.25)
    assert np.array_equal(track.cpu().numpy(), track_h)
    assert all(np.array_equal(g.cpu().numpy(), h) for g, h in zip(got, want))
    a, b = TK.track_score(*got, rows, rows, ident=ident), TK.track_score(*want, r, r, ident=i)
    assert a == b and a["gt"] == int((i > 0).sum()) > 8 and a["fp"] == 0 and a["ring_mae"] == 0
