"""The ring-count family across the 65,535 limit of grid y / z: every entry point that splits its batch into launches of at
most 65,535 frames (or frame pairs) is run once with 65,537 of them, so that the second launch -- the one with a non-zero
base -- does work, at the smallest shapes there are: 16 x 64 (exactly one tile) for the entries that read rows, 4 x 8 and
8 pixels for those that read pixels only, K = 2, M = 3.

Frame t holds pattern t % 4.  65,535 % 4 = 3, so a second launch that started from a wrong base would write a shifted
pattern.  The expected arrays are the Python-integer oracles (tests/helpers/mask_ref.py, mask_fit_ref.py, tracks_ref.py,
track_score_ref.py) on ONE period plus its wrap-around, tiled out to the full length with numpy indexing; no host rule runs
over 65,537 frames.  The identity statistics are sums over the movie: the oracle on 2, 3 and 4 periods (+ the wrap-around
frame) shows that every period adds the same five numbers, and the 16,384 periods are that arithmetic.  Equality is exact."""
import functools

import numpy as np
import pytest
import torch

from spnet_amd import masks as MK
from tests.helpers import mask_fit_ref as FR
from tests.helpers import mask_ref as MR
from tests.helpers import track_score_ref as SR
from tests.helpers import tracks_ref as TR

pytestmark = pytest.mark.gpu
N, PERIOD, H, W, K, M, IOU_Q = 65537, 4, 16, 64, 2, 3, 256          # IOU_Q: the default IoU of 0.25
PHASE = np.arange(N) % PERIOD

# A drifts right and back, B left and back; the row order alternates, B is missing from pattern 3
A = [(16, 8, 7, 5, 30, 1.0), (19, 7, 7, 5, 30, 2.0), (22, 8, 8, 5, 30, 3.0), (19, 9, 7, 5, 30, 4.0)]
B = [(46, 8, 6, 6, 0, 5.0), (44, 9, 6, 6, 0, 6.0), (42, 8, 6, 6, 0, 7.0)]
FRAMES = [[A[0], B[0]], [B[1], A[1]], [A[2], B[2]], [A[3]]]
# the prediction: the truth one pixel to the right, rows the other way round but in pattern 2; B is missing from pattern 1 too
SHIFT = lambda r: (r[0] + 1,) + r[1:]
PRED = [[SHIFT(B[0]), SHIFT(A[0])], [SHIFT(A[1])], [SHIFT(A[2]), SHIFT(B[2])], [SHIFT(A[3])]]
IDENT = [[1, 2], [2, 1], [1, 2], [1, 0]]
TRACK = [[9, 5], [5, 0], [6, 9], [5, 0]]                            # A's track is 6 in pattern 2: a switch there and back


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def _f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def _filled(*shape):
    return torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def movie():
    """(rows [P+1,K,6], count [P+1]) of one period plus its wrap-around frame, and the device tensors of all N frames."""
    rows, count = TR.pack(FRAMES + FRAMES[:1], K)
    MR.assert_trig_safe(rows[..., 4])
    return rows, count, _f64(rows[PHASE]), _i32(count[PHASE])


@functools.lru_cache(maxsize=None)
def linked():
    rows, count = movie()[:2]
    res = TR.link(rows, count, H, W, 1, IOU_Q)
    assert (res.next[:PERIOD, 0] >= 0).all(), "consecutive patterns link at the default IoU"
    return res


@functools.lru_cache(maxsize=None)
def scored(periods):
    """(rows_t, count_t, ident, rows_p, count_p, track) of `periods` periods plus the wrap-around frame, and their score."""
    reps = lambda x: x * periods + x[:1]
    rt, ct = TR.pack(reps(FRAMES), K)
    rp, cp = TR.pack(reps(PRED), K)
    ident, track = np.asarray(reps(IDENT), np.int64), np.asarray(reps(TRACK), np.int64)
    return (rt, ct, ident, rp, cp, track), SR.score(rt, ct, ident, rp, cp, track, H, W, IOU_Q, M)


def test_ring_masks():
    _need_gpu()
    rows, count, rows_d, count_d = movie()
    want = MR.ring_masks(rows[:PERIOD], count[:PERIOD], H, W)
    assert len({m.tobytes() for m in want}) == PERIOD
    got = MK.ring_masks_device(rows_d, count_d, H, W)
    assert torch.equal(got, torch.from_numpy(want).cuda()[torch.from_numpy(PHASE).cuda()])


def test_mask_compare():
    _need_gpu()
    rng = np.random.RandomState(1)
    pred, truth = (rng.choice(np.asarray([0, 0, 20, 24, 40], np.uint8), size=(PERIOD, 8)) for _ in range(2))
    want = MR.compare_counts(pred, truth, 5)
    assert len({tuple(w) for w in want.tolist()}) == PERIOD
    got = MK.mask_counts_device(torch.from_numpy(pred[PHASE]).cuda(), torch.from_numpy(truth[PHASE]).cuda(), 5)
    assert np.array_equal(got.cpu().numpy(), want[PHASE])


def test_mask_label_and_mask_moments():
    _need_gpu()
    masks = np.zeros((PERIOD, 4, 8), np.uint8)
    masks[0, 1:3, 1:4] = 30                                         # one component
    masks[1, 0, 0:2], masks[1, 2:4, 5:8] = 10, 20                   # two
    masks[2, 0, 7], masks[2, 3, 0], masks[2, 1:3, 3:5] = 10, 20, 30   # three: one more than C
    masks[3, :, 2], masks[3, 3, 2:7] = 40, 40                       # an L
    labels, comps = FR.fill(masks, 0)
    want_n, want_sums = FR.packed(comps, 2)
    assert want_n.tolist() == [1, 2, 3, 1]
    masks_d = torch.from_numpy(masks[PHASE]).cuda()
    labels_d = MK.label_components_device(masks_d, 0)
    assert np.array_equal(labels_d.cpu().numpy(), labels[PHASE])
    n_d, sums_d = MK.component_sums_device(masks_d, 0, 2, labels=labels_d)
    assert np.array_equal(n_d.cpu().numpy(), want_n[PHASE]) and np.array_equal(sums_d.cpu().numpy(), want_sums[PHASE])


def test_track_area_overlap_and_link():
    _need_gpu()
    from spnet_amd import _lib as L
    _, _, rows_d, count_d = movie()
    want = linked()
    st = L.current_stream()
    area, inter = _filled(N, K), _filled(N - 1, K, K)
    nxt, prv = (torch.full((N, K), -1, dtype=torch.int32, device="cuda") for _ in range(2))
    L.spnet_track_area(rows_d.data_ptr(), count_d.data_ptr(), N, K, H, W, area.data_ptr(), st)
    assert len({tuple(a) for a in want.area[:PERIOD].tolist()}) == PERIOD
    assert np.array_equal(area.cpu().numpy(), want.area[PHASE])
    L.spnet_track_overlap(rows_d.data_ptr(), count_d.data_ptr(), N, K, H, W, 0, N - 1, 1, inter.data_ptr(), st)
    assert np.array_equal(inter.cpu().numpy(), want.inter[1][PHASE[:-1]])       # pair t: patterns t % 4 and (t + 1) % 4
    L.spnet_track_link(inter.data_ptr(), area.data_ptr(), rows_d.data_ptr(), count_d.data_ptr(), N, K, 0, N - 1, 1, IOU_Q,
                       nxt.data_ptr(), prv.data_ptr(), st)
    # the oracle's flat indices, relative to their own frame: next points into the frame after, prev into the one before
    t = np.arange(N)[:, None]
    j = np.where(want.next[:PERIOD] >= 0, want.next[:PERIOD] - (np.arange(PERIOD)[:, None] + 1) * K, -1)[PHASE]
    want_next = np.where((j >= 0) & (t < N - 1), (t + 1) * K + j, -1)
    i = np.where(want.prev[1:] >= 0, want.prev[1:] - np.arange(PERIOD)[:, None] * K, -1)[(PHASE - 1) % PERIOD]
    want_prev = np.where((i >= 0) & (t > 0), (t - 1) * K + i, -1)
    assert np.array_equal(nxt.cpu().numpy(), want_next) and np.array_equal(prv.cpu().numpy(), want_prev)


def test_track_match_and_track_ident():
    _need_gpu()
    from spnet_amd import _lib as L
    (rt, ct, ident, rp, cp, track), want = scored(1)
    MR.assert_trig_safe(np.concatenate([rt[..., 4], rp[..., 4]]))
    assert len({tuple(m) + tuple(c) for m, c in zip(want.match[:PERIOD].tolist(), want.frame_counts[:PERIOD].tolist())}) == PERIOD
    # every period adds the same statistics (first_matched_frame stays): shown on 2, 3 and 4 periods, then arithmetic
    s2, s3, s4 = (scored(p)[1].ident_stats for p in (2, 3, 4))
    assert np.array_equal(s4 - s3, s3 - s2) and (s3 - s2)[:, 4].tolist() == [0] * (M + 1)
    assert (s3 - s2)[1:3, :2].min() > 0 and (s3 - s2)[1, 2] > 0 and (s3 - s2)[2, 3] > 0, "A switches, B breaks in every period"
    want_stats = s2 + ((N - 1) // PERIOD - 2) * (s3 - s2)
    rt_d, ct_d, id_d, rp_d, cp_d, tr_d = _f64(rt[PHASE]), _i32(ct[PHASE]), _i32(ident[PHASE]), _f64(rp[PHASE]), _i32(cp[PHASE]), \
        _i32(track[PHASE])
    st = L.current_stream()
    ws = torch.empty((L.spnet_track_match_ws(N, K, K),), dtype=torch.uint8, device="cuda")
    match, counts, stats = _filled(N, K), _filled(N, 3), _filled(M + 1, 5)
    L.spnet_track_match(rt_d.data_ptr(), ct_d.data_ptr(), id_d.data_ptr(), K, rp_d.data_ptr(), cp_d.data_ptr(), tr_d.data_ptr(), K,
                        N, H, W, IOU_Q, M, ws.data_ptr(), match.data_ptr(), counts.data_ptr(), st)
    assert np.array_equal(match.cpu().numpy(), want.match[PHASE]) and np.array_equal(counts.cpu().numpy(), want.frame_counts[PHASE])
    ws = torch.empty((L.spnet_track_ident_ws(N, K, M),), dtype=torch.uint8, device="cuda")
    L.spnet_track_ident(rt_d.data_ptr(), ct_d.data_ptr(), id_d.data_ptr(), _i32(want.match[PHASE]).data_ptr(), tr_d.data_ptr(), N,
                        K, K, M, ws.data_ptr(), stats.data_ptr(), st)
    assert np.array_equal(stats.cpu().numpy(), want_stats)
