"""spnet_amd/tracks.py without a GPU: link_tracks_host against the Python-integer oracle (tests/helpers/tracks_ref.py) on the
whole case table, the tie of the rule to the mask rule (areas and overlaps are counts on ring_masks_host's single-row masks),
what the named cases are there to show, the tables and their CSV files on a hand-written example, chunking, the stand-alone
program tools/tracks_host_check.cpp (csrc/tracks_core.h with the lanes in a loop, under AddressSanitizer and UBSan), and the
function predict_network calls for --tracks.  Every comparison is an equality of integers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from spnet_amd import masks as MK
from spnet_amd import tracks as TK
from tests.helpers import mask_ref as MR
from tests.helpers import tracks_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(range(len(R.cases())))
IDS = [c.name for c in R.cases()]


def _idx(name):
    return IDS.index(name)


def assert_equals_oracle(got, want, case, inters=None):
    track, age, nxt, prv, area = (np.asarray(a) for a in got)
    for name, g, w in (("area", area, want.area), ("next", nxt, want.next), ("prev", prv, want.prev),
                       ("track", track, want.track), ("age", age, want.age)):
        assert g.dtype == np.int32 and np.array_equal(g, w), (case.name, name)
    if inters is not None:
        assert sorted(inters) == list(range(1, case.G + 1))
        for d in inters:
            assert np.array_equal(np.asarray(inters[d]), want.inter[d]), (case.name, "inter", d)


def test_case_angles_are_trig_safe():
    for c in R.cases():
        MR.assert_trig_safe(c.rows[..., 4])


@pytest.mark.parametrize("index", CASES, ids=IDS)
def test_host_equals_oracle(index):
    c = R.cases()[index]
    got = TK.link_tracks_host(c.rows, c.count, c.H, c.W, iou=c.iou_q / 1024.0, max_gap=c.G, return_inter=True)
    assert_equals_oracle(got[:5], R.oracle(index), c, got[5])


def test_what_the_cases_show():
    o = lambda name: R.oracle(_idx(name))
    K = 4
    ident = o("identical frames")
    assert np.array_equal(ident.next[:2, :3], np.arange(K, 3 * K).reshape(2, K)[:, :3]) and (ident.age[2, :3] == 2).all()
    one = o("one frame")
    assert one.track[0].tolist() == [1, 2, 0, 0] and (one.next == -1).all()
    drift = o("drift across the threshold")
    assert (drift.inter[1][:, 0, 0] > 0).all() and drift.inter[1][3:, 0, 0].tolist() == [162] * 5 and drift.area[3:, 0].tolist() == [304] * 6
    assert drift.next[:, 0].tolist() == [-1, 2 * K, 3 * K, -1, -1, -1, -1, -1, -1]            # the track ends at frame 3
    assert drift.track[:, 0].tolist() == [1, K + 1, K + 1, K + 1] + [t * K + 1 for t in range(4, 9)]   # and new ones start
    cross = o("two that cross")
    assert (cross.next[:8, :2] >= 0).all() and cross.track[8, 0] > 0
    assert o("flicker, gap 1").track[:, 0].tolist() == [1, 1, 0, 3 * K + 1, 3 * K + 1]
    assert o("flicker, gap 2").track[:, 0].tolist() == [1, 1, 0, 1, 1] and o("flicker, gap 2").age[:, 0].tolist() == [0, 1, 0, 2, 3]
    free = o("flicker beside a free detection")
    assert free.track[:, 0].tolist() == [1, 1, 2 * K + 1, 1, 1] and free.next[2, 0] == 4 * K + 1
    tie = o("exact tie")
    assert tie.inter[1][0, 0, 0] == tie.inter[1][0, 0, 1] > 0 and tie.area[1, 0] == tie.area[1, 1]
    assert tie.next[0, 0] == K and tie.prev[1, 1] == -1                                       # forward: the lower j
    assert tie.inter[1][1, 0, 0] == tie.inter[1][1, 1, 0] and tie.prev[2, 0] == K and tie.next[1, 1] == -1    # backward: the lower i
    nm = o("non-mutual best")
    assert 0 < nm.inter[1][0, 0, 0] < nm.inter[1][0, 1, 0] and nm.next[0].tolist()[:2] == [-1, K] and nm.prev[1, 0] == 1
    at, below = o("exactly at the threshold"), o("one count below the threshold")
    c = R.case_named("exactly at the threshold")
    assert 1024 * at.inter[1][0, 0, 0] == c.iou_q * (at.area[0, 0] + at.area[1, 0] - at.inter[1][0, 0, 0])
    assert at.next[0, 0] == K and below.next[0, 0] == -1
    dead = o("dead rows")
    assert dead.live.tolist() == [[True, False, False, False], [True, False, False, False], [False] * 4, [True, True, False, False],
                                  [True, True, False, False]]
    assert dead.track[3].tolist() == [1, 3 * K + 2, 0, 0] and dead.age[4].tolist() == [3, 1, 0, 0]
    out = o("wholly outside the frame")
    assert out.live[:, :2].all() and (out.area == 0).all() and (out.next == -1).all() and out.track[2, 1] == 2 * K + 2
    assert (o("clipped by each edge").age[2] == 2).all()
    assert o("covers the whole frame").area.tolist() == [[17 * 70, 0, 0, 0]] * 2 and o("covers the whole frame").next[0, 0] == K
    pile = o("128 rows piled on one tile")
    assert pile.live.all() and (pile.inter[1] > 0).mean() > 0.9 and pile.inter[1].max() <= 1024
    for name, N in (("one chain through 40 frames", 40), ("one chain through 33 frames", 33)):
        chain = o(name)
        assert chain.age.max() == N - 1 and np.count_nonzero(chain.track == chain.track.max()) >= 1
        assert sorted(chain.age[chain.track == chain.track[N - 1].max()].tolist()) == list(range(N))
    assert o("seeded flicker, gap 4").age.max() >= 4 and len(np.unique(o("72 rows a frame, gap 3").track)) > 40


@pytest.mark.parametrize("name", ["clipped by each edge", "seeded flicker, gap 4", "dead rows"])
def test_areas_and_overlaps_are_counts_on_the_single_row_masks(name):
    c = R.case_named(name)
    N, K = c.rows.shape[:2]
    _, _, _, _, area, inters = TK.link_tracks_host(c.rows, c.count, c.H, c.W, iou=c.iou_q / 1024.0, max_gap=c.G, return_inter=True)
    alone = np.zeros((N, K, c.H, c.W), bool)
    for t in range(N):
        for k in range(min(max(int(c.count[t]), 0), K)):
            row = c.rows[t, k].copy()
            row[5] = 1.0                                       # value >= 1: rings takes no part in the pixel set
            if np.isfinite(c.rows[t, k, 5]):
                alone[t, k] = MK.ring_masks_host(row[None, None], np.ones(1, np.int64), c.H, c.W)[0] > 0
    assert np.array_equal(area, alone.sum((2, 3)))
    for d, inter in inters.items():
        want = (alone[:N - d, :, None] & alone[d:, None, :]).sum((3, 4))
        assert np.array_equal(inter, want), d


@pytest.mark.parametrize("name", ["seeded flicker, gap 4", "72 rows a frame, gap 3", "one chain through 33 frames"])
def test_chunked_equals_unchunked_on_the_host(name):
    c = R.case_named(name)
    kw = dict(H=c.H, W=c.W, iou=c.iou_q / 1024.0, max_gap=c.G, return_inter=True)
    whole = TK.link_tracks_host(c.rows, c.count, **kw)
    assert len(TK.pair_chunks(c.rows.shape[0], c.K, 1, 256 << 20)) == 1
    for ws in (1, 3 * 4 * c.K * c.K):                           # one pair a chunk, three pairs a chunk
        assert len(TK.pair_chunks(c.rows.shape[0], c.K, 1, ws)) > 1 or c.rows.shape[0] <= 3
        part = TK.link_tracks_host(c.rows, c.count, ws_bytes=ws, **kw)
        for a, b in zip(whole[:5], part[:5]):
            assert np.array_equal(a, b)
        assert all(np.array_equal(whole[5][d], part[5][d]) for d in whole[5])
    assert TK.pair_chunks(10, 4, 2, 3 * 64) == [(0, 3), (3, 3), (6, 2)] and TK.pair_chunks(1, 4, 1, 64) == []


def test_iou_is_converted_once():
    assert [TK.iou_to_q(v) for v in (0.25, 0.0, -1.0, 1.0, 7.0, 0.3, 1e-9)] == [256, 1, 1, 1024, 1024, 307, 1]
    with pytest.raises(ValueError):
        TK.iou_to_q(float("nan"))
    rows = np.zeros((2, 4, 6))
    for bad in (dict(max_gap=0), dict(max_gap=9), dict(H=0), dict(W=16385)):
        with pytest.raises(ValueError):
            TK.link_tracks_host(rows, None, **dict(dict(H=8, W=8), **bad))
    empty = TK.link_tracks_host(np.zeros((0, 4, 6)), None, 8, 8)
    assert all(a.shape == (0, 4) and a.dtype == np.int32 for a in empty)


def _example():
    """3 frames, K = 3: A runs through all three (rings 1, 5, 5), B through frames 0 and 1, C is alone in frame 2."""
    rows = np.zeros((3, 3, 6))
    rows[0, 0], rows[0, 2] = (10, 11, 4, 3, 0, 1.0), (30, 31, 5, 4, 90, 2.5)
    rows[1, 1], rows[1, 0] = (11, 12, 4, 3, 1, 5.0), (31, 32, 5, 4, 91, 2.0)
    rows[2, 2], rows[2, 0] = (12, 13, 4, 3, 2, 5.0), (50, 50, 2, 2, 0, 9.0)
    track = np.array([[1, 0, 3], [3, 1, 0], [7, 0, 1]], np.int32)
    age = np.array([[0, 0, 0], [1, 1, 0], [0, 0, 2]], np.int32)
    return rows, track, age


def test_tables_on_a_hand_written_example(tmp_path):
    rows, track, age = _example()
    names = ["f0.png", "f1.png", "f2.png"]
    table = TK.track_table(rows, track, age, names)
    assert table == [(0, "f0.png", 1, 0, 10.0, 11.0, 4.0, 3.0, 0.0, 1.0), (1, "f1.png", 1, 1, 11.0, 12.0, 4.0, 3.0, 1.0, 5.0),
                     (2, "f2.png", 1, 2, 12.0, 13.0, 4.0, 3.0, 2.0, 5.0), (0, "f0.png", 3, 0, 30.0, 31.0, 5.0, 4.0, 90.0, 2.5),
                     (1, "f1.png", 3, 1, 31.0, 32.0, 5.0, 4.0, 91.0, 2.0), (2, "f2.png", 7, 0, 50.0, 50.0, 2.0, 2.0, 0.0, 9.0)]
    summary = TK.track_summary(rows, track, age)
    assert summary == [(1, 0, 2, 3, 11.0 / 3.0, 5.0, 1), (3, 0, 1, 2, 2.25, 2.5, 0), (7, 2, 2, 1, 9.0, 9.0, 2)]
    assert [r[2] for r in TK.track_table(rows, track, age, min_len=2)] == [1, 1, 1, 3, 3]
    assert [r[0] for r in TK.track_summary(rows, track, age, min_len=3)] == [1]
    assert TK.track_table(rows, track, age, min_len=4) == [] and TK.track_summary(rows, track, age, min_len=4) == []
    assert TK.track_table(rows, track, age)[0][1] == ""
    with pytest.raises(ValueError):
        TK.track_table(rows, track, age, names[:2])
    with pytest.raises(ValueError):
        TK.track_table(rows, track, age, min_len=0)

    path = str(tmp_path / "tracks.csv")
    assert TK.write_tracks(path, rows, track, age, names, min_len=2) == (table[:5], summary[:2])
    lines = open(path).read().splitlines()
    assert lines[0] == "frame,name,track,age,cx,cy,a,b,angle,rings" and len(lines) == 6
    assert lines[2] == "1,f1.png,1,1,11.0,12.0,4.0,3.0,1.0,5.0"
    slines = open(str(tmp_path / "tracks_summary.csv")).read().splitlines()
    assert slines[0] == "track,first_frame,last_frame,n,mean_rings,max_rings,frame_of_max" and len(slines) == 3
    assert slines[1].split(",")[:4] == ["1", "0", "2", "3"] and float(slines[1].split(",")[4]) == 11.0 / 3.0
    assert slines[1].split(",")[5:] == ["5.0", "1"]
    assert TK.summary_path("a/b.c/tracks") == "a/b.c/tracks_summary"


def _grids(N, seed):
    """Hand-built de-normalised grids [N, 576]: four predictors hold drifting ellipses, one of them flickers through noobj."""
    Y = np.zeros((N, 72, 8), np.float32)
    Y[..., 6] = 1.0                                                            # noobj: dead
    for t in range(N):
        Y[t, 3] = (100 + 4 * t, 120, 30, 20, 1.0, 0.0, 0.0, 3.0 + t)
        Y[t, 17] = (300, 200 - 3 * t, 24, 24, 0.0, 1.0, 0.25, 5.0)
        Y[t, 40] = (400 - 5 * t, 300, 40, 16, -1.0, 0.0, 0.75 if t == 2 else 0.0, 7.0)
        Y[t, 71] = (250, 60, 12, 10, 0.0, -1.0, 0.49, 1.0 + seed)
    return Y.reshape(N, 576)


def test_tracks_from_predictions_on_the_host():
    Y = _grids(5, 0)
    rows, track, age, nxt, prv, area = TK.tracks_from_predictions(Y, 384, 512, max_gap=2, host=True)
    assert rows.shape == (5, 72, 6) and np.array_equal(rows, MK.prediction_rows(Y))
    assert np.count_nonzero(track[0]) == 4 and np.count_nonzero(track[2]) == 3
    assert track[:, 3].tolist() == [4] * 5 and age[:, 40].tolist() == [0, 1, 0, 2, 3] and track[4, 40] == 41
    summary = TK.track_summary(rows, track, age, min_len=3)
    assert [s[:4] for s in summary] == [(4, 0, 4, 5), (18, 0, 4, 5), (41, 0, 4, 4), (72, 0, 4, 5)]
    assert summary[0][5:] == (7.0, 4)


def test_sanitizer_host_check(tmp_path):
    """tools/tracks_host_check.cpp with -fsanitize=address,undefined, as a program of its own (no preloading)."""
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "tracks_host_check")
    cmd = [clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "spnet_amd", "csrc"), os.path.join(ROOT, "tools", "tracks_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in r.stderr and "cannot find" in r.stderr:
        pytest.skip("the compiler has no sanitizer runtime here")
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "all equal" and len(lines) > 80 and all(l.endswith("equal 1") for l in lines[:-1])
