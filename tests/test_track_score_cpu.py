"""The tracking score's host rule (spnet_amd/tracks.py match_tracks_host, ident_stats_host) against the sets-and-fractions
oracle (tests/helpers/track_score_ref.py) on the whole case table: exact integer equality, no tolerance anywhere.  And one
property that follows from the rules alone: strike sequences without jitter, linked from their own truth rows, score
perfectly."""
import numpy as np
import pytest

from spnet_amd import fake_espi as F
from spnet_amd import tracks as TK
from tests.helpers import mask_ref as MR
from tests.helpers import track_score_ref as R

CASES = list(range(len(R.cases())))
IDS = [c.name for c in R.cases()]


def assert_equals_oracle(got, want, case):
    match, counts, stats = (np.asarray(a) for a in got)
    assert match.shape == want.match.shape and counts.shape == (len(case.rows_t), 3) and stats.shape == (case.M + 1, 5)
    assert np.array_equal(match, want.match), case.name + ": match"
    assert np.array_equal(counts, want.frame_counts), case.name + ": frame_counts"
    assert np.array_equal(stats, want.ident_stats), case.name + ": ident_stats"


def host(case):
    return TK.score_tracks_host(case.rows_t, case.count_t, case.ident, case.rows_p, case.count_p, case.track, case.H, case.W,
                                iou=case.iou_q / 1024.0, M=case.M)


def test_c0_the_table_is_what_it_says():
    for c in R.cases():
        for rows in (c.rows_t, c.rows_p):
            MR.assert_trig_safe(rows[..., 4][np.isfinite(rows[..., 4])])
        assert TK.iou_to_q(c.iou_q / 1024.0) == c.iou_q
    o = {c.name: R.oracle(i) for i, c in enumerate(R.cases())}
    assert o["exact tie, two predictions"].match.tolist() == [[0, -1, -1, -1]]              # the lower index wins
    assert o["exact tie, two truths"].match.tolist() == [[0, -1, -1, -1]]
    assert o["exactly at iou_q"].frame_counts.tolist() == [[1, 0, 0]] and o["one count below iou_q"].frame_counts.tolist() == [[0, 1, 1]]
    assert o["an identity switch"].ident_stats[1].tolist() == [5, 5, 2, 0, 0]
    assert o["a fragment without a switch"].ident_stats[1].tolist() == [6, 3, 0, 1, 1]
    assert o["a fragment with a switch"].ident_stats[1].tolist() == [4, 3, 1, 1, 0]
    assert o["a duplicate identity in a frame"].ident_stats[2].tolist() == [2, 2, 1, 0, 0]
    assert o["ident above M and below 1"].ident_stats[:, 0].tolist() == [0, 0, 2]
    assert o["seeded, Kt 7, Kp 128"].ident_stats[:, 2].sum() > 0 and o["seeded, Kt 7, Kp 128"].frame_counts.min(0).tolist() != [0, 0, 0]


@pytest.mark.parametrize("index", CASES, ids=IDS)
def test_c1_host_rule_equals_the_oracle(index):
    case = R.cases()[index]
    assert_equals_oracle(host(case), R.oracle(index), case)


def test_c2_track_score_dictionary():
    case = R.case_named("a fragment with a switch")
    m, fc, st = host(case)
    s = TK.track_score(m, fc, st, case.rows_t, case.rows_p, ident=case.ident)
    assert tuple(s) == TK.SCORE_FIELDS
    assert (s["gt"], s["tp"], s["fn"], s["fp"], s["switches"], s["fragments"]) == (4, 3, 1, 0, 1, 1)
    assert s["mota"] == 1.0 - 2.0 / 4.0 and s["precision"] == 1.0 and s["recall"] == 0.75
    assert (s["identities"], s["mostly_tracked"], s["mostly_lost"]) == (1, 0, 0)
    assert s["ring_mae"] == 0.5 and s["onset_error"] == 0.0
    case = R.case_named("a fragment without a switch")
    s = TK.track_score(*host(case), case.rows_t, case.rows_p, ident=case.ident)
    assert s["onset_error"] == 0.5 and s["mostly_tracked"] == 1 and s["ring_mae"] == 1.5 / 8
    empty = TK.track_score(np.zeros((0, 4), np.int32), np.zeros((0, 3), np.int32), np.zeros((2, 5), np.int32),
                           np.zeros((0, 4, 6)), np.zeros((0, 4, 6)))
    assert empty["gt"] == 0 and empty["mota"] is None and empty["ring_mae"] is None and empty["onset_error"] is None


def test_c3_truth_table_round_trip_and_score_files(tmp_path):
    case = R.case_named("an identity switch")
    names = ["f%d.png" % n for n in range(5)]
    table = TK.write_truth_tracks(str(tmp_path / "truth_tracks.csv"), case.rows_t, case.ident, names)
    back = TK.read_truth_tracks(str(tmp_path / "truth_tracks.csv"))
    assert back == table and len(table) == 10 and [r[3] for r in table[:5]] == [0, 1, 2, 3, 4]
    rows, count, ident = TK.truth_arrays(back, names=list(reversed(names)))
    assert count.tolist() == [2] * 5 and np.array_equal(ident, case.ident[:, :2]) and np.array_equal(rows, case.rows_t[::-1, :2])
    rows, count, ident = TK.truth_arrays(back, n_frames=6)
    assert count.tolist() == [2] * 5 + [0]
    with pytest.raises(ValueError):
        TK.truth_arrays(back, names=names[:3])
    with pytest.raises(ValueError):
        TK.read_truth_tracks(__file__)
    m, fc, st = host(case)
    s = TK.track_score(m, fc, st, case.rows_t, case.rows_p, ident=case.ident)
    path = str(tmp_path / "p_score.csv")
    TK.write_track_score(path, s, st)
    lines = open(path).read().splitlines()
    assert tuple(lines[0].split(",")) == TK.SCORE_FIELDS and lines[1].split(",")[4] == "2" and len(lines) == 2
    idents = open(str(tmp_path / "p_score_idents.csv")).read().splitlines()
    assert idents == ["ident,present,matched,switches,fragments,first_matched_frame", "1,5,5,2,0,0", "2,5,5,0,0,0"]
    assert TK.score_path("a/b.csv") == "a/b_score.csv"


def test_c7_onset_uses_the_effective_identity_and_unknown_truth_frames_can_be_left_out():
    """A dead row, a row beyond count and the higher index of a duplicate carry identity 1 in frames 0 and 1; the identity is
    present from frame 2 on and matched from frame 3: onset_error is 1, not 3."""
    E, P = (20, 20, 10, 6, 30, 2.0), (22, 21, 10, 6, 30, 2.5)
    O = (55, 30, 8, 8, 0, 3.5)
    truth = [[((R.NAN, 1, 1, 1, 0, 1), 1), (O, 2)], [(O, 2), (O, 2), (E, 1)], [(E, 1), (O, 2)], [(E, 1), (O, 2)]]
    pred = [[(O, 8)], [(O, 8)], [(O, 8)], [(P, 9), (O, 8)]]
    case = R._case("late onset", 48, 80, 256, 2, truth, pred, count_t=[None, 2, None, None])
    got = host(case)
    assert_equals_oracle(got, R.score(case.rows_t, case.count_t, case.ident, case.rows_p, case.count_p, case.track, 48, 80, 256, 2),
                         case)
    assert got[2][1].tolist() == [2, 1, 0, 0, 3] and got[2][2].tolist() == [4, 4, 0, 0, 0]
    s = TK.track_score(*got, case.rows_t, case.rows_p, ident=case.ident, count_t=case.count_t)
    assert s["onset_error"] == (1 + 0) / 2
    names = ["f%d.png" % n for n in range(4)]
    table = TK.truth_table(case.rows_t, np.where(case.ident > 0, case.ident, 0), names)
    rows, count, ident = TK.truth_arrays(table, names=names[:2], skip_unknown=True)
    assert rows.shape[0] == 2 and count.tolist() == [2, 3] and ident[1].tolist()[:3] == [1, 2, 2]
    with pytest.raises(ValueError):
        TK.truth_arrays(table, names=names[:2])


def test_c4_argument_errors():
    case = R.case_named("truth only")
    with pytest.raises(ValueError):
        TK.score_tracks_host(case.rows_t, case.count_t, case.ident, case.rows_p[:1], case.count_p[:1], case.track[:1], 48, 80)
    for M in (0, 65537):
        with pytest.raises(ValueError):
            TK.score_tracks_host(case.rows_t, case.count_t, case.ident, case.rows_p, case.count_p, case.track, 48, 80, M=M)
    with pytest.raises(ValueError):
        TK.score_tracks_host(case.rows_t, case.count_t, case.ident + 70000, case.rows_p, case.count_p, case.track, 48, 80)
    assert TK.frame_chunks(5, 2, 3, 1) == [(n, 1) for n in range(5)] and TK.frame_chunks(5, 2, 3, 48) == [(0, 2), (2, 2), (4, 1)]


@pytest.mark.parametrize("iou", [1.0 / 1024, 0.25, 1.0])
def test_c5_unjittered_strike_truth_scores_perfectly(iou):
    """Strike sequences with J = 0: an identity's pixel set is the same in every frame of its run (only the ring count
    changes, which takes no part in the pixel set), its run is contiguous, and the base ellipses of a sequence do not
    overlap (here: one a grid cell).  So the linker at gap 1 chains every identity from its first to its last frame at
    any IoU threshold up to 1, and the score of those tracks against the truth is perfect -- exactly."""
    S, T, H, W = 3, 12, 96, 128
    waves0, nodes0, nnode0 = R.base_params(S, 5, H, W)
    _, nodes, nnode, ident = F.strike_params_host(waves0, nodes0, nnode0, T, seed=9, jitter=0)
    rows, count, ident = F.strike_rows(nodes, nnode, ident)
    assert (ident > 0).sum() > 3 * T // 2 and len(np.unique(ident)) > 4
    for s in range(S):                                       # a sequence is a movie of its own
        sl = slice(s * T, (s + 1) * T)
        track = TK.link_tracks_host(rows[sl], count[sl], H, W, iou=iou, max_gap=1)[0]
        got = TK.score_tracks_host(rows[sl], count[sl], ident[sl], rows[sl], count[sl], track, H, W, iou=iou)
        sc = TK.track_score(*got, rows[sl], rows[sl], ident=ident[sl])
        assert sc["gt"] == int((ident[sl] > 0).sum()) > 0
        assert sc["mota"] == 1 and sc["switches"] == 0 and sc["fragments"] == 0 and sc["ring_mae"] == 0 and sc["onset_error"] == 0
        assert sc["fn"] == 0 and sc["fp"] == 0 and sc["mostly_tracked"] == sc["identities"]


def test_c6_host_check_program_runs_clean_under_the_sanitizers(tmp_path):
    """tools/track_score_host_check.cpp with -fsanitize=address,undefined, as a program of its own (no preloading)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"                              # is there a sanitizer runtime to link?  Asked BEFORE the tool
    probe.write_text("int main() { return 0; }\n")             # is compiled, so that an error in the tool is never a skip
    if subprocess.run([clang] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler cannot link a sanitized program here")
    exe = str(tmp_path / "track_score_host_check")
    cmd = [clang] + flags + ["-I", os.path.join(root, "spnet_amd", "csrc"),
                             os.path.join(root, "tools", "track_score_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "all equal" and len(lines) > 100 and all(l.endswith("equal 1") for l in lines[:-1])


def test_c8_a_side_without_rows():
    """K = 0 on either side is admitted by the host rule: nothing matches, every open row of the other side is a miss."""
    E = (20, 20, 10, 6, 30, 2.0)
    rows, count, ident = np.asarray([[E], [E]], np.float64), np.asarray([1, 1]), np.asarray([[1], [1]])
    none_r, none_i = np.zeros((2, 0, 6)), np.zeros((2, 0), np.int64)
    match, counts, stats = TK.score_tracks_host(rows, count, ident, none_r, np.zeros(2, np.int64), none_i, 48, 80, M=1)
    assert match.tolist() == [[-1], [-1]] and counts.tolist() == [[0, 1, 0]] * 2 and stats.tolist() == [[0] * 5, [2, 0, 0, 0, -1]]
    match, counts, stats = TK.score_tracks_host(none_r, np.zeros(2, np.int64), none_i, rows, count, ident + 4, 48, 80, M=1)
    assert match.shape == (2, 0) and counts.tolist() == [[0, 0, 1]] * 2 and stats.tolist() == [[0] * 5, [0, 0, 0, 0, -1]]
