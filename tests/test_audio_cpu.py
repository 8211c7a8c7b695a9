"""The audio half's host side (spnet_amd/audio.py, fake_espi.strike_audio_host): the numpy twin of the note-envelope rule
against the Python-integer oracle (tests/helpers/audio_ref.py), the tables, onsets, note assignment, files, the synthetic
strike sound and the lag it was built with recovered end to end, the kernel's core under sanitizers as a program of its
own, and the parser errors of both scripts.  No GPU."""
import os
import shutil
import subprocess
import wave

import numpy as np
import pytest

from spnet_amd import audio as AU
from spnet_amd import fake_espi as F
from spnet_amd import tracks as TK

from tests.helpers import audio_ref as R
from tests.helpers import track_score_ref as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# |recovered lag - true lag| over the 16 sequences of test_e4_*, measured with the host path (window 2048 at 48 kHz and 200
# frames a second, onset at 0.1 of the maximum): errors -5 .. 0 frames (the window starts at the frame's instant and looks
# 8.5 frames ahead, so a rising note is heard early; the struck notes are exact).  DESIGN.md 5k records it; the tests allow
# one frame more.
MEASURED_WORST_LAG_ERROR = 5
LAG_TOLERANCE = MEASURED_WORST_LAG_ERROR + 1


def _pcm(S, L, seed):
    return np.random.RandomState(seed).randint(-32768, 32768, (S, L)).astype(np.int16)


def _steps(K):
    return AU.note_steps([261.63, 1000.5, 3000.0, 0.0, 23999.0][:K], 48000)


# ----------------------------------------------------------------------------- the twin against the oracle
@pytest.mark.parametrize("Wn,K,hop,offset", [(64, 1, (1, 1), 0), (64, 5, (300, 1), 0), (192, 5, (441, 10), -100),
                                             (192, 1, (441, 10), 690), (64, 5, (1, 1), 5000), (192, 5, (300, 1), -100)])
def test_a1_host_equals_the_python_integer_oracle(Wn, K, hop, offset):
    """S = 4 with len (0, 50 < Wn, L, beyond L): gaps between windows at hop 300 with Wn 64, a window that begins before the
    recording, one that runs past its end, one wholly past it."""
    L = 700
    pcm, lens, win = _pcm(4, L, Wn + K), [0, 50, L, L + 9], AU.window_table(Wn)
    got = AU.note_envelopes_host(pcm, lens, 5, hop, offset, _steps(K), win)
    want = R.note_envelopes(pcm.tolist(), lens, 5, hop, offset, _steps(K).tolist(), win.tolist(), AU.cos_table().tolist())
    assert got[0].dtype == np.int64 and got[0].shape == (4, 5, K)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not got[0][0].any() and not got[1][0].any()                     # len 0: nothing
    if offset < 5000:
        assert got[0][2].any()
    else:
        assert not got[0].any() and not got[1].any()                       # every window past the end


def test_a2_host_does_not_depend_on_the_chunk_or_the_split():
    pcm, win = _pcm(3, 900, 3), AU.window_table(64)
    whole = AU.note_envelopes_host(pcm, [900, 10, 400], 37, (441, 10), -7, _steps(5), win)
    small = AU.note_envelopes_host(pcm, [900, 10, 400], 37, (441, 10), -7, _steps(5), win, chunk=5)
    assert all(np.array_equal(a, b) for a, b in zip(whole, small))
    for s, ln in enumerate([900, 10, 400]):
        one = AU.note_envelopes_host(pcm[s:s + 1], [ln], 37, (441, 10), -7, _steps(5), win)
        assert np.array_equal(one[0][0], whole[0][s]) and np.array_equal(one[1][0], whole[1][s])
    tail = AU.note_envelopes_host(pcm, [900, 10, 400], 17, (441, 10), -7 + (20 * 441) // 10, _steps(5), win)
    assert np.array_equal(tail[0], whole[0][:, 20:]) and np.array_equal(tail[1], whole[1][:, 20:])


def test_a3_the_magnitude_bound_is_exact():
    """All samples -32768 with step 0 at Wn 8192: every term has the same sign.  With the Hann table, and with a window of
    32767 throughout -- the largest sum the limits allow, below 2^58."""
    pcm = np.full((1, 8192), -32768, np.int16)
    hann = AU.window_table(8192)
    re, im = AU.note_envelopes_host(pcm, None, 1, 1, 0, [0], hann)
    assert int(re[0, 0, 0]) == -32768 * 16384 * int(hann.astype(np.int64).sum()) and int(im[0, 0, 0]) == 0
    flat = np.full(8192, 32767, np.int16)
    re, im = AU.note_envelopes_host(pcm, None, 1, 1, 0, [0], flat)
    assert int(re[0, 0, 0]) == -32768 * 32767 * 16384 * 8192 == -144110790029344768 and int(im[0, 0, 0]) == 0
    assert abs(int(re[0, 0, 0])) < 2 ** 57
    assert AU.envelope(re, im, flat)[0, 0, 0] == 32768.0


def test_a4_limits_are_refused():
    pcm, win = _pcm(1, 100, 0), AU.window_table(64)
    ok = dict(length=None, T=2, hop=(1, 1), offset=0, steps=[1], window=win)
    AU.note_envelopes_host(pcm, **ok)
    for bad in (dict(T=0), dict(T=(1 << 20) + 1), dict(hop=(0, 1)), dict(hop=(1, 1 << 31)), dict(offset=(1 << 40) + 1),
                dict(offset=-(1 << 40) - 1), dict(steps=np.zeros(65, np.uint32)), dict(steps=np.zeros(0, np.uint32)),
                dict(window=np.zeros(63, np.int16)), dict(window=np.zeros(8193, np.int16)), dict(ctab=np.zeros(4095, np.int16))):
        with pytest.raises(ValueError):
            AU.note_envelopes_host(pcm, **dict(ok, **bad))
    with pytest.raises(ValueError):
        AU.note_envelopes_host(pcm[0], **ok)
    with pytest.raises(TypeError):
        AU.note_envelopes_host(pcm.astype(np.int32), **ok)
    with pytest.raises(ValueError):
        AU.window_table(63)
    with pytest.raises(ValueError):
        AU.note_steps([48000.0], 48000)


# ----------------------------------------------------------------------------- tables
def test_b1_tables():
    c = AU.cos_table()
    assert c.dtype == np.int16 and c.shape == (4096,) and c[0] == 16384 and c[2048] == -16384 and c[1024] == 0 == c[3072]
    assert c.min() == -16384 and c.max() == 16384
    assert np.array_equal(c[1:], c[1:][::-1])                                          # cos(x) = cos(2 pi - x)
    assert np.array_equal(c[:2048], -c[2048:])                                         # cos(x + pi) = -cos(x)
    assert np.array_equal(c[(np.arange(4096) + 3072) & 4095][1:], -c[(np.arange(4096) + 3072) & 4095][1:][::-1])   # the sine is odd
    for Wn in (64, 192, 2048, 8192):
        w = AU.window_table(Wn)
        assert w.dtype == np.int16 and w.shape == (Wn,) and w[0] == 0 and w.min() == 0 and w.max() == 32767 == w[Wn // 2]
        assert np.array_equal(w[1:], w[1:][::-1])
        want = 32767 * 0.5 * (1 - np.cos(2 * np.pi * np.arange(Wn) / Wn))
        assert np.abs(w - want).max() <= 0.5 + 1e-9
    assert AU.note_steps([0, 12000, 440], 48000).tolist() == [0, 1 << 30, round(440 / 48000 * 2 ** 32)]
    assert AU.hop_fraction(48000, 200) == (240, 1) and AU.hop_fraction(44100, 1000) == (441, 10)
    assert AU.hop_fraction(48000, 29.97) == (1600000, 999)


def test_b2_envelope_of_a_sine_is_half_its_amplitude():
    """The float step: a sine of amplitude A at a note's frequency has the envelope A / 2 (within the tables' rounding), a
    note 3 semitones off sees less than a hundredth of it through a window of 2048."""
    n = np.arange(4096)
    pcm = np.rint(8000 * np.sin(2 * np.pi * 440.0 * n / 48000 + 0.3)).astype(np.int16)[None, :]
    win = AU.window_table(2048)
    env = AU.envelope(*AU.note_envelopes_host(pcm, None, 3, 240, 0, AU.note_steps([440.0, 523.25], 48000), win), win)
    assert np.all(np.abs(env[0, :, 0] - 4000) < 8) and np.all(env[0, :, 1] < 40)


# ----------------------------------------------------------------------------- onsets and assignment
def test_c1_onset_frame_edges():
    assert AU.onset_frame([0, 0, 0], 0.1) == -1 and AU.onset_frame([], 0.1) == -1 and AU.onset_frame([0.0], 0) == -1
    assert AU.onset_frame([0, 1, 5, 10, 10, 3], 0.1) == 1 and AU.onset_frame([0, 1, 5, 10, 10, 3], 0.11) == 2
    assert AU.onset_frame([0, 1, 5, 10, 10, 3], 1) == 3                                # a plateau: its first frame
    assert AU.onset_frame([0, 1, 5, 10, 10, 3], 0) == 0                                # frac 0: the first frame
    assert AU.onset_frame([7, 7, 7], 1) == 0 and AU.onset_frame(np.array([0, 0, 2]), 0.5) == 2
    assert AU.onset_frame([0, 0.5, 1.0], 0.5) == 1                                     # >=, not >


def test_c2_assign_notes_rules_and_ties():
    notes = [("a", 440.0, 100.0, 100.0), ("b", 550.0, 180.0, 100.0), ("c", 660.0, 400.0, 300.0)]
    # track 5 sits between a and b at equal distance: the lower note index; track 9 is beyond the radius of every note
    assert AU.assign_notes([(5, 4, 140.0, 100.0), (9, 50, 300.0, 200.0)], notes, 40) == [5, None, None]
    assert AU.assign_notes([(5, 4, 140.0, 100.0)], notes, 39.9) == [None, None, None]
    # a note claimed twice keeps the longest; on equal length the lower track id, in either order of arrival
    assert AU.assign_notes([(3, 4, 101.0, 100.0), (8, 9, 110.0, 100.0), (2, 9, 90.0, 99.0)], notes, 40) == [2, None, None]
    assert AU.assign_notes([(8, 9, 110.0, 100.0), (2, 9, 90.0, 99.0), (3, 4, 101.0, 100.0)][::-1], notes, 40) == [2, None, None]
    assert AU.assign_notes([(1, 3, 400.0, 300.0), (2, 3, 181.0, 101.0)], notes, 40) == [None, 2, 1]
    assert AU.assign_notes([], notes, 40) == [None] * 3 and AU.assign_notes([(1, 3, 0.0, 0.0)], [], 40) == []


def test_c3_audio_lag_records():
    table = [(t, "", 7, t - 2, 100.0, 100.0, 9.0, 8.0, 30.0, float(r)) for t, r in zip(range(2, 8), (1, 2, 4, 4, 2, 1))]
    notes = [("a", 440.0, 101.0, 100.0), ("far", 550.0, 400.0, 300.0)]
    env = np.zeros((10, 2))
    env[5:, 0] = (1, 5, 10, 4, 1)
    rec = AU.audio_lag(table, notes, env, 200.0, 0.5, 40)
    assert rec[0] == ("a", 440.0, 7, 3, 6, 3, 15.0, 10.0, 4.0)
    assert rec[1] == ("far", 550.0, None, None, -1, None, None, 0.0, None)
    assert AU.track_centres(table) == [(7, 6, 100.0, 100.0)]
    with pytest.raises(ValueError):
        AU.audio_lag(table, notes, env[:, :1], 200.0)


# ----------------------------------------------------------------------------- files
def test_d1_wav_round_trip_and_refusals(tmp_path):
    pcm = _pcm(1, 1000, 4)[0]
    path = str(tmp_path / "a.wav")
    AU.write_wav(path, pcm, 44100)
    got, rate = AU.read_wav(path)
    assert rate == 44100 and got.dtype == np.int16 and np.array_equal(got, pcm)
    stereo = str(tmp_path / "s.wav")
    with wave.open(stereo, "wb") as w:
        w.setnchannels(2), w.setsampwidth(2), w.setframerate(48000)
        w.writeframes(np.stack([pcm, -pcm // 2], 1).astype("<i2").tobytes())
    got, rate = AU.read_wav(stereo)
    assert rate == 48000 and np.array_equal(got, pcm)                                  # the first channel
    for width in (1, 3, 4):
        other = str(tmp_path / ("w%d.wav" % width))
        with wave.open(other, "wb") as w:
            w.setnchannels(1), w.setsampwidth(width), w.setframerate(48000)
            w.writeframes(bytes(width * 10))
        with pytest.raises(ValueError):
            AU.read_wav(other)
    for bad in (pcm.astype(np.int32), pcm.astype(np.float32), pcm[None, :]):
        with pytest.raises(ValueError):
            AU.write_wav(str(tmp_path / "bad.wav"), bad, 48000)


def test_d2_notes_round_trip_and_refusals(tmp_path):
    notes = [("C4", 261.6255653005986, 101.0, 55.5), ("F#4", 369.99442271163446, 0.1, 300.0), ("a, b", 1 / 3, 1.0, 2.0)]
    path = str(tmp_path / "notes.csv")
    AU.write_notes(path, notes)
    assert open(path).readline().strip() == "name,freq_hz,cx,cy" and AU.read_notes(path) == notes
    open(path, "w").write("name,freq,cx,cy\nC4,1,2,3\n")
    with pytest.raises(ValueError):
        AU.read_notes(path)
    open(path, "w").write("name,freq_hz,cx,cy\nC4,1,2\n")
    with pytest.raises(ValueError):
        AU.read_notes(path)
    lag = str(tmp_path / "t_lag.csv")
    AU.write_lag(lag, [("a", 440.0, None, None, -1, None, None, 0.0, None), ("b", 1.5, 3, 2, 6, 4, 20.0, 9.25, 4.0)])
    assert open(lag).read().splitlines() == [",".join(AU.LAG_FIELDS), "a,440.0,,,-1,,,0.0,", "b,1.5,3,2,6,4,20.0,9.25,4.0"]
    assert AU.lag_path("x/t.csv") == "x/t_lag.csv" and AU.envelopes_path("x/t.csv") == "x/t_envelopes.csv"
    AU.write_envelopes(lag, np.array([[1.0, 2.5], [0.0, 3.0]]), notes[:2])
    assert open(lag).read().splitlines() == ["frame,C4,F#4", "0,1.0,2.5", "1,0.0,3.0"]


# ----------------------------------------------------------------------------- the synthetic strike sound
S_E2E, T_E2E, LAG_E2E, SEED_E2E = 16, 128, 4, 11


@pytest.fixture(scope="module")
def strikes():
    """16 seeded sequences of 128 frames with their sound at the defaults (48 kHz, 200 frames a second, lag 4, noise 8)."""
    waves0, nodes0, nnode0 = TS.base_params(S_E2E, SEED_E2E)
    pcm, info = F.strike_audio_host(nodes0, nnode0, T_E2E, seed=SEED_E2E, lag=LAG_E2E)
    frames = F.strike_params_host(waves0, nodes0, nnode0, T_E2E, SEED_E2E)
    return (waves0, nodes0, nnode0), pcm, info, frames


def test_e1_synthesis_is_pure_and_leaves_the_frames_alone(strikes):
    base, pcm, info, frames = strikes
    waves0, nodes0, nnode0 = base
    assert pcm.dtype == np.int16 and pcm.shape == (S_E2E, T_E2E * 240)
    again, _ = F.strike_audio_host(nodes0, nnode0, T_E2E, seed=SEED_E2E, lag=LAG_E2E)
    assert np.array_equal(again, pcm)
    for lo, hi in ((0, 5), (5, 16)):                         # a sequence depends on (seed, its global index) only
        part, pinfo = F.strike_audio_host(nodes0[lo:hi], nnode0[lo:hi], T_E2E, seed=SEED_E2E, first_sequence=lo, lag=LAG_E2E)
        assert np.array_equal(part, pcm[lo:hi]) and np.array_equal(pinfo["pitch"], info["pitch"][lo:hi])
    other, _ = F.strike_audio_host(nodes0, nnode0, T_E2E, seed=SEED_E2E + 1, lag=LAG_E2E)
    assert not np.array_equal(other, pcm)
    # the frames and labels of the strike rule are what they were: the oracle of the existing rule, untouched by the addendum
    want = TS.strike(waves0, nodes0, nnode0, T_E2E, SEED_E2E, 0, 0)
    for got, ref in zip(frames, want):
        assert np.array_equal(np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1))
    # pitches: 60 + 5 j + 0 .. 2, so adjacent slots are at least 3 semitones apart; names differ within a sequence
    j = np.arange(7)[None, :]
    assert np.all((info["pitch"] - 60 - 5 * j >= 0) & (info["pitch"] - 60 - 5 * j <= 2))
    assert np.all(np.diff(info["pitch"], axis=1) >= 3) and all(len(set(nm)) == 7 for nm in info["name"])
    assert np.allclose(info["freq"], 440.0 * 2.0 ** ((info["pitch"] - 69) / 12.0), rtol=1e-15)
    assert np.array_equal(info["lag"], np.where(info["struck"] | ~info["valid"], np.where(info["struck"], 0, LAG_E2E), LAG_E2E))
    assert np.all(info["struck"].sum(1) == 1) and np.all(info["lag"][info["struck"]] == 0)


def test_e2_seven_slots_at_full_scale_do_not_clip():
    """Every slot valid with the largest ring count the rule admits (255) and the largest noise: the fixed shift keeps the
    sum inside int16 without the clip ever acting -- the bound 7 * 255 * 256 * 16384 >> 18 = 28,560 plus 1,024."""
    _, nodes0, nnode0 = TS.base_params(3, 5)
    nodes0[:, :, 7], nodes0[:, :, 5], nnode0[:] = 1, 255, 7
    nodes0[:, :, :2] = np.where(nodes0[:, :, :1] > 0, nodes0[:, :, :2], 50)
    pcm, info = F.strike_audio_host(nodes0, nnode0, 64, seed=2, lag=0, noise=1024)
    assert info["valid"].all() and (7 * 255 * 256 * 16384 >> 18) + 1024 == 29584 < 32767
    # not silent either: the struck note alone has the amplitude 255 * 256 * 16384 >> 18 = 4080 from frame 0 on
    assert 4080 - 1024 <= np.abs(pcm.astype(np.int64)).max() <= 29584
    with pytest.raises(ValueError):
        F.strike_audio_host(nodes0, nnode0, 64, noise=1025)
    with pytest.raises(ValueError):
        F.strike_audio_host(nodes0, nnode0, 64, lag=65)
    with pytest.raises(ValueError):
        F.strike_audio_host(nodes0, nnode0, 64, rate=8000)


def _sequence(strikes, s):
    """(truth table, notes, truth_audio records) of sequence s."""
    (waves0, nodes0, nnode0), pcm, info, (_, nodes, nnode, ident) = strikes
    rows, count, idn = F.strike_rows(nodes[s * T_E2E:(s + 1) * T_E2E], nnode[s * T_E2E:(s + 1) * T_E2E], ident[s * T_E2E:(s + 1) * T_E2E])
    notes = [(info["name"][s][j], float(info["freq"][s, j]), float(nodes0[s, j, 0]), float(nodes0[s, j, 1]))
             for j in np.flatnonzero(info["valid"][s])]
    return TK.truth_table(rows, idn), notes, F.strike_audio_truth(info, s, T_E2E)


def test_e3_truth_audio_follows_the_envelope_rule(strikes):
    _, _, info, _ = strikes
    n_sym = 0
    for s in range(S_E2E):
        table, notes, truth = _sequence(strikes, s)
        curves = AU.track_curves(table, T_E2E)
        assert [r[0] for r in truth] == sorted(curves) and [r[1] for r in truth] == [n[0] for n in notes]
        for ident, name, freq, v_on, a_on in truth:
            j = (ident - 1) % 7
            assert (ident - 1) // 7 == s and name == info["name"][s][j] and freq == info["freq"][s, j]
            assert v_on == AU.onset_frame(curves[ident], AU.DEFAULT_ONSET_FRAC) >= 0
            onset, rise, lag = int(info["onset"][s, j]), int(info["rise"][s, j]), int(info["lag"][s, j])
            assert onset + lag <= a_on <= onset + rise + lag and onset <= v_on <= onset + rise
            if info["struck"][s, j]:
                assert (v_on, a_on) == (0, 0)
            else:
                n_sym += 1
                # the ring count is rounded to whole rings (one ring is reached half way up the rise), the loudness is not:
                # the two onsets lie on the same rise, `lag` frames apart
                assert abs((a_on - v_on) - LAG_E2E) <= rise
    assert n_sym >= 20


def test_e4_lag_recovered_end_to_end_on_the_host(strikes):
    """audio_lag fed the TRUTH tracks and the host envelopes at the defaults: every identity present for at least 8 frames
    is assigned its own note, and the recovered lag is the true one within the measured worst case plus one frame."""
    _, pcm, info, _ = strikes
    worst, n, errs = 0, 0, []
    for s in range(S_E2E):
        table, notes, truth = _sequence(strikes, s)
        env = AU.note_curves(pcm[s], 48000, notes, T_E2E, 200, host=True)
        rec = {r[0]: r for r in AU.audio_lag(table, notes, env, 200.0)}
        present = {}
        for r in table:
            present[r[2]] = present.get(r[2], 0) + 1
        for ident, name, _, v_on, a_on in truth:
            if present[ident] < 8:
                continue
            got = rec[name]
            assert got[2] == ident, (s, got, ident)
            assert got[3] == v_on and got[6] == 1000.0 * got[5] / 200.0
            errs.append(got[5] - (a_on - v_on))
            n += 1
    print("lag error (recovered - true) in frames: min %d max %d over %d notes" % (min(errs), max(errs), n))
    assert n >= 50 and max(abs(e) for e in errs) <= LAG_TOLERANCE
    assert max(abs(e) for e in errs) >= 1                    # a tolerance of 0 would be a claim the window cannot keep


# ----------------------------------------------------------------------------- the core under sanitizers
def test_f1_core_under_sanitizers(tmp_path):
    """tools/audio_host_check.cpp with -fsanitize=address,undefined as a program of its own (no preloading): the workgroup
    of csrc/audio.hip emulated over exact-size heap blocks against a naive 128-bit loop."""
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "audio_host_check")
    r = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "spnet_amd", "csrc"), os.path.join(ROOT, "tools", "audio_host_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "all equal" and "equal 0" not in r.stdout, r.stdout + r.stderr[-3000:]
    assert r.stdout.count("equal 1") >= 11 and r.stderr == ""


# ----------------------------------------------------------------------------- parser errors
@pytest.mark.parametrize("argv,message", [(["--audio"], "--audio goes with --strike"),
                                          (["--strike", "1", "--audio", "--audio_lag", "65"], "--audio_rate is at least 16000"),
                                          (["--strike", "1", "--audio", "--audio_rate", "8000"], "--audio_rate is at least 16000"),
                                          (["--strike", "1", "--audio", "--masks"], "--strike combines with --seed, --count_range")])
def test_g1_gen_fake_espi_argument_errors(argv, message, tmp_path, capsys):
    import gen_fake_espi
    with pytest.raises(SystemExit) as e:
        gen_fake_espi.main(["-d", str(tmp_path)] + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and os.listdir(tmp_path) == []
    assert "error: " + message in err and "unrecognized arguments" not in err


ALL_THREE = "--audio compares a recording with the tracks of --tracks PATH.csv at the notes of --notes notes.csv: give all three"


@pytest.mark.parametrize("argv,message", [(["--audio", "r.wav"], ALL_THREE), (["--audio", "r.wav", "--tracks", "t.csv"], ALL_THREE),
                                          (["--audio", "r.wav", "--notes", "n.csv"], ALL_THREE),
                                          (["--audio", "r.wav", "--tracks", "t.csv", "--notes", "n.csv"],
                                           "--audio with -d needs --audio_fps"),
                                          (["--audio", "r.wav", "--tracks", "t.csv", "--notes", "n.csv", "--audio_fps", "200",
                                            "--audio_window", "63"], "--audio_window is 64 .. 8192")])
def test_g2_predict_spnet_argument_errors(argv, message, capsys):
    import predict_spnet
    with pytest.raises(SystemExit) as e:
        predict_spnet.parse_args(argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and "error: " + message in err and "unrecognized arguments" not in err


def test_g3_predict_spnet_accepts_the_audio_flags():
    import predict_spnet
    a = predict_spnet.parse_args(["--tracks", "t.csv", "--audio", "r.wav", "--notes", "n.csv", "--audio_fps", "200"])
    assert (a.audio_window, a.onset_frac, a.note_radius, a.audio_offset) == (AU.DEFAULT_WINDOW, AU.DEFAULT_ONSET_FRAC,
                                                                             AU.DEFAULT_NOTE_RADIUS, 0)
    a = predict_spnet.parse_args(["--tracks", "t.csv", "--audio", "r.wav", "--notes", "n.csv", "--movie_in", "m.avi"])
    assert a.audio_fps is None                               # the reader's own rate is taken when the movie is opened
