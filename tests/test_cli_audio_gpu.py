"""gen_fake_espi.py --strike --audio and the lag step of predict_spnet.py --audio from the command line's side: the three
files a strike's sound consists of, their content against fake_espi.strike_audio_host, and the onsets of truth_audio.csv
recovered from the written WAV with the truth rows linked on the GPU."""
import csv
import os

import numpy as np
import pytest
import torch

from spnet_amd import audio as AU
from spnet_amd import fake_espi as F
from spnet_amd import tracks as TK
from tests.test_audio_cpu import LAG_TOLERANCE

pytestmark = pytest.mark.gpu
T, SEED = 32, 5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def strike_dir(tmp_path_factory):
    _need_gpu()
    import gen_fake_espi
    out = str(tmp_path_factory.mktemp("audio") / "set")
    gen_fake_espi.main(["-d", out, "--strike", "1", "--strike_frames", str(T), "--audio", "--seed", str(SEED)])
    return out


def _truth_audio(path):
    with open(path, newline="") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == F.TRUTH_AUDIO_FIELDS
    return [(int(v[0]), v[1], float(v[2]), int(v[3]), int(v[4])) for v in lines[1:]]


def test_k1_strike_audio_files(strike_dir):
    root = os.path.join(strike_dir, "strike_0000")
    stems = ["steelpan_%07d" % t for t in range(T)]
    assert sorted(os.listdir(strike_dir)) == ["strike_0000", "strike_0000.wav"]
    assert sorted(os.listdir(root)) == sorted([s + e for s in stems for e in (".png", ".csv")] +
                                              ["notes.csv", "truth_audio.csv", "truth_tracks.csv"])
    _, nodes0, nnode0 = (a.cpu().numpy() for a in F.draw_params_device(1, SEED, "cuda:0", (1, 7), 0))
    want, info = F.strike_audio_host(nodes0, nnode0, T, SEED)
    pcm, rate = AU.read_wav(os.path.join(strike_dir, "strike_0000.wav"))
    assert rate == 48000 and pcm.shape == (T * 240,) and np.array_equal(pcm, want[0])
    notes = AU.read_notes(os.path.join(root, "notes.csv"))
    valid = np.flatnonzero(info["valid"][0])
    assert len(valid) >= 1
    assert notes == [(info["name"][0][j], float(info["freq"][0, j]), float(nodes0[0, j, 0]), float(nodes0[0, j, 1])) for j in valid]
    truth = _truth_audio(os.path.join(root, "truth_audio.csv"))
    assert truth == F.strike_audio_truth(info, 0, T)
    # the identities are those of truth_tracks.csv, and every video onset is onset_frame of that identity's ring curve
    curves = AU.track_curves(TK.read_truth_tracks(os.path.join(root, "truth_tracks.csv")), T)
    assert sorted(curves) == [r[0] for r in truth]
    assert all(AU.onset_frame(curves[r[0]], AU.DEFAULT_ONSET_FRAC) == r[3] for r in truth)


def test_k2_lag_step_recovers_the_written_onsets(strike_dir, tmp_path):
    """The truth rows linked on the GPU (jitter 0: every identity is one chain), the envelopes of the written WAV computed on
    the GPU, audio_lag at the defaults: per note the video onset of truth_audio.csv exactly and the audio onset within the
    tolerance tests/test_audio_cpu.py measured; the two CSV files parse."""
    root = os.path.join(strike_dir, "strike_0000")
    truth = {r[1]: r for r in _truth_audio(os.path.join(root, "truth_audio.csv"))}
    rows_t, count_t, _ = TK.truth_arrays(TK.read_truth_tracks(os.path.join(root, "truth_tracks.csv")), n_frames=T)
    track, age = TK.link_tracks_device(rows_t, count_t, F.IM_H, F.IM_W)[:2]
    path = str(tmp_path / "tracks.csv")
    table, _ = TK.write_tracks(path, rows_t, track, age, min_len=1)
    notes = AU.read_notes(os.path.join(root, "notes.csv"))
    pcm, rate = AU.read_wav(os.path.join(strike_dir, "strike_0000.wav"))
    env = AU.note_curves(pcm, rate, notes, T, 200.0)
    assert np.array_equal(env, AU.note_curves(pcm, rate, notes, T, 200.0, host=True))
    lag = AU.audio_lag(table, notes, env, 200.0)
    AU.write_lag(AU.lag_path(path), lag)
    AU.write_envelopes(AU.envelopes_path(path), env, notes)
    assert [r[0] for r in lag] == [n[0] for n in notes] and set(truth) == {n[0] for n in notes}
    for name, _, tr, v_on, a_on, lag_frames, lag_ms, peak, max_rings in lag:
        _, _, _, v_true, a_true = truth[name]
        assert tr is not None and v_on == v_true and abs(a_on - a_true) <= LAG_TOLERANCE
        assert lag_frames == a_on - v_on and lag_ms == 5.0 * lag_frames and peak > 0 and max_rings >= 1
    lines = open(AU.lag_path(path)).read().splitlines()
    assert tuple(lines[0].split(",")) == AU.LAG_FIELDS and len(lines) == 1 + len(notes)
    lines = open(AU.envelopes_path(path)).read().splitlines()
    assert lines[0].split(",") == ["frame"] + [n[0] for n in notes] and len(lines) == 1 + T
    assert [float(v) for v in lines[T].split(",")[1:]] == env[T - 1].tolist()


def test_k3_predict_network_writes_envelopes_and_lag(strike_dir, tmp_path):
    """predict_network(tracks=, audio=, notes=, audio_fps=) with a freshly initialised model on the strike movie: whatever
    it tracks, the envelopes file holds the device envelopes of the written WAV and the lag file one parsable row per note."""
    import predict_spnet
    from spnet_amd import config as cf
    from spnet_amd import models as M
    root = os.path.join(strike_dir, "strike_0000")
    wav, notes_path = os.path.join(strike_dir, "strike_0000.wav"), os.path.join(root, "notes.csv")
    saved = cf.model_type
    try:
        cf.model_type = 'monolithic'
        model = M.Model((331, 331, 1), Y0size=576, seed=8)
        path = str(tmp_path / "tracks.csv")
        predict_spnet.predict_network(datapath=root, log_dir=str(tmp_path / "log") + "/", batch_size=16, model=model, tracks=path,
                                      track_min_len=1, audio=wav, notes=notes_path, audio_fps=200.0)
    finally:
        cf.model_type = saved
    notes = AU.read_notes(notes_path)
    pcm, rate = AU.read_wav(wav)
    env = AU.note_curves(pcm, rate, notes, T, 200.0)
    lines = open(AU.envelopes_path(path)).read().splitlines()
    assert lines[0].split(",") == ["frame"] + [n[0] for n in notes] and len(lines) == 1 + T
    assert np.array_equal(np.array([[float(v) for v in l.split(",")[1:]] for l in lines[1:]]), env)
    lines = open(AU.lag_path(path)).read().splitlines()
    assert tuple(lines[0].split(",")) == AU.LAG_FIELDS and [l.split(",")[0] for l in lines[1:]] == [n[0] for n in notes]
    for l, k in zip(lines[1:], range(len(notes))):
        v = l.split(",")
        assert len(v) == len(AU.LAG_FIELDS) and int(v[4]) == AU.onset_frame(env[:, k]) and float(v[7]) == env[:, k].max()
        assert (v[2] == "") == (v[3] == "") == (v[8] == "") and (v[5] == "") == (v[6] == "")
