"""gen_fake_espi.py --strike and predict_spnet.py --track_truth from the command line's side: the files a strike movie
consists of, their content against generate_strike_device, and the argument errors."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from spnet_amd import fake_espi as F
from spnet_amd import tracks as TK

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_k1_strike_movie_files(tmp_path):
    _need_gpu()
    import gen_fake_espi
    out = str(tmp_path / "set")
    gen_fake_espi.main(["-d", out, "--strike", "1", "--strike_frames", "4", "--strike_jitter", "2", "--seed", "5", "--movie"])
    root = os.path.join(out, "strike_0000")
    stems = ["steelpan_%07d" % t for t in range(4)]
    assert sorted(os.listdir(root)) == sorted([s + e for s in stems for e in (".png", ".csv")] + ["truth_tracks.csv"])
    assert sorted(os.listdir(out)) == ["strike_0000", "strike_0000.avi"]
    _, (rows, count), ident, U = F.generate_strike_device(1, 4, 5, 2, want_u8=True)
    U, rows, count, ident = (a.cpu().numpy() for a in (U, rows, count, ident))
    for t, s in enumerate(stems):
        assert np.array_equal(np.asarray(Image.open(os.path.join(root, s + ".png"))), U[t])
        got = [tuple(float(v) for v in l.split(",")) for l in open(os.path.join(root, s + ".csv")).read().splitlines()]
        assert got == ([tuple(r) for r in rows[t, :count[t]].tolist()] if count[t] else [(0.0,) * 6])
    truth = TK.read_truth_tracks(os.path.join(root, "truth_tracks.csv"))
    assert truth == TK.truth_table(rows, ident, [s + ".png" for s in stems]) and len(truth) == int((ident > 0).sum()) > 0
    r2, c2, i2 = TK.truth_arrays(truth, names=[s + ".png" for s in stems])
    K = r2.shape[1]
    assert np.array_equal(c2, count) and np.array_equal(i2, ident[:, :K]) and np.array_equal(r2, rows[:, :K])
    from spnet_amd.jpeg import MjpegReader
    assert len(MjpegReader(os.path.join(out, "strike_0000.avi"))) == 4
    # the device PNG encoder writes the same pixels
    out2 = str(tmp_path / "set2")
    gen_fake_espi.main(["-d", out2, "--strike", "1", "--strike_frames", "4", "--strike_jitter", "2", "--seed", "5", "--device_png"])
    for s in stems:
        a, b = (np.asarray(Image.open(os.path.join(o, "strike_0000", s + ".png"))) for o in (out, out2))
        assert np.array_equal(a, b)


RANGES = "--strike is at least 0, --strike_frames 1 .. 4096 and --strike_jitter 0 .. 8"


@pytest.mark.parametrize("argv,message", [(["--strike", "1", "--strike_frames", "0"], RANGES),
                                          (["--strike", "1", "--strike_frames", "4097"], RANGES),
                                          (["--strike", "1", "--strike_jitter", "9"], RANGES), (["--strike", "-1"], RANGES),
                                          (["--strike", "1", "--masks"], "--strike combines with --seed, --count_range"),
                                          (["--movie"], "--movie goes with --strike")])
def test_k2_gen_fake_espi_argument_errors(argv, message, tmp_path, capsys):
    """The message is the flag's own p.error text: an unknown flag would exit with 2 as well, with another message."""
    import gen_fake_espi
    with pytest.raises(SystemExit) as e:
        gen_fake_espi.main(["-d", str(tmp_path)] + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and os.listdir(tmp_path) == []
    assert "error: " + message in err and "unrecognized arguments" not in err


def test_k3_predict_spnet_track_truth_needs_tracks(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict_spnet.py"), "--track_truth", str(tmp_path / "t.csv")],
                       cwd=str(tmp_path), capture_output=True, text=True)
    assert r.returncode == 2 and os.listdir(tmp_path) == []
    assert "error: --track_truth scores the tracks of --tracks PATH.csv: give both" in r.stderr
    assert "unrecognized arguments" not in r.stderr


def test_k4_predict_network_scores_its_tracks_against_the_truth(tmp_path):
    """predict_network(tracks=, track_truth=) with a freshly initialised model on a strike movie of 6 frames at batch size 4:
    the loader keeps 4 frames, the truth of the other two is left out, and both score files are written and parse."""
    _need_gpu()
    import gen_fake_espi
    import predict_spnet
    from spnet_amd import config as cf
    from spnet_amd import models as M
    out = str(tmp_path / "set")
    gen_fake_espi.main(["-d", out, "--strike", "1", "--strike_frames", "6", "--seed", "5"])
    root = os.path.join(out, "strike_0000")
    truth = TK.read_truth_tracks(os.path.join(root, "truth_tracks.csv"))
    saved = cf.model_type
    try:
        cf.model_type = 'monolithic'
        model = M.Model((331, 331, 1), Y0size=576, seed=8)
        path = str(tmp_path / "tracks.csv")
        predict_spnet.predict_network(datapath=root, log_dir=str(tmp_path / "log") + "/", batch_size=4, model=model, tracks=path,
                                      track_min_len=1, track_truth=os.path.join(root, "truth_tracks.csv"))
    finally:
        cf.model_type = saved
    lines = open(TK.score_path(path)).read().splitlines()
    assert tuple(lines[0].split(",")) == TK.SCORE_FIELDS and len(lines) == 2
    score = dict(zip(TK.SCORE_FIELDS, lines[1].split(",")))
    kept = [r for r in truth if r[0] < 4]
    assert 0 < len(kept) < len(truth) and int(score["gt"]) == len(kept) == int(score["tp"]) + int(score["fn"])
    idents = open(str(tmp_path / "tracks_score_idents.csv")).read().splitlines()
    assert tuple(idents[0].split(",")) == TK.STAT_FIELDS
    assert {int(l.split(",")[0]) for l in idents[1:]} == {r[2] for r in kept}
