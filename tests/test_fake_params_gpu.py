"""spnet_fake_espi_params (csrc/espi_params.hip) bit for bit against its host restatement (tests/helpers/
fake_params_ref.py), its guards, and what is built on it: fake_espi.draw_params_device / labels_from_params /
generate_device(params="device") / FakeStream, callbacks.FreshFakeESPI inside Model.fit, and gen_fake_espi.py."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import fake_params_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 384, 512
PAD = 64                        # guard elements behind every output
SEED = 0                        # at this seed the (7, 7) stream of 257 frames has late acceptances and dropped antinodes
HIP_ERROR_INVALID_VALUE = 1
_REF = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ref(cr):
    """The restated parameters of frames 0..256 at SEED, once per count range (a frame does not depend on its neighbours:
    tests/test_fake_params_cpu.py, so shorter launches are compared with a prefix)."""
    if cr not in _REF:
        _REF[cr] = R.params(0, 257, seed=SEED, count_range=cr)
    return _REF[cr]


def _launch(first, N, seed, cr, h=H, w=W, tries=True):
    """One raw launch into guarded buffers -> (status, waves, nodes, nnode, tries) as numpy, guards checked."""
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    bufs = [torch.full((N * 5 + PAD,), -7.0, dtype=torch.float32, device="cuda"),
            torch.full((N * 56 + PAD,), -7.0, dtype=torch.float32, device="cuda"),
            torch.full((N + PAD,), -7, dtype=torch.int32, device="cuda"),
            torch.full((N * 7 + PAD,), -7, dtype=torch.int32, device="cuda")]
    rc = L._lib.spnet_fake_espi_params(first, N, h, w, seed, cr[0], cr[1], F.trig2_table("cuda").data_ptr(), bufs[0].data_ptr(),
                                       bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr() if tries else None,
                                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for hb, n in zip(host, (N * 5, N * 56, N, N * 7)):
        assert (hb[n:] == -7).all(), "the kernel wrote past the end of an output"
    return rc, host[0][:N * 5].reshape(N, 5), host[1][:N * 56].reshape(N, 7, 8), host[2][:N], host[3][:N * 7].reshape(N, 7)


def test_trig2_table_is_the_helpers():
    from spnet_amd import fake_espi as F
    np.testing.assert_array_equal(F.trig2_table(), R.trig2_table())


@pytest.mark.parametrize("cr", [(1, 7), (0, 6), (7, 7)])
@pytest.mark.parametrize("N", [1, 65, 257])
def test_kernel_equals_the_restatement(N, cr):
    _need_gpu()
    ref = _ref(cr)
    if cr == (7, 7):            # the crowded stream must exercise more than one round of 64 tries, and the give-up
        assert (ref["tries"] >= 64).any() and (ref["tries"] == -1).any()
        assert (ref["tries"][:65] >= 64).any()
    rc, waves, nodes, nnode, tries = _launch(0, N, SEED, cr)
    assert rc == 0
    for name, got in (("waves", waves), ("nodes", nodes), ("nnode", nnode), ("tries", tries)):
        want = ref[name][:N]
        assert got.dtype == want.dtype
        np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32), err_msg="%s (bit patterns)" % name)


def test_first_frame_split_equals_whole():
    _need_gpu()
    whole = _launch(0, 130, 3, (1, 7))
    a, b = _launch(0, 65, 3, (1, 7)), _launch(65, 65, 3, (1, 7))
    for w, x, y in zip(whole[1:], a[1:], b[1:]):
        np.testing.assert_array_equal(w, np.concatenate([x, y]))
    # without the diagnostics array the three outputs are the same
    for w, x in zip(whole[1:4], _launch(0, 130, 3, (1, 7), tries=False)[1:4]):
        np.testing.assert_array_equal(w, x)
    # a frame index past 2^32 reaches the key (the restatement, frames 2^40 - 2 and 2^40 - 1)
    far = _launch(2 ** 40 - 2, 2, 3, (1, 7))
    want = R.params(2 ** 40 - 2, 2, seed=3)
    for name, got in zip(("waves", "nodes", "nnode", "tries"), far[1:]):
        np.testing.assert_array_equal(got, want[name])


def test_guards():
    _need_gpu()
    from spnet_amd import _lib as L
    from spnet_amd import fake_espi as F
    for kw in (dict(cr=(3, 2)), dict(cr=(1, 8)), dict(cr=(-1, 3)), dict(h=63), dict(h=2049), dict(w=63), dict(w=2049),
               dict(first=-1)):
        args = dict(first=0, N=4, seed=0, cr=(1, 7), h=H, w=W)
        args.update(kw)
        rc, waves, nodes, nnode, tries = _launch(args["first"], args["N"], args["seed"], args["cr"], args["h"], args["w"])
        assert rc == HIP_ERROR_INVALID_VALUE, kw
        assert (waves == -7).all() and (nodes == -7).all() and (nnode == -7).all() and (tries == -7).all(), kw
    # N < 0, N == 0 and the NULL pointers: raw calls on sentinel buffers
    st = torch.cuda.current_stream().cuda_stream
    t2 = F.trig2_table("cuda")
    wv, nd = torch.full((20,), -7.0, device="cuda"), torch.full((224,), -7.0, device="cuda")
    nn, tr = torch.full((4,), -7, dtype=torch.int32, device="cuda"), torch.full((28,), -7, dtype=torch.int32, device="cuda")
    ptrs = [t2.data_ptr(), wv.data_ptr(), nd.data_ptr(), nn.data_ptr()]
    fn = L._lib.spnet_fake_espi_params
    assert fn(0, -1, H, W, 0, 1, 7, *ptrs, tr.data_ptr(), st) == HIP_ERROR_INVALID_VALUE
    for k in range(4):
        p = list(ptrs)
        p[k] = None
        assert fn(0, 4, H, W, 0, 1, 7, *p, tr.data_ptr(), st) == HIP_ERROR_INVALID_VALUE, k
    assert fn(0, 0, H, W, 0, 1, 7, *ptrs, tr.data_ptr(), st) == 0          # nothing to do
    torch.cuda.synchronize()
    assert (wv == -7).all() and (nd == -7).all() and (nn == -7).all() and (tr == -7).all()
    with pytest.raises(L.HipError):                                        # the checked binding raises
        L.spnet_fake_espi_params(0, 4, H, W, 0, 3, 2, *ptrs, tr.data_ptr(), st)
    # the smallest and the largest frame the entry accepts run and stay inside their arrays
    for h, w in ((64, 64), (2048, 2048), (64, 2048)):
        rc, waves, nodes, nnode, tries = _launch(0, 5, 1, (7, 7), h, w)
        want = R.params(0, 5, seed=1, count_range=(7, 7), H=h, W=w)
        assert rc == 0
        for name, got in zip(("waves", "nodes", "nnode", "tries"), (waves, nodes, nnode, tries)):
            np.testing.assert_array_equal(got, want[name], err_msg="%s at %dx%d" % (name, h, w))


def test_generate_device_with_device_params():
    _need_gpu()
    from spnet_amd import fake_espi as F
    wv, nd, nn = F.draw_params_device(7, seed=4, count_range=(1, 7))
    labels = F.labels_from_params(nd, nn)
    want = R.params(0, 7, seed=4)
    assert labels == [[tuple(int(v) for v in want["nodes"][f, j, :6]) for j in range(want["nnode"][f])] for f in range(7)]
    assert all(type(v) is int for fr in labels for row in fr for v in row)
    X3, l3, U3 = F.generate_device(7, seed=4, noise=False, want_u8=True, chunk=3, params="device")
    X7, l7, U7 = F.generate_device(7, seed=4, noise=False, want_u8=True, chunk=7, params="device")
    assert l3 == labels and l7 == labels
    assert torch.equal(U3, U7) and torch.equal(X3, X7)
    assert len(torch.unique(U7)) == 3                                   # canvas, bands, rings: frames were drawn
    # with the sensor noise: the same frames wherever the chunk boundaries are the same; labels regardless
    Xa, la = F.generate_device(7, seed=4, chunk=7, params="device")
    Xb, lb = F.generate_device(7, seed=4, chunk=7, params="device")
    assert torch.equal(Xa, Xb) and la == labels and lb == labels
    # first_frame: frames 3..6 of the stream
    Xf, lf = F.generate_device(4, seed=4, noise=False, params="device", first_frame=3)
    assert lf == labels[3:] and torch.equal(Xf, X7[3:])
    with pytest.raises(ValueError):
        F.generate_device(2, seed=4, first_frame=3)
    with pytest.raises(ValueError):
        F.generate_device(2, seed=4, params="gpu")
    # params="host" is the call without the argument
    Xh, lh, Uh = F.generate_device(5, seed=2, want_u8=True, params="host")
    X0, l0, U0 = F.generate_device(5, seed=2, want_u8=True)
    assert lh == l0 and torch.equal(Xh, X0) and torch.equal(Uh, U0)
    assert lh == [[n[:6] for n in F.draw_params(s)[1]] for s in F.frame_seeds(5, 2)]
    # resized layout: labels unchanged, frames of the network size
    Xr, lr = F.generate_device(3, seed=4, params="device", size=331)
    assert Xr.shape == (3, 331, 331, 1) and lr == labels[:3]


TRAIN_HW = (64, 96)             # the smallest frames the suite runs the Xception engine at (tests/test_fullsize_gpu.py)


def test_fresh_fake_espi_in_fit(monkeypatch, capsys):
    _need_gpu()
    from spnet_amd import callbacks as C
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    monkeypatch.setattr(cf, "model_type", "monolithic")
    n = 4
    stream = F.FakeStream(n, seed=11, size=TRAIN_HW)
    want = [tuple(t.clone() for t in stream.epoch(e, verbose=False)) for e in (0, 1)]
    assert want[0][0].shape == (n,) + TRAIN_HW + (1,) and want[0][1].shape == (n, 576)
    assert not torch.equal(want[0][0], want[1][0]) and not torch.equal(want[0][1], want[1][1])
    # targets: the file path's codec of the epoch's labels
    _, labels = stream.frames(n, n)
    np.testing.assert_array_equal(want[1][1].cpu().numpy(), F.targets_from_labels(labels)[0])
    X, Y = np.zeros((n,) + TRAIN_HW + (1,), np.float32), np.zeros((n, 576), np.float32)
    cb = C.FreshFakeESPI(X, Y, stream)
    assert torch.equal(cb.X_dev, want[0][0]) and torch.equal(cb.Y_dev, want[0][1])
    seen = []

    class Spy(C.Callback):
        def on_batch_begin(self, batch, logs=None):
            if batch == 0:
                seen.append((cb.X_dev.clone(), cb.Y_dev.clone()))
    np.random.seed(1)
    model = M.Model(TRAIN_HW + (1,), Y0size=576, seed=5)
    hist = model.fit(X, Y, batch_size=2, epochs=2, shuffle=True, verbose=0, callbacks=[cb, Spy()])
    assert model._train_frames[1] is cb.X_dev and model._train_targets[1] is cb.Y_dev
    assert cb.epochs_filled == [0, 1] and len(seen) == 2
    for e in (0, 1):
        assert torch.equal(seen[e][0], want[e][0]) and torch.equal(seen[e][1], want[e][1])
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[0][1], seen[1][1])
    assert all(np.isfinite(v) for v in hist["loss"]) and len(hist["loss"]) == 2
    assert "third ellipse" in capsys.readouterr().out
    # with AugmentOnTheFly behind it: the augmenter reads the fresh frames and fit() reads the augmenter's output
    import random
    from spnet_amd import augmentation as A
    fresh = C.FreshFakeESPI(None, None, stream)
    aug = C.AugmentOnTheFly(fresh.X, fresh.Y, chunk=4, seed=1)
    assert aug.X_orig.data_ptr() == fresh.X_dev.data_ptr()
    ref = A.DeviceAugmenter(want[0][0].clone())              # fill range of the frames the augmenter was built on
    for cbk in (fresh, aug):
        cbk.set_model(model)
    assert model._train_frames == (id(fresh.X), aug.X_aug) and model._train_targets[1] is fresh.Y_dev
    for e in (0, 1):
        np.random.seed(20 + e)
        random.seed(20 + e)
        fresh.on_epoch_begin(e)
        aug.on_epoch_begin(e)
        ref.X.copy_(want[e][0])
        out = torch.empty_like(ref.X)
        np.random.seed(20 + e)
        random.seed(20 + e)
        ref.augment(list(range(n)), out)
        torch.cuda.synchronize()
        assert torch.equal(fresh.X_dev, want[e][0]) and torch.equal(fresh.Y_dev, want[e][1])
        assert torch.equal(aug.X_aug, out) and not torch.equal(out, want[e][0])
    fresh2 = C.FreshFakeESPI(None, None, stream)
    aug2 = C.AugmentOnTheFly(fresh2.X, fresh2.Y, chunk=4, seed=1)
    hist = model.fit(fresh2.X, fresh2.Y, batch_size=2, epochs=1, shuffle=False, verbose=0, callbacks=[fresh2, aug2])
    assert model._train_frames[1] is aug2.X_aug and np.isfinite(hist["loss"][0])


def test_gen_fake_espi_script(tmp_path, monkeypatch):
    _need_gpu()
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    from spnet_amd import utils
    from PIL import Image
    out = tmp_path / "data"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "gen_fake_espi.py"), "-n", "10", "-a", "-d", str(out)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    X, labels, U = F.generate_device(10, seed=0, want_u8=True, chunk=256, params="device")
    U = U.cpu().numpy()
    for sub, numbers in (("Train", range(0, 8)), ("Val", range(8, 10))):
        pngs, csvs = sorted(glob.glob(str(out / sub / "*.png"))), sorted(glob.glob(str(out / sub / "*.csv")))
        assert [os.path.basename(p) for p in pngs] == ["steelpan_%07d.png" % i for i in numbers]
        assert [os.path.basename(p) for p in csvs] == ["steelpan_%07d.csv" % i for i in numbers]
        for i, png, csv in zip(numbers, pngs, csvs):
            assert open(csv).read() == F.rows_to_csv(labels[i])
            np.testing.assert_array_equal(np.asarray(Image.open(png)), U[i])
    monkeypatch.setattr(cf, "model_type", "monolithic")
    Xt, Yt, files, _ = utils.build_dataset(path=str(out / "Train") + "/", shuffle=False)
    assert Xt.shape == (8, 331, 331, 1) and Yt.shape == (8, 576)
    np.testing.assert_array_equal(Yt, F.targets_from_labels(labels[:8])[0])
    Xv, Yv, _, _ = utils.build_dataset(path=str(out / "Val") + "/", shuffle=False)
    assert Xv.shape[0] == 2
    np.testing.assert_array_equal(Yv, F.targets_from_labels(labels[8:])[0])
