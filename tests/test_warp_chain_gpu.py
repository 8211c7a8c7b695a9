"""Batched warp chain on the device: spnet_warp_chain_u8 against the three separate steps (tests/helpers/warp_chain_ref.py
over oracle/warp_ref.py) and against the per-image flip_image -> rotate_image -> translate_image, bit for bit (both sides are
integer arithmetic); AugmentOnTheFly(warp=True), Model.fit on warped targets, the offline augment_preproc tool and
train_spnet.py --warp."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import warp_chain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INVALID = 1          # hipErrorInvalidValue


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _frames(h, w, n=3, seed=0):
    """uniform noise, 0/255 binary, smooth fringes: uint8 [n, h, w]"""
    rs = np.random.RandomState(seed + 31 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    base = [rs.randint(0, 256, (h, w)), rs.randint(0, 2, (h, w)) * 255,
            127.5 + 127.5 * np.sin(xx / 9.0 + yy / 23.0) * np.cos(yy / 7.0)]
    return np.stack([base[k % 3] if k < 3 else rs.randint(0, 256, (h, w)) for k in range(n)]).astype(np.uint8)


def _params(A, index, cases, h, w):
    p = A.new_warp_params(index, h, w)
    for j, c in enumerate(cases):
        A.set_warp(p, j, *c)
    return p


def _cases(h, w):
    shifts = [(0, 0), (40, 40), (-40, -40), (40, -40), (-13, 29), (w + 5, 0), (0, -(h + 1))]
    angles = [0, 20.0, -20.0, 3.25, 17.5]
    out = [(f, a, xt, yt) for f in (-2, 0, 1, -1) for a in angles for xt, yt in shifts[:3]]
    out += [(f, a, xt, yt) for f, a in ((-1, 17.5), (-2, -20.0), (0, 0)) for xt, yt in shifts[3:]]
    return out


def _run(A, X, p, want_f=True):
    wr = A.DeviceWarper(torch.from_numpy(X).cuda())
    B = len(p["index"])
    out_u8 = torch.full((B, wr.H, wr.W), 99, dtype=torch.uint8, device="cuda")
    out_f = torch.full((B, wr.H, wr.W), 7.0, dtype=torch.float32, device="cuda") if want_f else None
    wr.apply(p, out_u8=out_u8, out_f=out_f)
    torch.cuda.synchronize()
    return out_u8, out_f


@pytest.mark.parametrize("hw", [(384, 512), (331, 331), (17, 23), (40, 2048), (2048, 24)])
def test_kernel_equals_the_three_steps(hw):
    _need_gpu()
    from spnet_amd import _lib as L
    from spnet_amd import augmentation as A
    h, w = hw
    X = _frames(h, w)
    cases = _cases(h, w) if h * w < 200000 else _cases(h, w)[::3]
    if h * w < 90000:
        cases = cases + [(1, 90.0, 3, -2), (-1, 135.0, 0, 0)]          # wide source footprints: the unstaged path
    index = [j % 3 for j in range(len(cases))]
    p = _params(A, index, cases, h, w)
    out_u8, out_f = _run(A, X, p)
    got = out_u8.cpu().numpy()
    for j, c in enumerate(cases):
        np.testing.assert_array_equal(got[j], R.warp_image(X[index[j]], *c), err_msg="%s frame %d" % (c, j))
        if abs(c[2]) >= w or abs(c[3]) >= h:
            assert not got[j].any()
    np.testing.assert_array_equal(got, A.warp_chain_host(X, p))         # and the numpy restatement of the single gather
    # out_f == spnet_u8_to_input(out_u8), also when it is the only output
    n = out_u8.numel()
    src = out_u8 if n % 16 == 0 else torch.cat([out_u8.reshape(-1), torch.zeros(16 - n % 16, dtype=torch.uint8, device="cuda")])
    ref_f = torch.empty(src.numel(), dtype=torch.float32, device="cuda")
    L.spnet_u8_to_input(src.data_ptr(), ref_f.data_ptr(), src.numel(), L.current_stream())
    torch.cuda.synchronize()
    assert torch.equal(out_f.reshape(-1), ref_f[:n])
    wr = A.DeviceWarper(torch.from_numpy(X).cuda())
    only_f = torch.empty_like(out_f)
    wr.apply(p, out_f=only_f)
    torch.cuda.synchronize()
    assert torch.equal(only_f, out_f)


def test_kernel_equals_the_per_image_functions():
    _need_gpu()
    from spnet_amd import augmentation as A
    h, w = 384, 512
    X = _frames(h, w)
    cases = [(0, 17.5, 0, 0), (1, -20.0, 40, -40), (-1, 3.25, -12, 31), (-2, 20.0, 0, 0), (0, 0, 7, 7)]
    p = _params(A, [0, 1, 2, 0, 1], cases, h, w)
    got = _run(A, X, p, want_f=False)[0].cpu().numpy()
    for j, (f, a, xt, yt) in enumerate(cases):
        img = np.repeat(X[p["index"][j]][..., None], 3, axis=2)
        img, _, _ = A.flip_image(img, [], "f", f)
        img, _, _ = A.rotate_image(img, [], "f", a)
        # translate_image draws its shift: np.random.random() = (t / 40 + 1) / 2 is fed back through a patched generator
        draws = iter([(xt / 40 + 1) / 2, (yt / 40 + 1) / 2])
        keep = np.random.random
        np.random.random = lambda: next(draws)
        try:
            img, _, prefix = A.translate_image(img, [], "f", 1 if (xt, yt) != (0, 0) else 0)
        finally:
            np.random.random = keep
        if (xt, yt) != (0, 0):
            assert prefix == "f_t%d,%d" % (xt, yt)
        for ch in range(3):
            np.testing.assert_array_equal(got[j], img[..., ch], err_msg=str(cases[j]))


def test_general_matrix_with_a_wide_footprint_and_extreme_shifts():
    """A minifying matrix: a tile's source box exceeds what is staged in LDS, the taps read the frame directly."""
    _need_gpu()
    from oracle import warp_ref as WR
    from spnet_amd import augmentation as A
    h, w = 384, 512
    X = _frames(h, w)
    M = [[0.25, 0.05, 3.0], [-0.02, 0.2, 1.0]]
    p = _params(A, [0, 1, 2, 0], [(-2, 0, 0, 0)] * 4, h, w)
    p["minv"][:] = A.invert_affine_cv2(M).reshape(6)
    p["xt"][2], p["yt"][2] = 2 ** 31 - 1, 5
    p["xt"][3], p["yt"][3] = 0, -2 ** 31
    got = _run(A, X, p, want_f=False)[0].cpu().numpy()
    for j in range(2):
        np.testing.assert_array_equal(got[j], WR.warp_affine_cv2(X[j][..., None], M)[..., 0])
    assert not got[2:].any()


def test_sel_repeated_and_out_of_range_and_unaligned_views():
    _need_gpu()
    from spnet_amd import augmentation as A
    h, w = 33, 47
    X = _frames(h, w, n=4)
    cases = [(1, 11.0, 3, -4)] * 6
    index = [2, 2, -5, 9, 0, 3]
    p = _params(A, index, cases, h, w)
    # frames and output at odd byte offsets
    buf = torch.zeros(X.size + 3, dtype=torch.uint8, device="cuda")
    buf[3:] = torch.from_numpy(X).cuda().reshape(-1)
    wr = A.DeviceWarper(buf[3:].reshape(4, h, w))
    assert wr.X.data_ptr() % 4 == 3
    obuf = torch.zeros(6 * h * w + 1, dtype=torch.uint8, device="cuda")
    out = obuf[1:].reshape(6, h, w)
    wr.apply(p, out_u8=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for j, i in enumerate(index):
        np.testing.assert_array_equal(got[j], R.warp_image(X[min(max(i, 0), 3)], *cases[j]))
    assert int(obuf[0]) == 0


def test_a_frame_does_not_depend_on_its_batch():
    _need_gpu()
    from spnet_amd import augmentation as A
    h, w = 96, 128
    X = _frames(h, w, n=5)
    np.random.seed(5)
    cases = [A.draw_warp(h, w) for _ in range(300)]
    index = [j % 5 for j in range(300)]
    big = _run(A, X, _params(A, index, cases, h, w), want_f=False)[0]
    for j in (0, 137, 299):
        one = _run(A, X, _params(A, [index[j]], [cases[j]], h, w), want_f=False)[0]
        assert torch.equal(one[0], big[j])


def test_bad_arguments_are_refused_and_write_nothing():
    _need_gpu()
    from spnet_amd import _lib as L
    from spnet_amd import augmentation as A
    h, w = 20, 30
    X = torch.from_numpy(_frames(h, w)).cuda()
    p = _params(A, [0, 1], [(0, 5.0, 1, 1)] * 2, h, w)
    rec = np.zeros(2, A.WARP_RECORD)
    rec["m"], rec["flip"] = p["minv"], p["flip"]
    recd = torch.from_numpy(rec.view(np.int32).reshape(-1).copy()).cuda()
    sel = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.full((2, h, w), 99, dtype=torch.uint8, device="cuda")
    outf = torch.full((2 * h * w + 1,), 7.0, dtype=torch.float32, device="cuda")
    s = L.current_stream()
    good = (X.data_ptr(), 3, sel.data_ptr(), recd.data_ptr(), 2, h, w, out.data_ptr(), None, s)

    def bad(**kw):
        names = ("src", "n_src", "sel", "params", "N", "H", "W", "out_u8", "out_f", "stream")
        args = [kw.get(k, v) for k, v in zip(names, good)]
        with pytest.raises(L.HipError) as e:
            L.spnet_warp_chain_u8(*args)
        assert "hipError_t %d" % HIP_INVALID in str(e.value)
    bad(src=None)
    bad(params=None)
    bad(out_u8=None)                                   # no output at all
    bad(H=0)
    bad(W=2049)
    bad(H=2049)
    bad(N=-1)
    bad(n_src=0)
    bad(sel=None, N=4)                                 # no sel: N frames need N sources
    bad(params=recd.data_ptr() + 4)                    # records are 8-byte aligned
    bad(out_f=outf.data_ptr() + 2)                     # a float output is 4-byte aligned
    torch.cuda.synchronize()
    assert bool((out == 99).all()) and bool((outf == 7.0).all())
    L.spnet_warp_chain_u8(*good)                       # and the good call works
    L.spnet_warp_chain_u8(*(good[:4] + (0,) + good[5:]))       # N = 0: nothing to do
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out[1].cpu().numpy(), R.warp_image(X[0].cpu().numpy(), 0, 5.0, 0, 0))


# ----------------------------------------------------------------------------- training integration and the offline tool
@pytest.fixture(scope="module")
def espi_dir(tmp_path_factory):
    _need_gpu()
    from spnet_amd import fake_espi as F
    d = tmp_path_factory.mktemp("warp_espi")
    F.write_dataset(str(d / "Train"), 64, seed=5)
    return str(d / "Train") + "/"


def _pil_codec(u8, size):
    """The input codec (utils._load_one): RGB, Lanczos resize (None: the file's own size), channel 0, (v / 255 - 0.5) * 2."""
    from PIL import Image
    img = Image.fromarray(u8).convert("RGB")
    if size is not None:
        img = img.resize((size, size), Image.LANCZOS)
    arr = np.asarray(img, dtype=np.float32)
    return ((arr / 255.0 - 0.5) * 2.0)[:, :, 0:1]


def _full_frames(files):
    from PIL import Image
    return np.stack([np.asarray(Image.open(f).convert("RGB"), dtype=np.uint8)[:, :, 0] for f in files])


def _spied_callback(X, Y, files, **kw):
    """AugmentOnTheFly(warp=True) that records, per chunk, the warp parameters after the targets were made, the targets
    and the augmentation parameters the draw returned."""
    from spnet_amd import callbacks as C
    cb = C.AugmentOnTheFly(X, Y, warp=True, warp_files=files, **kw)
    log = []
    targets, apply = cb.warper.targets, cb.augmenter.apply

    def spy_targets(wp):
        Yc, rej = targets(wp)
        log.append(dict(wp={k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in wp.items()}, Y=Yc.copy(), rej=rej.copy()))
        return Yc, rej

    def spy_apply(p, out, src=None):
        log[-1]["p"] = p
        return apply(p, out, src=src)
    cb.warper.targets, cb.augmenter.apply = spy_targets, spy_apply
    return cb, log


@pytest.mark.parametrize("layout", ["monolithic", "big"])
def test_augment_on_the_fly_with_warp(espi_dir, layout, monkeypatch):
    import random
    from spnet_amd import augmentation as A
    from spnet_amd import config as cf
    from spnet_amd import utils
    monkeypatch.setattr(cf, "model_type", layout)
    n = 20
    X, Y, files, _ = utils.build_dataset(path=espi_dir, load_frac=n / 64, shuffle=False)
    files = list(files[:n])
    size = None if layout == "big" else 331
    assert X.shape == ((n, 384, 512, 1) if layout == "big" else (n, 331, 331, 1))
    full = _full_frames(files)
    meta = [utils.read_metadata(f[:-4] + ".csv") for f in files]
    cb, log = _spied_callback(X, Y, files, chunk=8, seed=1)
    np.random.seed(4)
    random.seed(4)
    cb.on_epoch_begin(0)
    torch.cuda.synchronize()
    got_X, got_Y = cb.X_aug.cpu().numpy(), cb.Y_aug.cpu().numpy()
    assert len(log) == 3
    lo = 0
    for rec in log:
        wp, p = rec["wp"], rec["p"]
        B = len(wp["index"])
        assert wp["index"].tolist() == list(range(lo, lo + B)) and p["index"].tolist() == wp["index"].tolist()
        # pixels: oracle warp at full size -> Pillow resize -> codec -> the existing augmenter with the returned parameters
        warped = np.stack([_pil_codec(R.warp_image(full[i], int(wp["flip"][j]), float(wp["angle"][j]), int(wp["xt"][j]),
                                                   int(wp["yt"][j])), size) for j, i in enumerate(wp["index"])])
        ref_aug = A.DeviceAugmenter(torch.from_numpy(warped).cuda())
        want = torch.empty_like(ref_aug.X)
        ref_aug.apply(dict(p, index=np.arange(B, dtype=np.int32)), want)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(got_X[lo:lo + B], want.cpu().numpy())
        # targets: warp_targets of the same draws, and the per-sample codec of the three-step metadata
        np.testing.assert_array_equal(got_Y[lo:lo + B], rec["Y"])
        for j, i in enumerate(wp["index"]):
            md = R.warp_meta(meta[i], int(wp["flip"][j]), float(wp["angle"][j]), int(wp["xt"][j]), int(wp["yt"][j]), 512, 384)
            np.testing.assert_array_equal(got_Y[i], R.targets(md))
        lo += B
    assert lo == n and not np.array_equal(got_Y, Y)


def test_per_sample_seeds_do_not_depend_on_chunk_or_shard(espi_dir, monkeypatch):
    from spnet_amd import callbacks as C
    from spnet_amd import config as cf
    from spnet_amd import utils
    monkeypatch.setattr(cf, "model_type", "monolithic")
    n = 16
    X, Y, files, _ = utils.build_dataset(path=espi_dir, load_frac=n / 64, shuffle=False)
    files = list(files[:n])
    a = C.AugmentOnTheFly(X, Y, warp=True, warp_files=files, chunk=4, seed=7)
    b = C.AugmentOnTheFly(X, Y, warp=True, warp_files=files, chunk=16, seed=7)
    state = np.random.get_state()
    a._augment_shard(np.array([3, 9, 1, 14, 6, 0, 11]), 2)
    b._augment_shard(np.array([11, 6, 2, 3, 1]), 2)
    assert np.array_equal(np.random.get_state()[1], state[1])            # the process-wide stream is left alone
    torch.cuda.synchronize()
    for i in (11, 6, 3, 1):
        assert torch.equal(a.X_aug[i], b.X_aug[i]) and torch.equal(a.Y_aug[i], b.Y_aug[i])
        assert not torch.equal(a.X_aug[i], a.X_orig[i])
    assert torch.equal(a.X_aug[2], a.X_orig[2])                          # not in a's shard: pristine


def test_warp_off_is_the_parent_behaviour(espi_dir, monkeypatch):
    import random
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as C
    from spnet_amd import config as cf
    from spnet_amd import utils
    monkeypatch.setattr(cf, "model_type", "monolithic")
    n = 12
    X, Y, _, _ = utils.build_dataset(path=espi_dir, load_frac=n / 64, shuffle=False)
    cb = C.AugmentOnTheFly(X, Y, chunk=5, seed=1)
    assert cb.warper is None and not hasattr(cb, "Y_aug")
    np.random.seed(9)
    random.seed(9)
    cb.on_epoch_begin(0)
    after = (np.random.get_state(), random.getstate())
    # the parent's loop, restated: DeviceAugmenter.augment chunk by chunk
    aug = A.DeviceAugmenter(torch.from_numpy(X).cuda())
    want = aug.X.clone()
    np.random.seed(9)
    random.seed(9)
    for lo in range(0, n, 5):
        hi = min(n, lo + 5)
        aug.augment(list(range(lo, hi)), want[lo:hi])
    torch.cuda.synchronize()
    assert torch.equal(cb.X_aug, want)
    assert np.array_equal(np.random.get_state()[1], after[0][1]) and np.random.get_state()[2] == after[0][2]
    assert random.getstate() == after[1]


def test_fit_trains_on_the_warped_targets(espi_dir, monkeypatch):
    from spnet_amd import _lib as L
    from spnet_amd import callbacks as C
    from spnet_amd import config as cf
    from spnet_amd import models as M
    from spnet_amd import utils
    monkeypatch.setattr(cf, "model_type", "monolithic")
    X, Y, files, _ = utils.build_dataset(path=espi_dir, shuffle=False)
    assert X.shape[0] == 64
    np.random.seed(1)
    model = M.create_model_functional(X, Y0size=576, freeze_fac=0.0)
    cb = C.AugmentOnTheFly(X, Y, warp=True, warp_files=list(files), chunk=32, seed=1)
    seen = []
    gather = L.gather_rows

    def spy(src, index, dst):
        gather(src, index, dst)
        if dst.shape[-1] == 576:
            seen.append((src.data_ptr(), torch.equal(dst, cb.Y_aug[index.long()])))
    monkeypatch.setattr(L, "gather_rows", spy)
    hist = model.fit(X, Y, batch_size=8, epochs=1, shuffle=True, verbose=0, callbacks=[cb])
    assert len(seen) == 8
    assert all(ptr == cb.Y_aug.data_ptr() and same for ptr, same in seen)
    assert not torch.equal(cb.Y_aug.cpu(), torch.from_numpy(Y))
    assert np.isfinite(hist["loss"][0])


def test_augment_data_tool_and_train_cli(tmp_path):
    _need_gpu()
    from PIL import Image
    import augment_preproc as AP
    from spnet_amd import fake_espi as F
    from spnet_amd import utils
    data = tmp_path / "data"
    F.write_dataset(str(data / "Train"), 6, seed=8)
    F.write_dataset(str(data / "Val"), 8, seed=9)
    train = str(data / "Train")
    originals = sorted(glob.glob(train + "/*.png"))
    Image.open(originals[2]).convert("RGB").save(originals[2])                  # one 3-channel file
    before = {f: np.asarray(Image.open(f)) for f in originals}
    rows = {f: utils.read_metadata(f[:-4] + ".csv") for f in originals}
    written = AP.augment_data(path=train, n_augs=3, seed=2, chunk=7)
    assert len(written) == 18 and len(set(p for p, _ in written)) == 18
    assert len(glob.glob(train + "/*.png")) == 24 and len(glob.glob(train + "/*.csv")) == 24
    shifted = 0
    for k, (prefix, prm) in enumerate(written):
        src = originals[k // 3]
        xt, yt = prm["xt"] or 0, prm["yt"] or 0
        stem = src[:-4]
        want_name = stem + ({0: "_v", 1: "_h", -1: "_vh"}.get(prm["flip"], "")) + "_r{:>.2f}".format(prm["angle"]) + \
            ("_t%d,%d" % (xt, yt) if prm["xt"] is not None else "")
        assert prefix == want_name
        shifted += prm["xt"] is not None
        img = Image.open(prefix + ".png")
        assert img.mode == Image.open(src).mode
        np.testing.assert_array_equal(np.asarray(img), R.warp_image(before[src], prm["flip"], prm["angle"], xt, yt))
        md = R.warp_meta(rows[src], prm["flip"], prm["angle"], xt, yt, 512, 384)
        assert open(prefix + ".csv").read() == "\n".join("{0},{1},{2},{3},{4},{5}".format(*r) for r in md)
    assert shifted > 0
    X, Y, file_list, _ = utils.build_dataset(path=train + "/", shuffle=False)
    assert X.shape[0] == 24 and Y.shape == (24, 576)
    # train_spnet.py --warp runs to completion on that directory
    work = tmp_path / "work"
    work.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_spnet.py"), "-d", str(data), "-b", "8", "-e", "1", "--warp",
                        "--name", "w"], cwd=str(work), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert "SPNet execution completed." in r.stdout and "warps rejected" in r.stdout
