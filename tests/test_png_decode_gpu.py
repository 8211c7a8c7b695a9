"""PNG decoding on the GPU (spnet_amd/csrc/png_decode.hip through spnet_amd/png.py) against Pillow's decode of the same
bytes, over the corpus of tests/helpers/png_decode_corpus.py.  For every good file the list of host-fallback indices
must be empty: the fallback must not be what makes a test pass."""
import io
import os

import numpy as np
import pytest
import torch

from spnet_amd import png as P
from tests.helpers import png_decode_corpus as C

pytestmark = pytest.mark.gpu
GUARD = 64
PATTERN = 0xA5


def by_shape(cases):
    groups = {}
    for c in cases:
        groups.setdefault(c.shape, []).append(c)
    return groups


@pytest.fixture(scope="module")
def good():
    cases = C.good_files()
    frames = torch.from_numpy(C.noise((3,) + C.SMALL, 61)).cuda()           # the project's own encoder: a round trip
    for k, data in enumerate(P.encode_png_device(frames)):
        cases.append(C.Case("own_encoder_%d" % k, bytes(data), C.SMALL, None))
    return cases


def test_every_good_file_decodes_on_the_device_as_pillow_decodes_it(good):
    seen = 0
    for shape, cases in sorted(by_shape(good).items()):
        datas = [c.data for c in cases]
        full, status, fallback = P.decode_png_device(datas, channels="all", return_info=True)
        assert fallback == [] and not status.any(), (shape, [(cases[k].name, P.STATUS_NAMES[status[k]]) for k in fallback])
        assert full.is_cuda and full.dtype == torch.uint8 and tuple(full.shape) == (len(cases),) + shape
        got = full.cpu().numpy()
        for k, c in enumerate(cases):
            assert np.array_equal(got[k], C.pillow_pixels(c.data)), c.name
        seen += len(cases)
    assert seen == len(good)


def test_channel_zero_equals_load_one_in_batches_that_mix_colour_types(good):
    groups = {}
    for c in good:
        groups.setdefault(c.shape[:2], []).append(c)
    assert any(len({c.shape[2] for c in cases}) == 4 for cases in groups.values())
    for hw, cases in sorted(groups.items()):
        first, status, fallback = P.decode_png_device([c.data for c in cases], channels="first", return_info=True)
        assert fallback == [] and not status.any(), hw
        assert tuple(first.shape) == (len(cases),) + hw
        got = first.cpu().numpy()
        for k, c in enumerate(cases):
            assert np.array_equal(got[k], C.load_one_pixels(c.data)), c.name


def test_host_only_formats_come_back_through_the_fallback():
    host = C.host_only_files()
    goodies = [c for c in C.pillow_files() if c.shape[2] in (1, 3)]
    cases = [host[0], goodies[0]] + host[1:3] + [goodies[1]] + host[3:]
    want = [k for k, c in enumerate(cases) if c in host]
    out, status, fallback = P.decode_png_device([c.data for c in cases], return_info=True)
    assert fallback == want and not status.any()
    got = out.cpu().numpy()
    for k, c in enumerate(cases):
        assert np.array_equal(got[k], C.load_one_pixels(c.data)), c.name


def test_files_of_differing_size_are_refused_by_name(tmp_path):
    a, b = C.pillow_files()[0], C.filter_files()[0]
    paths = []
    for name, c in (("a.png", a), ("b.png", a), ("odd.png", b)):
        paths.append(str(tmp_path / name))
        with open(paths[-1], "wb") as f:
            f.write(c.data)
    with pytest.raises(ValueError, match="odd.png"):
        P.read_png_device(paths)
    with pytest.raises(ValueError, match="file 1"):
        P.decode_png_device([a.data, b.data])


def test_no_file_one_file_and_more_files_than_resident_workgroups():
    out, status, fallback = P.decode_png_device([], return_info=True)
    assert out.shape[0] == 0 and out.is_cuda and len(status) == 0 and fallback == []
    c = [c for c in C.filter_files() if c.shape == (17, 31, 3) and c.name.startswith("filtermix")][0]
    one = P.decode_png_device([c.data], channels="all")
    assert np.array_equal(one.cpu().numpy()[0], C.pillow_pixels(c.data))
    many, status, fallback = P.decode_png_device([c.data] * 2000, channels="all", return_info=True)
    assert fallback == [] and not status.any()
    assert bool((many == one).all())


def test_malformed_files_end_alone_and_write_nothing_outside_their_slot(tmp_path):
    """Malformed streams (the stand-alone host program has passed on the same bytes in tests/test_png_decode_cpu.py)
    interleaved with good files in one launch, called at the C ABI so that guard bytes can surround every slot."""
    from spnet_amd import _lib as L
    bad = C.malformed_files() + C.bit_flip_files()             # the 200 flips the host program has seen
    shape = C.SMALL
    H, W, ch = shape
    goodies = [c for c in C.filter_files() if c.shape == shape]
    cases = []
    for k, c in enumerate(bad):
        cases += [c, goodies[k % len(goodies)]]
    N = len(cases)
    length = H * (1 + W * ch)
    streams = [bytes(P.parse_png(c.data).zstream) for c in cases]
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum([len(s) for s in streams])
    offsets += GUARD
    blob = np.full(int(offsets[-1]) + GUARD, PATTERN, np.uint8)
    for k, s in enumerate(streams):
        blob[int(offsets[k]):int(offsets[k + 1])] = np.frombuffer(s, np.uint8)
    stride = length + GUARD
    d_blob, d_off = torch.from_numpy(blob).cuda(), torch.from_numpy(offsets).cuda()
    d_out = torch.full((GUARD + N * stride,), PATTERN, dtype=torch.uint8, device="cuda")
    d_pix = torch.full((GUARD + N * H * W * ch + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    d_status = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    L.spnet_png_inflate(d_blob.data_ptr(), int(d_blob.numel()), d_off.data_ptr(), N, length, stride,
                        d_out.data_ptr() + GUARD, d_status.data_ptr(), L.current_stream())
    L.spnet_png_unfilter(d_out.data_ptr() + GUARD, stride, N, H, W, ch, 0, d_pix.data_ptr() + GUARD, d_status.data_ptr(),
                         L.current_stream())
    status = d_status.cpu().numpy()
    out = d_out.cpu().numpy()
    pix = d_pix.cpu().numpy()
    assert np.array_equal(d_blob.cpu().numpy(), blob)
    assert (out[:GUARD] == PATTERN).all() and (pix[:GUARD] == PATTERN).all() and (pix[-GUARD:] == PATTERN).all()
    slots = out[GUARD:].reshape(N, stride)
    assert (slots[:, length:] == PATTERN).all(), "guard bytes behind a slot were written"
    frames = pix[GUARD:-GUARD].reshape(N, H, W, ch)
    import zlib
    for k, c in enumerate(cases):
        if c.expect is None and c.name.startswith("flip_"):               # zlib is the judge of a flipped stream
            try:
                ok = len(zlib.decompress(streams[k])) == length
            except zlib.error:
                ok = False
            assert (status[k] == 0) == ok, c.name
        elif c.expect is not None:
            assert status[k] != 0, c.name
            assert status[k] in c.expect or c.name == "bad_filter_5" and status[k] == C.BAD_FILTER, (c.name, status[k])
        else:
            assert status[k] == 0, (c.name, P.STATUS_NAMES[status[k]])
            assert np.array_equal(frames[k], C.pillow_pixels(c.data)), c.name
    # through the public reader every malformed file behaves as the default path's decoder does on it
    for k, c in enumerate(bad):
        path = str(tmp_path / (c.name + ".png"))
        with open(path, "wb") as f:
            f.write(c.data)
        neighbour = str(tmp_path / "good.png")
        with open(neighbour, "wb") as f:
            f.write(goodies[0].data)
        try:
            want = C.load_one_pixels(c.data)
        except Exception as e:                # noqa: BLE001 - whatever the default path raises is the contract
            with pytest.raises(type(e)):
                P.read_png_device([neighbour, path])
            continue
        got, status, fallback = P.read_png_device([neighbour, path], return_info=True)
        assert np.array_equal(got[1].cpu().numpy(), want), c.name
        assert np.array_equal(got[0].cpu().numpy(), C.load_one_pixels(goodies[0].data))


def test_entry_points_refuse_bad_arguments():
    from spnet_amd import _lib as L
    t = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    o = torch.zeros(4, dtype=torch.int64, device="cuda")
    s = torch.zeros(4, dtype=torch.int32, device="cuda")
    for args in ((t.data_ptr(), 1024, o.data_ptr(), 1, 0, 0, t.data_ptr(), s.data_ptr()),            # L < 1
                 (t.data_ptr(), 1024, o.data_ptr(), 1, 64, 63, t.data_ptr(), s.data_ptr()),          # stride < L
                 (t.data_ptr(), 1024, o.data_ptr() + 4, 1, 64, 64, t.data_ptr(), s.data_ptr()),      # misaligned offsets
                 (0, 1024, o.data_ptr(), 1, 64, 64, t.data_ptr(), s.data_ptr())):
        with pytest.raises(Exception):
            L.spnet_png_inflate(*args, L.current_stream())
    for args in ((t.data_ptr(), 64, 1, 3, 5, 5, t.data_ptr(), 0, s.data_ptr()),                      # 5 channels
                 (t.data_ptr(), 10, 1, 3, 5, 1, t.data_ptr(), 0, s.data_ptr()),                      # stride < L
                 (t.data_ptr(), 18, 1, 3, 5, 1, 0, 0, s.data_ptr())):                                # no output
        with pytest.raises(Exception):
            L.spnet_png_unfilter(*args, L.current_stream())
    # an extent outside the blob ends that file alone
    o[0], o[1] = 0, 5000
    L.spnet_png_inflate(t.data_ptr(), 1024, o.data_ptr(), 1, 64, 64, t.data_ptr(), s.data_ptr(), L.current_stream())
    assert int(s[0]) == 12


# ----------------------------------------------------------------------------- end to end at toy size
@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from spnet_amd import fake_espi as F
    data = tmp_path_factory.mktemp("decode_frames")
    F.write_dataset(str(data) + "/", 16, seed=6)
    return data, sorted(str(p) for p in data.glob("*.png"))


def test_build_x_and_predict_are_bit_identical_with_device_decode(dataset, tmp_path):
    import predict_spnet
    from spnet_amd import config as cf
    from spnet_amd import models as M
    from spnet_amd import utils as U
    assert cf.model_type == "monolithic"
    data, files = dataset
    X_host, dims = U.build_X(16, files, force_dim=331, grayscale=True, as_uint8=True, device_resize=True)
    X_dev, dims_dev = U.build_X(16, files, force_dim=331, grayscale=True, as_uint8=True, device_decode=True)
    assert X_dev.is_cuda and X_dev.dtype == torch.uint8 and tuple(X_dev.shape) == (16, 384, 512, 1) and dims_dev == dims
    assert np.array_equal(X_dev.cpu().numpy(), X_host)
    _, status, fallback = P.read_png_device(files, return_info=True)
    assert fallback == [] and not status.any()
    model = M.Model((331, 331, 1), Y0size=576, seed=8)
    y_host = model.predict(X_host, batch_size=8, resize=True)
    y_dev = model.predict(X_dev, batch_size=8, resize=True)
    assert np.array_equal(np.asarray(y_dev), np.asarray(y_host))


def run_cli(cmd, cwd):
    """A child process, as tests/test_cli_gpu.py starts its entry points."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, cmd[0])] + cmd[1:], cwd=cwd, env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_predict_and_evaluate_cli_write_the_same_csv_with_device_decode(dataset, tmp_path):
    """predict_spnet.py --device_decode against --device_resize --u8_frames, evaluate_spnet.py --device_decode against the
    default: each flag goes through argparse, the loaders and the model set-up of a fresh process."""
    from spnet_amd import models as M
    data, _ = dataset
    model = M.Model((331, 331, 1), Y0size=576, seed=8)
    model.save_weights(str(tmp_path / "w.hdf5"))
    model.save(str(tmp_path / "full_model.h5"))
    del model
    csv = {}
    for name, flags in (("resize", ["--device_resize", "--u8_frames"]), ("decode", ["--device_decode"])):
        out = run_cli(["predict_spnet.py", "-w", "w.hdf5", "-d", str(data), "-b", "8", "-l", "logs/p_%s/" % name] + flags,
                      str(tmp_path))
        assert "FPS = " in out
        csv[name] = (tmp_path / "logs" / ("p_" + name) / "hawley_spnet.csv").read_bytes()
    assert len(csv["resize"].splitlines()) >= 16 and csv["decode"] == csv["resize"]
    for name, flags in (("default", []), ("decode", ["--device_decode"])):
        out = run_cli(["evaluate_spnet.py", "-d", str(data), "-b", "8", "-l", "logs/e_%s/" % name] + flags, str(tmp_path))
        assert "mAP = " in out
        csv[name] = ((tmp_path / "logs" / ("e_" + name) / "hawley_spnet.csv").read_bytes(),
                     [l for l in out.splitlines() if l.startswith(("mAP", "Mean pixel error"))])
    assert len(csv["default"][0].splitlines()) >= 16 and csv["decode"] == csv["default"]


def test_first_augmented_epoch_is_the_same_with_device_decode(dataset):
    """AugmentOnTheFly(warp=True): one epoch begin of both callbacks from the same seeds -- the augmented frames and the
    recomputed targets are equal, so the frames handed to the warper and every draw after them are."""
    import random
    from spnet_amd import callbacks as CB
    from spnet_amd import utils as U
    data, files = dataset
    X, _ = U.build_X(16, files, force_dim=331, grayscale=True)
    Y, _ = U.build_Y(16, [os.path.splitext(f)[0] + ".csv" for f in files], files)
    got = {}
    for flag in (False, True):
        cb = CB.AugmentOnTheFly(X, Y, seed=3, chunk=8, warp=True, warp_files=files, device_decode=flag)
        assert cb.warper.X.is_cuda and cb.warper.X.dtype == torch.uint8 and cb.warper.X.is_contiguous()
        np.random.seed(4)
        random.seed(4)
        cb.on_epoch_begin(0)
        torch.cuda.synchronize()
        got[flag] = (cb.X_aug.cpu().numpy(), cb.Y_aug.cpu().numpy(), cb.warper.X.cpu().numpy())
    assert not np.array_equal(got[False][0], X) and not np.array_equal(got[False][1], Y)          # something was augmented
    for a, b in zip(got[False], got[True]):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.fixture(scope="module")
def real_frames(tmp_path_factory):
    """Real frames of the mix-up: two grey files, one RGB file whose channels differ, one grey file with tRNS."""
    from PIL import Image
    d = tmp_path_factory.mktemp("real")
    rng = np.random.default_rng(5)
    for k in range(2):
        Image.fromarray(rng.integers(0, 256, (384, 512), dtype=np.uint8), "L").save(str(d / ("a%d_grey.png" % k)))
    Image.fromarray(rng.integers(0, 256, (384, 512, 3), dtype=np.uint8), "RGB").save(str(d / "b_rgb.png"))
    Image.fromarray(rng.integers(0, 256, (384, 512), dtype=np.uint8), "L").save(str(d / "c_trns.png"), transparency=7)
    return str(d)


def test_real_frames_of_the_mix_up_with_device_decode(real_frames, dataset):
    """--bp_real: grey files are decoded on the device, an RGB file goes to the host and keeps convert("L")'s pixels."""
    import random
    from PIL import Image
    from spnet_amd import augmentation as A
    from spnet_amd import callbacks as CB
    from spnet_amd import utils as U
    files, want = A.read_real_frames(real_frames, 384, 512)
    files_d, got, host = A.read_real_frames(real_frames, 384, 512, device_decode=True, return_info=True)
    assert files_d == files and [os.path.basename(files[k]) for k in host] == ["b_rgb.png", "c_trns.png"]
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    rgb = np.asarray(Image.open(files[2]).convert("RGB"))
    assert not np.array_equal(rgb[:, :, 0], want[2])                  # channel 0 would have been wrong for this file
    with pytest.raises(ValueError, match="real image"):
        A.read_real_frames(real_frames, 331, 331, device_decode=True)
    pools = [A.BandpassPool(real_frames, 384, 512, device_decode=flag) for flag in (False, True)]
    assert bool((pools[0].images == pools[1].images).all()) and bool((pools[0].table == pools[1].table).all())
    # through the callback: the first augmented epoch with the mix-up on every frame
    data, names = dataset
    X, _ = U.build_X(16, names, force_dim=None, grayscale=True)
    Y, _ = U.build_Y(16, [os.path.splitext(f)[0] + ".csv" for f in names], names)
    out = {}
    for flag in (False, True):
        A.BandpassPool._cache.clear()
        cb = CB.AugmentOnTheFly(X, Y, seed=3, chunk=8, bandpass_real=real_frames, bpmix_prob=1.0, device_decode=flag)
        np.random.seed(4)
        random.seed(4)
        cb.on_epoch_begin(0)
        torch.cuda.synchronize()
        out[flag] = cb.X_aug.cpu().numpy()
    A.BandpassPool._cache.clear()
    assert not np.array_equal(out[False], X) and np.array_equal(out[True], out[False])


def test_augment_preproc_writes_the_same_files_with_device_decode(dataset, tmp_path):
    """augment_preproc.py --device_decode: grey, RGB and RGBA originals decoded on the device, a palette file by the host;
    every PNG and CSV written is byte for byte the one of the default run."""
    import shutil
    from PIL import Image
    import augment_preproc
    data, files = dataset
    dirs = {}
    for flag in (False, True):
        d = tmp_path / ("aug_%d" % flag)
        d.mkdir()
        for f in files[:5]:
            shutil.copy(f, str(d))
            shutil.copy(os.path.splitext(f)[0] + ".csv", str(d))
        grey = Image.open(files[5])
        for k, img in enumerate((grey.convert("RGB"), grey.convert("RGBA"), grey.convert("P"))):
            img.save(str(d / ("z_extra%d.png" % k)))
            shutil.copy(os.path.splitext(files[5])[0] + ".csv", str(d / ("z_extra%d.csv" % k)))
        written = augment_preproc.augment_data(path=str(d), n_augs=2, seed=1, chunk=6, device_decode=flag)
        assert len(written) == 16
        dirs[flag] = d
    names = sorted(os.listdir(dirs[False]))
    assert names == sorted(os.listdir(dirs[True])) and len(names) == 2 * (8 + 16)
    for name in names:
        assert (dirs[True] / name).read_bytes() == (dirs[False] / name).read_bytes(), name
