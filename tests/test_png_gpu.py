"""The device PNG encoder (csrc/png.hip through spnet_amd/png.py) against its numpy / Python specification
(tests/helpers/png_ref.py, itself checked against zlib and Pillow in tests/test_png_cpu.py): histogram, Adler-32 and the zlib
stream byte for byte, each frame alone and inside a mixed batch, at a byte offset that is not word aligned and with
sentinels around the slots; then the writers that use it, end to end.

Frames: the smallest that can still break the packer (1 x 1; odd sizes whose stream ends in mid-word; one literal; two
literals; flat noise with 8-9 bit codes; Fibonacci counts, which need the length limiter) and the two full-size ones (more
than one 16,384-symbol tile, so the carried bit offset and the workgroup scan are exercised).

Size bound (derived, not measured): zlib stream <= ceil(9/8 * filtered bytes) + 1024.  A Huffman code averages less than the
entropy + 1 bits per symbol and a 257-symbol source has at most log2(257) < 8.01 bits, so an unlimited code stays below 9.01
bits per byte -- and a code that needed the limiter comes from a skewed histogram whose average is far below 8; the 1024
bytes cover the header (< 2048 bits), the 0.01 * n term at these sizes, the Adler-32, the zlib header and the padding.  The
helper's streams meet it on the CPU (test_png_cpu.py) before the device is asked to."""
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import png_ref as R

pytestmark = pytest.mark.gpu

BASE = 3            # the first slot starts here: not word aligned
PAD = 64            # sentinel bytes behind the last slot
SENTINEL = 0xA5

NAMES = sorted(R.small_frames()) + ["espi_384x512", "rgb_384x512x3"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def frames():
    _need_gpu()
    from spnet_amd import fake_espi as F
    out = dict(R.small_frames())
    _, _, U = F.generate_device(1, seed=4, want_u8=True)
    espi = U.cpu().numpy()[0]
    assert espi.shape == (384, 512) and espi.dtype == np.uint8
    out["espi_384x512"] = espi
    out["rgb_384x512x3"] = np.stack([espi, espi[::-1] // 2, 255 - espi], axis=2)
    return out


@pytest.fixture(scope="module")
def reference(frames):
    """name -> (zlib stream, intermediate values) of the helper; computed once, never changed."""
    return {k: R.zlib_stream(v) for k, v in frames.items()}


def _encode(batch):
    """Runs both kernels on a [N, ...] host batch; the whole output buffer comes back, sentinels included."""
    from spnet_amd import png as P
    dev = torch.from_numpy(batch).cuda()
    hist, adler = P.frame_statistics(dev)
    plan = P.plan_frames(hist)
    end = BASE + int(plan["offsets"][-1])
    size = (end + PAD + 3) // 4 * 4
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    buf[:BASE] = SENTINEL
    buf[end:] = SENTINEL
    P.pack_frames(dev, plan, adler, out=buf, base=BASE)
    out = buf.cpu().numpy()
    off = plan["offsets"] + BASE
    streams = [out[int(off[n]):int(off[n + 1])].tobytes() for n in range(batch.shape[0])]
    return dict(hist=hist, adler=adler.cpu().numpy().view(np.uint32), plan=plan, out=out, end=end, streams=streams)


def _check_frame(frame, z, hist, adler, want=None):
    from spnet_amd import png as P
    stream = R.filtered_stream(frame)
    assert np.array_equal(hist, R.histogram(stream))
    assert int(adler) == R.adler32(stream) == zlib.adler32(stream.tobytes())
    if want is not None:
        assert len(z) == len(want)
        assert z == want                                                      # byte for byte
    assert zlib.decompress(z) == stream.tobytes()
    assert len(z) <= -(-9 * stream.size // 8) + 1024
    channels = 1 if frame.ndim == 2 else frame.shape[2]
    im = Image.open(io.BytesIO(P.png_container(z, frame.shape[1], frame.shape[0], channels)))
    im.load()
    assert np.array_equal(np.asarray(im), frame)


def _check_guards(res):
    assert (res["out"][:BASE] == SENTINEL).all() and (res["out"][res["end"]:] == SENTINEL).all()
    assert res["out"].size - res["end"] >= PAD


@pytest.mark.parametrize("name", NAMES)
def test_one_frame_alone(name, frames, reference):
    frame = frames[name]
    want, info = reference[name]
    assert len(want) <= -(-9 * info["stream"].size // 8) + 1024               # the helper meets the bound first
    res = _encode(frame[None])
    _check_frame(frame, res["streams"][0], res["hist"][0], res["adler"][0], want)
    _check_guards(res)
    assert res["end"] - BASE == len(want)
    again = _encode(frame[None])
    assert np.array_equal(again["out"], res["out"])                           # two runs, identical bytes


@pytest.mark.parametrize("name", NAMES)
def test_frame_in_a_mixed_batch(name, frames, reference):
    """Five frames of one shape and different contents: other offsets, other bit tails, slots that share words."""
    frame = frames[name]
    batch = R.batch_of(frame, 5)
    assert np.array_equal(batch[2], frame)
    res = _encode(batch)
    small = frame.size <= 20000
    for n in range(5):
        want = reference[name][0] if n == 2 else (R.zlib_stream(batch[n])[0] if small else None)
        _check_frame(batch[n], res["streams"][n], res["hist"][n], res["adler"][n], want)
    _check_guards(res)
    assert len({len(s) for s in res["streams"]}) > 1 or name == "grey_1x1"    # the slots really differ in size
    again = _encode(batch)
    assert np.array_equal(again["out"], res["out"])


def test_public_encoders_and_the_writer(frames, reference, tmp_path):
    from spnet_amd import png as P
    for name in ("grey_7x13", "rgb_3x5", "espi_384x512"):
        frame = frames[name]
        dev = torch.from_numpy(np.stack([frame, frame[::-1].copy()])).cuda()
        files = P.encode_png_device(dev)
        assert files[0] == R.png_bytes(frame, reference[name][0])
        for tag, data, crc in R.read_chunks(files[1]):
            assert crc == zlib.crc32(data, zlib.crc32(tag))
        paths = [str(tmp_path / ("%s_%d.png" % (name, k))) for k in range(2)]
        sizes = P.write_png_device(dev, paths, threads=2)
        assert [open(p, "rb").read() for p in paths] == files and sizes == [len(f) for f in files]
        assert np.array_equal(np.asarray(Image.open(paths[1])), frame[::-1])
    assert P.encode_png_device(torch.empty((0, 4, 4), dtype=torch.uint8, device="cuda")) == []
    with pytest.raises(ValueError):
        P.write_png_device(torch.zeros((2, 4, 4), dtype=torch.uint8, device="cuda"), ["one.png"])


def test_entry_points_refuse_bad_arguments():
    from spnet_amd import _lib as L
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    words = torch.zeros(1024, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 32], dtype=torch.int64, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    s = L.current_stream()
    p, w = src.data_ptr(), words.data_ptr()
    for bad in ((1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 5), (-1, 8, 8, 1), (1, 1 << 14, 1 << 14, 1)):
        with pytest.raises(L.HipError):
            L.spnet_png_hist(p, *bad, w, w, s)
    with pytest.raises(L.HipError):
        L.spnet_png_hist(p, 1, 8, 8, 1, w + 1, w, s)                          # misaligned histogram
    with pytest.raises(L.HipError):
        L.spnet_png_pack(p, 1, 8, 8, 1, w, w, w, offs.data_ptr(), w, out.data_ptr(), 62, s)      # not whole words
    with pytest.raises(L.HipError):
        L.spnet_png_pack(p, 1, 8, 8, 1, w, w, w, offs.data_ptr(), w, out.data_ptr() + 1, 60, s)
    L.spnet_png_hist(p, 0, 8, 8, 1, w, w, s)                                  # empty batch: nothing to do
    # a slot that is too small for its stream is cut off at the slot's end, never written past it
    frame = torch.arange(64, dtype=torch.uint8, device="cuda").reshape(1, 8, 8)
    from spnet_amd import png as P
    hist, adler = P.frame_statistics(frame)
    plan = P.plan_frames(hist)
    plan["offsets"][1] = 20
    buf = torch.zeros(128, dtype=torch.uint8, device="cuda")
    buf[20:] = SENTINEL
    P.pack_frames(frame, plan, adler, out=buf)
    got = buf.cpu().numpy()
    assert (got[20:] == SENTINEL).all() and got[0] == 0x78 and got[1] == 0x01


def _decoded(directory):
    return {f: np.asarray(Image.open(os.path.join(directory, f))) for f in sorted(os.listdir(directory)) if f.endswith(".png")}


def _texts(directory):
    return {f: open(os.path.join(directory, f)).read() for f in sorted(os.listdir(directory)) if f.endswith(".csv")}


@pytest.fixture(scope="module")
def datasets(tmp_path_factory):
    """Eight fake-ESPI frames written twice by gen_fake_espi's writer: Pillow's files, and the device encoder's."""
    _need_gpu()
    import gen_fake_espi as G
    host, dev = (str(tmp_path_factory.mktemp(k)) for k in ("png_host", "png_device"))
    rows_h = G.gen_dataset(datapath=host, numframes=8, everything=True, seed=6, chunk=5)
    rows_d = G.gen_dataset(datapath=dev, numframes=8, everything=True, seed=6, chunk=5, device_png=True)
    assert rows_h == rows_d
    return host, dev


def test_gen_fake_espi_writer_with_device_png(datasets):
    host, dev = datasets
    n = 0
    for sub in ("Train", "Val"):
        a, b = _decoded(os.path.join(host, sub)), _decoded(os.path.join(dev, sub))
        assert sorted(a) == sorted(b) and a
        for f in a:
            assert a[f].shape == (384, 512) and np.array_equal(a[f], b[f]), f
        assert _texts(os.path.join(host, sub)) == _texts(os.path.join(dev, sub))
        n += len(a)
    assert n == 8


def test_augment_preproc_with_device_png(datasets, tmp_path):
    """A grey and an RGB image, three copies each: the warped planes are interleaved and encoded in HBM."""
    import shutil
    import augment_preproc as AP
    src = os.path.join(datasets[0], "Train")
    out = {}
    for mode in ("host", "device"):
        d = str(tmp_path / mode)
        os.makedirs(d)
        shutil.copy(os.path.join(src, "steelpan_0000000.csv"), os.path.join(d, "a.csv"))
        shutil.copy(os.path.join(src, "steelpan_0000001.csv"), os.path.join(d, "b.csv"))
        shutil.copy(os.path.join(src, "steelpan_0000000.png"), os.path.join(d, "a.png"))
        g = np.asarray(Image.open(os.path.join(src, "steelpan_0000001.png")))
        Image.fromarray(np.stack([g, g // 2, 255 - g], axis=2)).save(os.path.join(d, "b.png"))
        written = AP.augment_data(path=d, n_augs=3, seed=2, device_png=(mode == "device"))
        assert len(written) == 6
        out[mode] = (_decoded(d), _texts(d))
    assert sorted(out["host"][0]) == sorted(out["device"][0]) and len(out["host"][0]) == 8
    for f, pix in out["host"][0].items():
        assert pix.shape == ((384, 512, 3) if f.startswith("b") else (384, 512)) and np.array_equal(pix, out["device"][0][f]), f
    assert out["host"][1] == out["device"][1]


def test_show_pred_ellipses_with_device_png(datasets, tmp_path):
    from spnet_amd import config as cf
    from spnet_amd import utils
    train = os.path.join(datasets[1], "Train")                               # the device-written frames are the input
    files = [os.path.join(train, f) for f in sorted(os.listdir(train)) if f.endswith(".png")][:3]
    v = cf.vars_per_pred
    Yp = np.zeros((3, 4 * v), np.float32)
    Yp[:, 6::v] = 1.0                                                         # every slot empty ...
    Yt = Yp.copy()
    for j in range(3):                                                        # ... but one or two ellipses per frame
        Yp[j, 0:8] = (150 + 40 * j, 120 + 30 * j, 60, 35, np.cos(0.8 * j), np.sin(0.8 * j), 0, 3.4 + j)
        Yt[j, 0:8] = (155 + 40 * j, 118 + 30 * j, 58, 36, np.cos(0.8 * j), np.sin(0.8 * j), 0, 3.0 + j)
    Yp[1, v:v + 8] = (400, 300, 30, 20, 1.0, 0.0, 0, 1.0)
    outs = {}
    for mode in ("host", "device"):
        d = str(tmp_path / mode)
        os.makedirs(d)
        utils.show_pred_ellipses(Yt, Yp, files, num_draw=3, log_dir=d, out_csv=os.path.join(d, "pred.csv"), png=mode,
                                 png_chunk=2)
        outs[mode] = (_decoded(d), _texts(d))
    pix_h, pix_d = outs["host"][0], outs["device"][0]
    assert sorted(pix_h) == sorted(pix_d) == ["steelpan_pred_%05d.png" % j for j in range(3)]
    for f in pix_h:
        assert pix_h[f].shape == (384, 512, 3) and np.array_equal(pix_h[f], pix_d[f]), f
        assert (pix_h[f] != np.asarray(Image.open(files[0]).convert("RGB"))).any()
    assert outs["host"][1] == outs["device"][1] and outs["host"][1]["pred.csv"].count("\n") == 4
    with pytest.raises(ValueError):
        utils.show_pred_ellipses(Yt, Yp, files, num_draw=1, log_dir=str(tmp_path), png="gpu")
