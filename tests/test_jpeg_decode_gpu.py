"""The device JPEG decoder (spnet_amd/csrc/jpeg_decode.hip behind spnet_amd.jpeg.decode_jpeg_device) against Pillow, byte for
byte: the corpus of tests/helpers/jpeg_decode_corpus.py (this project's encoder and Pillow's; custom Huffman tables, chroma
4:4:4 / 4:2:2 / 4:2:0, restart markers per row, every two MCUs, none), the shapes at which the interval table changes form,
damaged files beside sound ones, the routing of mixed batches, the movie reader and the --movie_in surface."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import jpeg_decode_corpus as C
from tests.helpers import jpeg_ref

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def expected():
    """name -> Pillow's pixels; computed once, never changed."""
    _need_gpu()
    return C.expected(C.corpus())


def _check(datas, wants):
    """Both channel modes of one call over `datas` (one size, one component count) against Pillow's pixels [H][W][C]."""
    from spnet_amd import jpeg as J
    first, status, fallback = J.decode_jpeg_device(datas, channels="first", return_info=True)
    assert fallback == [] and not status.any(), (status.tolist(), fallback)
    got = first.cpu().numpy()
    for k, want in enumerate(wants):
        assert np.array_equal(got[k], want[:, :, 0]), (k, int((got[k] != want[:, :, 0]).sum()))
    full, status, fallback = J.decode_jpeg_device(datas, channels="all", return_info=True)
    assert fallback == [] and not status.any()
    got = full.cpu().numpy()
    for k, want in enumerate(wants):
        assert got[k].shape == want.shape and np.array_equal(got[k], want), (k, int((got[k] != want).sum()))


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_corpus_equals_pillow(shape, expected):
    """Every file of one size in ONE call: both encoders, every option, several Huffman table sets, all three samplings."""
    cases = [c for c in C.corpus() if c.shape == shape]
    _check([c.data for c in cases], [expected[c.name] for c in cases])


def test_interval_shapes_of_our_writer():
    """Height 88 at width 8: 11 intervals, the RST counter wraps.  Width 520 at height 8: 65 MCUs in a row, the 64-MCU cap
    gives two intervals in one row.  A q100 noise frame whose scan holds a stuffed FF 00."""
    _need_gpu()
    from spnet_amd import jpeg as J
    tall = jpeg_ref.encode_jpeg(C.content("noise", (88, 8), 1), 90)
    assert J.parse_jpeg(tall).bounds.shape[0] == 11 and b"\xff\xd0" in tall[tall.index(b"\xff\xd7"):]
    wide = jpeg_ref.encode_jpeg(C.content("noise", (8, 520), 2), 90)
    assert J.parse_jpeg(wide).bounds.shape[0] == 2 and J.parse_jpeg(wide).restart == 64
    noisy = jpeg_ref.encode_jpeg(C.content("noise", (24, 40), 3), 100)
    lo, hi = int(J.parse_jpeg(noisy).bounds[0][0]), int(J.parse_jpeg(noisy).bounds[-1][1])
    assert b"\xff\x00" in noisy[lo:hi]
    for data in (tall, wide, noisy):
        _check([data], [C.pillow_pixels(data)])


def test_tiles_and_subsampled_halos_beyond_one_tile():
    """70 x 300 colour: three tiles across and three down (32 x 128 tiles), so the chroma halo of 4:2:2 and 4:2:0 is taken
    from neighbouring tiles' blocks, and the right and bottom edges are off the MCU grid."""
    _need_gpu()
    frame = C.content("ramp", (70, 300, 3))
    frame[20:50, 100:200] = C.content("noise", (30, 100, 3), 4)
    datas = [C.pillow_jpeg(frame, quality=90, subsampling=s) for s in (0, 1, 2)] + [jpeg_ref.encode_jpeg(frame, 90)]
    _check(datas, [C.pillow_pixels(d) for d in datas])


def test_a_frame_without_dht():
    _need_gpu()
    bare = C.without_dht(C.pillow_jpeg(C.content("noise", (24, 40)), quality=90))
    _check([bare], [C.pillow_pixels(bare)])


def test_mixed_batch_through_read_frames_device(tmp_path):
    """Device JPEG files, a progressive file and a PNG in one list: order kept, the progressive file decoded by the host."""
    _need_gpu()
    from spnet_amd import jpeg as J
    frames = [C.content("noise", (24, 40), s) for s in range(5)]
    files = [jpeg_ref.encode_jpeg(frames[0], 90), C.progressive(frames[1]), None, C.pillow_jpeg(frames[3], quality=50),
             jpeg_ref.encode_jpeg(frames[4], 10)]
    paths = []
    for k, data in enumerate(files):
        p = str(tmp_path / ("f%d.%s" % (k, "png" if data is None else "jpg")))
        if data is None:
            Image.fromarray(frames[k]).save(p)
        else:
            with open(p, "wb") as f:
                f.write(data)
        paths.append(p)
    out, status, fallback = J.read_frames_device(paths, return_info=True)
    assert fallback == [1] and not status.any()
    got = out.cpu().numpy()
    for k, p in enumerate(paths):
        assert np.array_equal(got[k], np.asarray(Image.open(p).convert("RGB"))[:, :, 0]), k
    assert np.array_equal(got[2], frames[2])
    # read_jpeg_device alone, and the PNG-only list (the PNG decoder's own call)
    assert np.array_equal(J.read_jpeg_device([paths[0], paths[4]]).cpu().numpy(), got[[0, 4]])
    assert np.array_equal(J.read_frames_device([paths[2]]).cpu().numpy(), got[[2]])
    with pytest.raises(ValueError, match="one size"):
        J.decode_jpeg_device([files[0], jpeg_ref.encode_jpeg(C.content("noise", (8, 8)), 90)])


@pytest.mark.parametrize("kind", ["flipped", "cut", "unassigned"])
def test_damaged_file_between_sound_ones(kind):
    """The kernels' own statuses and writes (the frames pre-filled with a sentinel), then the public call."""
    _need_gpu()
    from spnet_amd import _lib as L
    from spnet_amd import jpeg as J
    bad, sound = C.damaged()
    datas = [sound, bad[kind], sound]
    infos = [J.parse_jpeg(d) for d in datas]
    assert all(i.device for i in infos)
    plan = J.plan_decode(infos)
    H, W = infos[0].height, infos[0].width
    dev = {k: torch.from_numpy(plan[k].view(np.uint8).reshape(-1).copy()).cuda() for k in ("intervals", "files", "tables",
                                                                                           "quant", "blob")}
    coef = torch.zeros((plan["blocks"], 64), dtype=torch.int16, device="cuda")
    status = torch.full((3,), 77, dtype=torch.int32, device="cuda")
    out = torch.full((3 * H * W + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    L.spnet_jpeg_entropy(dev["blob"].data_ptr(), int(plan["blob"].size), dev["intervals"].data_ptr(),
                         int(plan["intervals"].shape[0]), dev["files"].data_ptr(), 3, dev["tables"].data_ptr(),
                         int(plan["tables"].shape[0]), coef.data_ptr(), int(plan["blocks"]), status.data_ptr(),
                         L.current_stream())
    L.spnet_jpeg_pixels(coef.data_ptr(), int(plan["blocks"]), dev["files"].data_ptr(), 3, dev["quant"].data_ptr(),
                        int(plan["quant"].shape[0]), H, W, 1, out.data_ptr(), 0, status.data_ptr(), L.current_stream())
    st = status.cpu().numpy()
    assert st[0] == 0 and st[2] == 0 and st[1] != 0, st
    host = out.cpu().numpy()
    want = C.pillow_pixels(sound)[:, :, 0]
    assert np.array_equal(host[:H * W].reshape(H, W), want) and np.array_equal(host[2 * H * W:3 * H * W].reshape(H, W), want)
    assert (host[H * W:2 * H * W] == SENTINEL).all() and (host[3 * H * W:] == SENTINEL).all()     # a rejected file: untouched
    # the public call: Pillow's behaviour for the final result
    try:
        pil = C.pillow_pixels(bad[kind])[:, :, 0]
    except Exception as e:                                   # noqa: BLE001 -- whatever the default path raises
        with pytest.raises(type(e)):
            J.decode_jpeg_device(datas)
        return
    got, status, fallback = J.decode_jpeg_device(datas, return_info=True)
    assert fallback == [1] and status[1] != 0 and status[0] == 0 and status[2] == 0
    got = got.cpu().numpy()
    assert np.array_equal(got[0], want) and np.array_equal(got[2], want) and np.array_equal(got[1], pil)


def test_no_files():
    _need_gpu()
    from spnet_amd import jpeg as J
    assert tuple(J.decode_jpeg_device([]).shape) == (0, 0, 0)
    assert tuple(J.decode_jpeg_device([], channels="all").shape) == (0, 0, 0, 0)
    for channels, shape in (("first", (0, 0, 0)), ("all", (0, 0, 0, 0))):
        out, status, info = J.decode_jpeg_device([], channels=channels, return_info=True)
        assert tuple(out.shape) == shape and out.dtype == torch.uint8 and out.is_cuda
        assert status.shape == (0,) and status.dtype == np.int32
        assert isinstance(info, J.DecodeInfo) and info == [] and (info.lane_intervals, info.sync_intervals) == (0, 0)


@pytest.mark.parametrize("at", [0, 1, 2])
def test_host_only_file_among_device_files(at):
    """Two files the device decodes and a progressive one the host has to, first, in the middle and last: the device's
    frames are scattered into their places, the host's uploaded into its own; Pillow's pixels in input order."""
    _need_gpu()
    from spnet_amd import jpeg as J
    frames = [C.content("noise", (16, 16), s) for s in range(3)]
    datas = [jpeg_ref.encode_jpeg(frames[0], 90), C.pillow_jpeg(frames[1], quality=60)]
    datas.insert(at, C.progressive(frames[2]))
    assert [J.parse_jpeg(d).device for d in datas] == [k != at for k in range(3)]
    want = np.stack([C.pillow_pixels(d) for d in datas])
    for channels, pixels in (("first", want[:, :, :, 0]), ("all", want)):
        out, status, info = J.decode_jpeg_device(datas, channels=channels, return_info=True)
        assert info == [at] and not status.any() and info.lane_intervals + info.sync_intervals == 3
        assert np.array_equal(out.cpu().numpy(), pixels)


def test_round_trips_through_the_device_encoder_and_a_movie(tmp_path):
    _need_gpu()
    from spnet_amd import jpeg as J
    grey = torch.from_numpy(np.stack([C.content("noise", (40, 72), s) for s in range(3)])).cuda()
    colour = torch.from_numpy(np.stack([C.content("ramp", (21, 35, 3)), C.content("noise", (21, 35, 3), 7)])).cuda()
    for frames, q in ((grey, 90), (colour, 75)):
        files = J.encode_jpeg_device(frames, q)
        _check(files, [C.pillow_pixels(f) for f in files])
    path = str(tmp_path / "m.avi")
    with J.MjpegWriter(path, 72, 40, fps=30.0, channels=1, quality=80) as w:
        w.add(grey[:2])
        w.add(grey[2:])
    r = J.MjpegReader(path)
    assert len(r) == 3 and r.size == (72, 40) and r.fps == 30.0
    want = np.stack([C.pillow_pixels(r.frame_bytes(k))[:, :, 0] for k in range(3)])
    assert np.array_equal(r.read_device().cpu().numpy(), want)
    assert np.array_equal(r.read_device(slice(2, None, -2)).cpu().numpy(), want[[2, 0]])
    assert np.array_equal(r.read_device([1], channels="all").cpu().numpy(), want[[1], :, :, None])


def test_predict_on_a_movie_equals_predict_on_its_frames_as_files(tmp_path):
    """predict_network(movie_in=) on a 4-frame AVI: the rows of hawley_spnet.csv (names aside) are those of the run on the
    same JPEG frames as files through the default host path; the overlays become a movie again."""
    _need_gpu()
    import predict_spnet
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    from spnet_amd import jpeg as J
    from spnet_amd import models as M
    src = tmp_path / "png"
    F.write_dataset(str(src) + "/", 4, seed=6)
    pngs = sorted(p for p in os.listdir(src) if p.endswith(".png"))
    frames = np.stack([np.asarray(Image.open(src / p).convert("RGB"))[:, :, 0] for p in pngs])
    files = J.encode_jpeg_device(torch.from_numpy(frames).cuda(), 90)
    jpg = tmp_path / "jpg"
    jpg.mkdir()
    for k, data in enumerate(files):
        (jpg / ("strike_%05d.jpg" % k)).write_bytes(data)
    with J.MjpegWriter(str(tmp_path / "strike.avi"), frames.shape[2], frames.shape[1], channels=1,
                       encoder=lambda fr: files[:len(fr)]) as w:
        w.add(torch.from_numpy(frames))
    saved = cf.model_type
    try:
        cf.model_type = 'monolithic'
        model = M.Model((331, 331, 1), Y0size=576, seed=8)
        predict_spnet.predict_network(datapath=str(jpg), log_dir=str(tmp_path / "host") + "/", batch_size=4, model=model)
        predict_spnet.predict_network(movie_in=str(tmp_path / "strike.avi"), log_dir=str(tmp_path / "movie") + "/",
                                      batch_size=4, model=model, device_jpeg=True, movie=str(tmp_path / "strike_pred.avi"))
    finally:
        cf.model_type = saved
    a = (tmp_path / "host" / "hawley_spnet.csv").read_text().replace(".jpg", "")
    b = (tmp_path / "movie" / "hawley_spnet.csv").read_text()
    assert a == b and "strike_00003" in b
    assert sorted(os.listdir(tmp_path / "movie")) == ["hawley_spnet.csv"] + ["steelpan_pred_%05d.jpg" % k for k in range(4)]
    again = J.MjpegReader(str(tmp_path / "strike_pred.avi"))
    assert len(again) == 4 and again.size == (512, 384)
    assert again.frame_bytes(0) == (tmp_path / "movie" / "steelpan_pred_00000.jpg").read_bytes()
