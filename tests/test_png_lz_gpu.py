"""The LZ77 stage of the device PNG encoder (csrc/png_lz.hip through spnet_amd/png.py, lz77=True) against its restatement
(tests/helpers/png_lz_ref.py, itself checked against zlib and Pillow in tests/test_png_lz_cpu.py): the two histograms and
the chosen zlib stream byte for byte, each frame alone and inside a mixed batch of five in which some frames take the LZ
stream and some the literal-only fallback, at a byte offset that is not word aligned and with sentinels around the slots;
then the public functions, the entry points' argument checks and one writer end to end.

Frames: tests/helpers/png_lz_ref.lz_frames (no match at all; all-zero: length 258 at distance 1, symbol 285, overlapping
copies; periods 2 and 3; grey replicated into RGB; the repeat at distance exactly 32768 and its twin at 32769; a second tile
that repeats the first; Fibonacci counts) and the two full-size ones, a fake-ESPI frame and the same frame replicated into
three channels.  The token of 15 + 5 + 15 + 13 = 48 bits is made by handing spnet_png_lz_pack a valid code set in which the
length symbol and the distance symbol of the far frame's match have 15 bits (any complete code is legal input); production's
own codes for the frames here stay shorter (the Fibonacci frame's LZ codes are 13 and 9 deep), which the CPU test states."""
import io
import os
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import png_lz_ref as Z
from tests.helpers import png_ref as R

pytestmark = pytest.mark.gpu

BASE = 3            # the first slot starts here: not word aligned
PAD = 64            # sentinel bytes behind the last slot
SENTINEL = 0xA5

NAMES = sorted(Z.lz_frames()) + ["espi_384x512", "espi_rgb_384x512x3"]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def frames():
    _need_gpu()
    from spnet_amd import fake_espi as F
    out = dict(Z.lz_frames())
    _, _, U = F.generate_device(1, seed=4, want_u8=True)
    espi = U.cpu().numpy()[0]
    assert espi.shape == (384, 512) and espi.dtype == np.uint8
    out["espi_384x512"] = espi
    out["espi_rgb_384x512x3"] = np.stack([espi] * 3, axis=2)
    return out


@pytest.fixture(scope="module")
def reference(frames):
    """name -> (chosen stream, took LZ, the LZ stream's intermediate values) of the helper; computed once, never changed."""
    return {k: Z.chosen_stream(v) for k, v in frames.items()}


def _encode(batch, lengths=None):
    """Runs the three kernels (and the literal packer for the fallback frames) on a [N, ...] host batch; the whole output
    buffer comes back, sentinels included."""
    from spnet_amd import png as P
    dev = torch.from_numpy(batch).cuda()
    hist, adler = P.frame_statistics(dev)
    lhist, dhist = P.lz_statistics(dev)
    plan = P.plan_frames_lz(hist, lhist, dhist)
    end = BASE + int(plan["offsets"][-1])
    size = (end + PAD + 3) // 4 * 4
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    buf[:BASE] = SENTINEL
    buf[end:] = SENTINEL
    P.pack_frames_lz(dev, plan, adler, out=buf, base=BASE)
    out = buf.cpu().numpy()
    off = plan["offsets"] + BASE
    streams = [out[int(off[n]):int(off[n + 1])].tobytes() for n in range(batch.shape[0])]
    return dict(lhist=lhist, dhist=dhist, plan=plan, out=out, end=end, streams=streams)


def _check_frame(frame, z, lhist, dhist, use_lz, want=None):
    from spnet_amd import png as P
    stream = R.filtered_stream(frame)
    if want is not None:
        data, took_lz, info = want
        assert np.array_equal(lhist, info["lhist"]) and np.array_equal(dhist, info["dhist"])
        assert bool(use_lz) == took_lz
        assert len(z) == len(data)                                            # the slot is the planned size
        assert z == data                                                      # byte for byte
    assert zlib.decompress(z) == stream.tobytes()
    assert int(lhist[:256].sum()) + sum(int(c) for c in dhist) <= stream.size and int(lhist[256]) == 1
    channels = 1 if frame.ndim == 2 else frame.shape[2]
    png = P.png_container(z, frame.shape[1], frame.shape[0], channels)
    im = Image.open(io.BytesIO(png))
    im.load()
    assert np.array_equal(np.asarray(im), frame)
    return png


def _check_guards(res):
    assert (res["out"][:BASE] == SENTINEL).all() and (res["out"][res["end"]:] == SENTINEL).all()
    assert res["out"].size - res["end"] >= PAD


def _round_trip(pngs, frames):
    from spnet_amd import png as P
    got, status, host = P.decode_png_device(pngs, channels="all", return_info=True)
    assert not status.any() and host == []
    want = np.stack([f.reshape(f.shape[0], f.shape[1], -1) for f in frames])
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("name", NAMES)
def test_one_frame_alone(name, frames, reference):
    frame = frames[name]
    res = _encode(frame[None])
    png = _check_frame(frame, res["streams"][0], res["lhist"][0], res["dhist"][0], res["plan"]["use_lz"][0], reference[name])
    _check_guards(res)
    assert res["end"] - BASE == len(reference[name][0]) <= len(R.zlib_stream(frame)[0])
    _round_trip([png], [frame])
    again = _encode(frame[None])
    assert np.array_equal(again["out"], res["out"])                           # two runs, identical bytes
    assert np.array_equal(again["lhist"], res["lhist"]) and np.array_equal(again["dhist"], res["dhist"])


@pytest.mark.parametrize("name", NAMES)
def test_frame_in_a_mixed_batch(name, frames, reference):
    """Five frames of one shape and different contents (the last one is noise: literal-only), slots that share words."""
    frame = frames[name]
    batch = R.batch_of(frame, 5)
    assert np.array_equal(batch[2], frame)
    res = _encode(batch)
    small = frame.size <= 20000
    use = res["plan"]["use_lz"]
    pngs = []
    for n in range(5):
        want = reference[name] if n == 2 else (Z.chosen_stream(batch[n]) if small else None)
        pngs.append(_check_frame(batch[n], res["streams"][n], res["lhist"][n], res["dhist"][n], use[n], want))
        if not use[n]:
            assert res["streams"][n] == R.zlib_stream(batch[n])[0]            # a fallback frame: the literal-only bytes
    _check_guards(res)
    if name in ("zeros_64x64", "tile_repeat_17000", "far_32768", "espi_rgb_384x512x3", "replicated_16x24x3"):
        assert use.any() and not use.all()                                    # both packers wrote into this buffer
    _round_trip(pngs, list(batch))
    again = _encode(batch)
    assert np.array_equal(again["out"], res["out"])


def test_noise_frame_is_never_longer(frames):
    """lz77=True on the full-size noise frame: the literal-only bytes if the host chose the fallback, else fewer bytes."""
    from spnet_amd import png as P
    dev = torch.from_numpy(frames["espi_384x512"][None]).cuda()
    plain = P.zlib_streams_device(dev)[0].tobytes()
    lz = P.zlib_streams_device(dev, lz77=True)[0].tobytes()
    hist, _ = P.frame_statistics(dev)
    plan = P.plan_frames_lz(hist, *P.lz_statistics(dev))
    assert plain == R.zlib_stream(frames["espi_384x512"])[0]
    if plan["use_lz"][0]:
        assert len(lz) < len(plain)
    else:
        assert lz == plain
    rgb = torch.from_numpy(frames["espi_rgb_384x512x3"][None]).cuda()
    assert len(P.zlib_streams_device(rgb, lz77=True)[0]) < len(P.zlib_streams_device(rgb)[0])


def test_a_token_of_48_bits(frames):
    """The far frame's match (length 199: symbol 283, 5 extra bits; distance 32768: symbol 29, 13 extra bits) packed with a
    code set that gives both symbols 15 bits: one token of 48 bits crosses the packer's 32-bit flush twice."""
    from spnet_amd import _lib as L
    from spnet_amd import png as P
    frame = frames["far_32768"]
    info = Z.lz_stream(frame)[1]
    assert (34919, 199, 32768) in info["tokens"] and Z.length_symbol(199)[:2] == (283, 5) and Z.distance_symbol(32768)[:2] == (29, 13)
    ll, dl = Z.forced_lengths(286, 283), Z.forced_lengths(30, 29)
    assert ll[283] + 5 + dl[29] + 13 == 48
    lc, dc = R.canonical(ll), R.canonical(dl)
    acc, nbits = P.lz_block_header(ll, dl)
    want, total = Z.assemble(info["stream"], info["tokens"], ll, lc, dl, dc, [(acc >> k) & 1 for k in range(nbits)])
    assert zlib.decompress(want) == info["stream"].tobytes()
    dev = torch.from_numpy(frame[None]).cuda()
    _, adler = P.frame_statistics(dev)
    arrays = [np.array([BASE, BASE + len(want)], np.int64),
              (np.array(lc, np.int64) | (np.array(ll, np.int64) << 16)).astype(np.uint32),
              (np.array(dc, np.int64) | (np.array(dl, np.int64) << 16)).astype(np.uint32),
              np.frombuffer(acc.to_bytes(P.LZ_HEADER_WORDS * 4, "little"), dtype="<u4").astype(np.uint32),
              np.array([nbits], np.int32)]
    blob = torch.from_numpy(np.concatenate([v.view(np.uint8) for v in arrays])).cuda()
    at = np.cumsum([0] + [v.nbytes for v in arrays[:-1]]) + blob.data_ptr()
    size = (BASE + len(want) + PAD + 3) // 4 * 4
    buf = torch.zeros(size, dtype=torch.uint8, device="cuda")
    buf[:BASE] = SENTINEL
    buf[BASE + len(want):] = SENTINEL
    L.spnet_png_lz_pack(dev.data_ptr(), 1, 40, 1024, 1, int(at[1]), int(at[2]), int(at[3]), int(at[4]), int(at[0]),
                        adler.data_ptr(), buf.data_ptr(), size, L.current_stream())
    out = buf.cpu().numpy()
    assert out[BASE:BASE + len(want)].tobytes() == want
    assert zlib.decompress(out[BASE:BASE + len(want)].tobytes()) == info["stream"].tobytes()
    assert (out[:BASE] == SENTINEL).all() and (out[BASE + len(want):] == SENTINEL).all()


def test_public_encoders_and_the_writer(frames, reference, tmp_path):
    from spnet_amd import png as P
    for name in ("period3_7x13", "rgb_3x5", "replicated_16x24x3", "tile_repeat_17000"):
        frame = frames[name]
        other = frame[::-1].copy()
        dev = torch.from_numpy(np.stack([frame, other])).cuda()
        files = P.encode_png_device(dev, lz77=True)
        assert files[0] == R.png_bytes(frame, reference[name][0])
        assert files[1] == R.png_bytes(other, Z.chosen_stream(other)[0])
        assert P.encode_png_device(dev) == [R.png_bytes(f) for f in (frame, other)]          # the default: the old bytes
        paths = [str(tmp_path / ("%s_%d.png" % (name, k))) for k in range(2)]
        sizes = P.write_png_device(dev, paths, threads=2, lz77=True)
        assert [open(p, "rb").read() for p in paths] == files and sizes == [len(f) for f in files]
        assert np.array_equal(np.asarray(Image.open(paths[1])), other)
    empty = torch.empty((0, 4, 4), dtype=torch.uint8, device="cuda")
    assert P.encode_png_device(empty, lz77=True) == [] and P.write_png_device(empty, [], lz77=True) == []
    assert P.zlib_streams_device(empty, lz77=True) == []


def test_entry_points_refuse_bad_arguments():
    _need_gpu()
    from spnet_amd import _lib as L
    src = torch.zeros(64, dtype=torch.uint8, device="cuda")
    words = torch.zeros(1024, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 32], dtype=torch.int64, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    s = L.current_stream()
    p, w, o, q = src.data_ptr(), words.data_ptr(), offs.data_ptr(), out.data_ptr()
    for bad in ((1, 0, 8, 1), (1, 8, 0, 1), (1, 8, 8, 5), (-1, 8, 8, 1), (1, 1 << 14, 1 << 14, 1)):
        with pytest.raises(L.HipError):
            L.spnet_png_lz_scan(p, *bad, w, w, s)
        with pytest.raises(L.HipError):
            L.spnet_png_lz_pack(p, *bad, w, w, w, w, o, w, q, 64, s)
    for args in ((0, 1, 8, 8, 1, w, w), (p, 1, 8, 8, 1, 0, w), (p, 1, 8, 8, 1, w, 0), (p, 1, 8, 8, 1, w + 1, w),
                 (p, 1, 8, 8, 1, w, w + 2)):
        with pytest.raises(L.HipError):
            L.spnet_png_lz_scan(*args, s)                                     # null or misaligned
    good = [p, 1, 8, 8, 1, w, w, w, w, o, w, q, 64]
    for k, v in ((0, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 0), (5, w + 1), (6, w + 2), (7, w + 1), (8, w + 3),
                 (9, o + 4), (10, w + 1), (11, q + 1), (12, 62), (12, -4)):
        args = list(good)
        args[k] = v
        with pytest.raises(L.HipError):
            L.spnet_png_lz_pack(*args, s)
    L.spnet_png_lz_scan(p, 0, 8, 8, 1, w, w, s)                               # empty batch: nothing to do
    L.spnet_png_lz_pack(p, 0, 8, 8, 1, w, w, w, w, o, w, q, 64, s)
    # a slot that is too small for its stream is cut off at the slot's end, never written past it
    from spnet_amd import png as P
    frame = torch.zeros((1, 64, 64), dtype=torch.uint8, device="cuda")
    hist, adler = P.frame_statistics(frame)
    plan = P.plan_frames_lz(hist, *P.lz_statistics(frame))
    assert plan["use_lz"][0] and plan["offsets"][1] > 20
    plan["offsets"][1] = 20
    buf = torch.zeros(128, dtype=torch.uint8, device="cuda")
    buf[20:] = SENTINEL
    P.pack_frames_lz(frame, plan, adler, out=buf)
    got = buf.cpu().numpy()
    assert (got[20:] == SENTINEL).all() and got[0] == 0x78 and got[1] == 0x01


def test_gen_fake_espi_command_line_with_device_png_lz(tmp_path):
    """Five frames by `gen_fake_espi.py --device_png_lz`, run as a command (a fresh child process), against the default
    writer's files: the same labels and, file by file, the same pixels."""
    _need_gpu()
    import subprocess
    import sys
    import gen_fake_espi as G
    host, dev = str(tmp_path / "host"), str(tmp_path / "lz")
    rows_h = G.gen_dataset(datapath=host, numframes=5, seed=6)
    root = os.path.dirname(os.path.abspath(G.__file__))
    done = subprocess.run([sys.executable, os.path.join(root, "gen_fake_espi.py"), "-d", dev, "-n", "5", "--seed", "6",
                           "--device_png_lz"], cwd=root, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    for k in range(5):
        stem = "steelpan_" + str(k).zfill(7) + ".csv"
        assert open(os.path.join(host, "Train", stem)).read() == open(os.path.join(dev, "Train", stem)).read()
    assert len(rows_h) == 5
    names = sorted(f for f in os.listdir(os.path.join(host, "Train")) if f.endswith(".png"))
    assert len(names) == 5 and names == sorted(f for f in os.listdir(os.path.join(dev, "Train")) if f.endswith(".png"))
    for f in names:
        a = np.asarray(Image.open(os.path.join(host, "Train", f)))
        b = np.asarray(Image.open(os.path.join(dev, "Train", f)))
        assert a.shape == (384, 512) and np.array_equal(a, b), f


def test_show_pred_ellipses_accepts_device_lz(frames, tmp_path):
    from spnet_amd import config as cf
    from spnet_amd import utils
    src = str(tmp_path / "frame.png")
    Image.fromarray(frames["espi_384x512"]).save(src)
    v = cf.vars_per_pred
    Yp = np.zeros((1, 4 * v), np.float32)
    Yp[:, 6::v] = 1.0
    Yp[0, 0:8] = (150, 120, 60, 35, 1.0, 0.0, 0, 3.4)
    pix = {}
    for mode in ("host", "device", "device-lz"):
        d = str(tmp_path / mode)
        os.makedirs(d)
        utils.show_pred_ellipses(Yp.copy(), Yp, [src], num_draw=1, log_dir=d, png=mode)
        path = os.path.join(d, "steelpan_pred_00000.png")
        pix[mode] = (np.asarray(Image.open(path)), os.path.getsize(path))
    assert np.array_equal(pix["host"][0], pix["device"][0]) and np.array_equal(pix["host"][0], pix["device-lz"][0])
    assert pix["device-lz"][1] < pix["device"][1]                             # grey replicated into RGB: the matches pay
