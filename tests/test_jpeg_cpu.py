"""The host side of the JPEG / Motion-JPEG writer (spnet_amd/jpeg.py) and the numpy restatement the device is held to
(tests/helpers/jpeg_ref.py), without a GPU: Pillow reads what the reference encoder writes, the tables are libjpeg's, the
quality is Pillow's own encoder's, the quantiser's reciprocal is the division, the 32-bit sums cannot overflow, and the AVI
container has the RIFF layout its readers expect."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

from spnet_amd import jpeg as J
from tests.helpers import jpeg_ref as R


def _segments(data, marker):
    """The payloads of every `marker` segment before the scan."""
    pos, out = 2, []
    while pos < len(data):
        assert data[pos] == 0xFF
        m, size = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if m == marker:
            out.append(data[pos + 4:pos + 2 + size])
        if m == 0xDA:
            break
        pos += 2 + size
    return b"".join(out)


def _tables_as_pillow(got):
    """Pillow's `quantization` as natural-order lists: releases before 8.3 return the tables in zigzag order."""
    tabs = [list(got[k]) for k in sorted(got)]
    probe = io.BytesIO()
    Image.new("L", (8, 8)).save(probe, "JPEG", quality=50)            # quality 50: the Annex K base table itself
    first = list(Image.open(io.BytesIO(probe.getvalue())).quantization[0])
    if first == list(J.LUMINANCE_BASE):
        return tabs
    assert first == [J.LUMINANCE_BASE[k] for k in J.ZIGZAG]
    return [[t[J.ZIGZAG.index(k)] for k in range(64)] for t in tabs]


def _pillow_encode(frame, quality):
    """Pillow's encoder with our tables, 4:4:4; the DQT bytes are checked, so the table order it was given is right."""
    qt = J.quant_tables(quality)
    ours = _segments(J.jpeg_header(8, 8, 3, quality), 0xDB)
    n = 1 if frame.ndim == 2 else 2
    for order in (range(64), J.ZIGZAG):
        buf = io.BytesIO()
        Image.fromarray(frame).save(buf, "JPEG", qtables=[[int(qt[t][k]) for k in order] for t in range(n)], subsampling=0)
        if _segments(buf.getvalue(), 0xDB) == ours[:65 * n]:
            return buf.getvalue()
    raise AssertionError("Pillow did not write the tables it was given")


def _psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / np.mean(d * d))


def _quality_frames():
    rng = np.random.default_rng(5)
    grey = rng.integers(0, 256, (40, 48), dtype=np.uint8)                                   # 48 x 40
    yy, xx = np.mgrid[0:29, 0:37]
    rgb = np.clip(np.stack([xx * 6, yy * 8, (xx + yy) * 3], 2) + rng.integers(-12, 13, (29, 37, 3)), 0, 255).astype(np.uint8)
    return dict(grey=grey, rgb=rgb)


# ----------------------------------------------------------------------------- tables and header
def test_zigzag_and_huffman_tables_are_the_standards():
    assert sorted(J.ZIGZAG) == list(range(64)) and J.ZIGZAG[:6] == (0, 1, 8, 16, 9, 2) and J.ZIGZAG[-3:] == (55, 62, 63)
    for _, _, (bits, vals) in J.HUFFMAN_TABLES:
        assert sum(bits) == len(vals) == len(set(vals))
        codes = J.huffman_codes((bits, vals))
        assert sum(1 << (16 - n) for _, n in codes.values()) < (1 << 16)            # a prefix code, all-ones unused
    # libjpeg writes the same four tables when it is not asked to optimise them
    buf = io.BytesIO()
    Image.new("RGB", (8, 8)).save(buf, "JPEG", quality=50, subsampling=0)
    want, got = _segments(buf.getvalue(), 0xC4), _segments(J.jpeg_header(8, 8, 3, 50), 0xC4)

    def split(x):
        out, i = {}, 0
        while i < len(x):
            n = sum(x[i + 1:i + 17])
            out[x[i]] = x[i + 1:i + 17 + n]
            i += 17 + n
        return out
    assert split(want) == split(got) and sorted(split(got)) == [0x00, 0x01, 0x10, 0x11]


@pytest.mark.parametrize("quality", [1, 50, 90, 100])
def test_quant_tables_are_libjpegs(quality):
    qt = J.quant_tables(quality)
    assert qt.shape == (2, 64) and qt.min() >= 1 and qt.max() <= 255
    want = Image.new("RGB", (8, 8))
    buf = io.BytesIO()
    want.save(buf, "JPEG", quality=quality, subsampling=0)
    mine = _tables_as_pillow(Image.open(io.BytesIO(buf.getvalue())).quantization)
    assert mine == [list(qt[0]), list(qt[1])]                                       # Pillow's own tables at this quality
    # and Pillow reads them back from what the reference encoder writes
    rng = np.random.default_rng(quality)
    for frame in (rng.integers(0, 256, (9, 17), dtype=np.uint8), rng.integers(0, 256, (9, 17, 3), dtype=np.uint8)):
        im = Image.open(io.BytesIO(R.encode_jpeg(frame, quality)))
        im.load()
        got = _tables_as_pillow(im.quantization)
        assert got == [list(qt[t]) for t in range(len(got))] and len(got) == (1 if frame.ndim == 2 else 2)
    if quality == 50:
        assert list(qt[0]) == list(J.LUMINANCE_BASE) and list(qt[1]) == list(J.CHROMINANCE_BASE)
    for bad in (0, 101, 50.5):
        with pytest.raises(ValueError):
            J.quant_tables(bad)


def test_header_segments():
    h = J.jpeg_header(21, 13, 3, 90)
    assert h[:4] == b"\xff\xd8\xff\xe0" and h[6:11] == b"JFIF\x00"
    assert _segments(h, 0xC0) == struct.pack(">BHHB", 8, 13, 21, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])     # true size
    assert _segments(h, 0xDD) == struct.pack(">H", 3) == struct.pack(">H", J.restart_interval(21, 3))
    assert _segments(J.jpeg_header(520, 8, 1, 90), 0xDD) == struct.pack(">H", 64)
    assert _segments(J.jpeg_header(520, 8, 1, 90, restart_interval=5), 0xDD) == struct.pack(">H", 5)
    assert h[-14:] == b"\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00"
    g = J.jpeg_header(21, 13, 1, 90)
    assert len(_segments(g, 0xDB)) == 65 and g[-10:] == b"\xff\xda\x00\x08\x01\x01\x00\x00\x3f\x00"
    for bad in ((0, 8, 1), (8, 65536, 1), (8, 8, 2), (8, 8, 4)):
        with pytest.raises(ValueError):
            J.jpeg_header(*bad)
    assert J.JPEG_TRAILER == b"\xff\xd9"


def test_interval_rule_is_the_librarys():
    """restart_interval / intervals of jpeg.py, of the reference and of the library's queries (no GPU needed) agree."""
    from spnet_amd import _lib as L
    for H, W in ((8, 8), (13, 21), (8, 520), (72, 8), (384, 512), (1, 1), (65535, 65535), (9, 513), (16, 512)):
        for c in (1, 3):
            assert L.spnet_jpeg_restart_interval(W, c) == J.restart_interval(W, c) == R.restart_interval(W)
            assert L.spnet_jpeg_intervals(H, W, c) == J.intervals(H, W, c)
    assert J.restart_interval(520) == 64 and J.intervals(8, 520) == 2 and J.intervals(72, 8) == 9
    for bad in ((0, 8, 1), (8, 0, 1), (65536, 8, 1), (8, 65536, 3), (8, 8, 2), (8, 8, 4)):
        assert L.spnet_jpeg_intervals(*bad) == -1


# ----------------------------------------------------------------------------- the reference encoder against Pillow
@pytest.mark.parametrize("shape", [(8, 8), (16, 24), (13, 21, 3), (8, 520), (72, 8), (29, 37, 3)])
def test_pillow_opens_the_reference_encoders_files(shape):
    rng = np.random.default_rng(sum(shape))
    frame = rng.integers(0, 256, shape, dtype=np.uint8)
    data = R.encode_jpeg(frame, 90)
    scan, sizes, _ = R.encode_scan(frame, 90)
    assert len(sizes) == J.intervals(shape[0], shape[1]) and len(scan) == int(sizes.sum()) + 2 * (len(sizes) - 1)
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.mode == ("L" if len(shape) == 2 else "RGB") and im.size == (shape[1], shape[0])
    assert _psnr(np.asarray(im), frame) > 20            # noise at quality 90: the picture, not garbage after a marker


def test_constant_grey_decodes_exactly():
    for frame in (np.full((16, 24), 128, np.uint8), np.full((13, 21, 3), 128, np.uint8)):
        scan, _, stats = R.encode_scan(frame, 90)
        assert stats["eob"] == (2 * 3 if frame.ndim == 2 else 2 * 3 * 3) and stats["ac_category"] == 0      # EOB-only blocks
        im = Image.open(io.BytesIO(R.encode_jpeg(frame, 90)))
        assert (np.asarray(im) == 128).all()


MARGIN_DB = 0.033


@pytest.mark.parametrize("name", ["grey", "rgb"])
@pytest.mark.parametrize("quality", [75, 90])
def test_quality_is_pillows_own(name, quality):
    """PSNR against the source of (a) the reference encoder's bytes and (b) Pillow's encoder's bytes at the same tables and
    4:4:4, both decoded by Pillow: (a) >= (b) - MARGIN_DB.  The two differ in DCT (and colour) rounding only.  Measured
    (b) - (a): grey 48 x 40 noise +0.0021 dB at 75, -0.0069 at 90; RGB 37 x 29 gradient + noise -0.0069 at 75, +0.0129 at
    90.  The margin is the largest measured gap, 0.013 dB, plus 0.02 dB; a gap above 0.1 dB would be a DCT bug."""
    frame = _quality_frames()[name]
    ours = np.asarray(Image.open(io.BytesIO(R.encode_jpeg(frame, quality))))
    theirs = np.asarray(Image.open(io.BytesIO(_pillow_encode(frame, quality))))
    a, b = _psnr(ours, frame), _psnr(theirs, frame)
    print("%s q%d: ours %.4f dB, Pillow %.4f dB, gap %.4f dB" % (name, quality, a, b, b - a))
    assert a >= b - MARGIN_DB


# ----------------------------------------------------------------------------- arithmetic
def test_reciprocal_is_the_division():
    """The kernel divides by 2Q with (n * ceil(2^24 / 2Q)) >> 24.  Exhaustive over what can reach it: every numerator
    n = (|q| >> 14) + Q with |q| < 2^25 (the bound of the column sums; the check runs to 2^14, past it) and every Q 1 ..
    255.  That ((|q| >> 14) + Q) // 2Q is the definition (|q| + (Q << 14)) // (Q << 15) is exhaustive over |q| < 2^25 too:
    both are non-decreasing step functions of |q|, so they are equal everywhere once they agree on both sides of every
    step of the definition and at the ends."""
    n = np.arange(1 << 14, dtype=np.int64)
    top = (1 << 25) - 1
    for Q in range(1, 256):
        m = 0xFFFFFF // (2 * Q) + 1
        assert m == -(-(1 << 24) // (2 * Q)) and m < (1 << 24)                   # ceil; fits the entry's 24 bits
        assert ((n * m) >> 24 == n // (2 * Q)).all()
        assert (n << 8).max() < (1 << 32) and int(n.max()) * m < (1 << 38)        # __umulhi(n << 8, m): no lost bit
        steps = np.arange(1, top // (Q << 15) + 2, dtype=np.int64) * (Q << 15) - (Q << 14)           # value becomes c at these
        pts = np.unique(np.clip(np.concatenate([steps - 1, steps, [0, top]]), 0, top))
        assert ((pts + (Q << 14)) // (Q << 15) == ((pts >> 14) + Q) // (2 * Q)).all()
    q = np.arange(1 << 20, dtype=np.int64)                                        # and point by point at the low end
    for Q in (1, 2, 3, 16, 99, 255):
        assert ((q + (Q << 14)) // (Q << 15) == ((q >> 14) + Q) // (2 * Q)).all()


def test_sums_stay_inside_32_bits():
    """The extreme blocks: the 0/255 checkerboard and its transpose (largest alternating sums), all-0 and all-255 (largest
    sums of all: row 0 of K has the largest absolute sum, 8 * 1448 = 11584)."""
    assert np.abs(R.K).sum(axis=1).max() == 11584 and np.abs(R.K).max() == 2009
    board = ((np.indices((8, 8)).sum(0) & 1) * 255).astype(np.uint8)
    info = {}
    for block in (board, board.T.copy(), 255 - board, np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8)):
        coef = R.frame_coefficients(block, 100, info).reshape(64)
        assert abs(int(coef[0])) <= 1024 and np.abs(coef[1:]).max() <= 1023       # categories 11 (as a difference) and 10
    assert info["rows"] <= 11584 * 128 < (1 << 21)
    assert info["p"] <= 2896
    assert info["q"] <= 11584 * 2896 < (1 << 25)
    assert info == dict(rows=1482752, p=2896, q=33547264)                         # reached by the all-0 block
    # the colour transform: sums of a row of constants, 8-bit samples
    assert 19595 + 38470 + 7471 == 65536 and -11059 - 21709 + 32768 == 0 and 32768 - 27439 - 5329 == 0
    assert 32768 * 255 + 8421375 < (1 << 31) and -(11059 + 21709) * 255 + 8421375 >= 0
    ycc = R.components(np.array([[[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]]], np.uint8))
    assert ycc[:, 0, 0].tolist() == [255, 128, 128] and ycc[:, 0, 1].tolist() == [0, 128, 128]
    assert ycc[:, 0, 2].tolist() == [76, 85, 255] and ycc[:, 0, 3].tolist() == [29, 255, 107]


def test_reference_exercises_zrl_stuffing_and_restart_wrap():
    rng = np.random.default_rng(11)
    _, _, stats = R.encode_scan(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8), 100)
    assert stats["stuffed"] > 0
    yy, xx = np.mgrid[0:16, 0:24]
    _, _, stats = R.encode_scan(((5 * xx + 15 * yy) & 255).astype(np.uint8), 10)
    assert stats["zrl"] > 0
    scan, sizes, _ = R.encode_scan(rng.integers(0, 256, (72, 8), dtype=np.uint8), 90)
    at, marks = 0, []
    for s in sizes[:-1]:
        at += int(s)
        marks.append(scan[at:at + 2])
        at += 2
    assert marks == [bytes([0xFF, 0xD0 + (k & 7)]) for k in range(8)] and at + int(sizes[-1]) == len(scan)


# ----------------------------------------------------------------------------- the movie container
def _fake_files(frames):
    """One 'JPEG file' per frame whose bytes name the frame: odd and even lengths."""
    return [b"\xff\xd8" + bytes([int(f.flat[0])]) * (5 + int(f.flat[0])) + b"\xff\xd9" for f in frames]


def test_mjpeg_writer_layout(tmp_path):
    path = str(tmp_path / "m.avi")
    calls = []

    def encoder(frames):
        calls.append(len(frames))
        return _fake_files(frames)

    frames = np.zeros((5, 6, 10, 3), np.uint8)
    frames[:, 0, 0, 0] = [1, 2, 3, 4, 5]
    with J.MjpegWriter(path, 10, 6, fps=12.5, encoder=encoder) as w:
        w.add(frames[:2])
        w.add(frames[2:])
        w.add(frames[:0])
        assert w.frames == 5
    assert calls == [2, 3] and w.closed
    data = open(path, "rb").read()
    avi = R.parse_avi(data)                                       # walks every chunk: each size inside its parent
    files = _fake_files(frames)
    assert avi["frames"] == files and {len(f) & 1 for f in files} == {0, 1}
    assert avi["total_frames"] == 5 and avi["length"] == 5 and avi["streams"] == 1 and avi["flags"] & 0x10
    assert (avi["width"], avi["height"], avi["bi_width"], avi["bi_height"]) == (10, 6, 10, 6)
    assert avi["fcc_type"] == b"vids" and avi["handler"] == b"MJPG" and avi["compression"] == b"MJPG"
    assert (avi["bi_size"], avi["bi_bits"]) == (40, 24)
    assert (avi["rate"], avi["scale"]) == (25, 2) and avi["usec_per_frame"] == 80000
    assert struct.unpack("<I", data[4:8])[0] == len(data) - 8
    assert len(avi["index"]) == 5
    for (tag, flags, off, length), f, at in zip(avi["index"], files, avi["chunk_at"]):
        assert tag == b"00dc" and flags == 0x10 and avi["movi_tag"] + off == at and at % 2 == 0
        assert data[at:at + 4] == b"00dc" and struct.unpack("<I", data[at + 4:at + 8])[0] == length == len(f)
        assert data[at + 8:at + 8 + length] == f
        if length & 1:
            assert data[at + 8 + length] == 0                      # padded to even length
    # an empty movie is a valid file too
    with J.MjpegWriter(str(tmp_path / "e.avi"), 10, 6, encoder=encoder) as e:
        pass
    empty = R.parse_avi(open(str(tmp_path / "e.avi"), "rb").read())
    assert empty["frames"] == [] and empty["total_frames"] == 0 and (empty["rate"], empty["scale"]) == (5, 1)


def test_mjpeg_writer_refuses(tmp_path):
    w = J.MjpegWriter(str(tmp_path / "m.avi"), 10, 6, encoder=_fake_files)
    for bad in (np.zeros((1, 6, 11, 3), np.uint8), np.zeros((1, 7, 10, 3), np.uint8), np.zeros((1, 6, 10), np.uint8),
                np.zeros((6, 10, 3), np.uint8)):
        with pytest.raises(ValueError):
            w.add(bad)
    w.add(np.zeros((1, 6, 10, 3), np.uint8))
    before = (w.frames, w._size)
    w._size = J.RIFF_LIMIT - 40                                    # as if 2 GiB had been written
    with pytest.raises(ValueError, match="2 GiB"):
        w.add(np.zeros((1, 6, 10, 3), np.uint8))
    assert w.frames == before[0]                                   # nothing of the refused call was written
    w._size = before[1]
    w.close()
    w.close()
    with pytest.raises(ValueError):
        w.add(np.zeros((1, 6, 10, 3), np.uint8))
    assert R.parse_avi(open(str(tmp_path / "m.avi"), "rb").read())["total_frames"] == 1
    for bad in (dict(channels=2), dict(fps=0), dict(fps=-1.0)):
        with pytest.raises(ValueError):
            J.MjpegWriter(str(tmp_path / "x.avi"), 10, 6, encoder=_fake_files, **bad)
    with pytest.raises(ValueError):
        J.MjpegWriter(str(tmp_path / "x.avi"), 0, 6)


def test_device_entry_points_need_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        J.encode_jpeg_device(torch.zeros((1, 8, 8), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        J.write_jpeg_device(torch.zeros((1, 8, 8), dtype=torch.uint8), ["x.jpg"])
