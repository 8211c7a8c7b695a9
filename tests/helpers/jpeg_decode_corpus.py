"""The JPEG files the decoder tests share (tests/test_jpeg_decode_cpu.py, tests/test_jpeg_decode_gpu.py), built in memory:
files of this project's encoder (tests/helpers/jpeg_ref.py restates it byte for byte) and of Pillow / libjpeg with custom
Huffman tables, every chroma subsampling, restart markers per MCU row, every two MCUs and none; damaged files; files the
device leaves to the host."""
import io
from collections import namedtuple

import numpy as np
from PIL import Image

from spnet_amd import jpeg as J
from tests.helpers import jpeg_ref

Case = namedtuple("Case", "name data shape")           # shape: (H, W) grey, (H, W, 3) colour

SHAPES = ((19, 37), (8, 8), (24, 40, 3), (17, 70, 3))
QUALITIES = (10, 50, 90, 100)
PILLOW_OPTIONS = (("plain", {}), ("optimize", dict(optimize=True)), ("rst_rows", dict(restart_marker_rows=1)),
                  ("rst_blocks", dict(restart_marker_blocks=2)))


def content(kind, shape, seed=0):
    """noise; ramp: a ramp that wraps at 256 (sharp edges far from DC: runs of 16 zeros, ZRL); flat: DC only."""
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if kind == "flat":
        return np.full(shape, 77, np.uint8)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    a = ((5 * xx + 15 * yy) & 255).astype(np.uint8)
    return a if len(shape) == 2 else np.stack([a, a[::-1], ((3 * xx + 7 * yy) & 255).astype(np.uint8)], axis=-1)


def pillow_jpeg(frame, **options):
    b = io.BytesIO()
    Image.fromarray(frame).save(b, "JPEG", **options)
    return b.getvalue()


def pillow_pixels(data):
    """What the default path sees: [H][W][C]."""
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a.reshape(a.shape[0], a.shape[1], -1)


def build(shapes=SHAPES):
    cases = []
    for shape in shapes:
        tag = "x".join(str(v) for v in shape)
        for kind in ("noise", "ramp", "flat"):
            frame = content(kind, shape)
            for q in QUALITIES:
                cases.append(Case("%s-%s-q%d-ours" % (tag, kind, q), jpeg_ref.encode_jpeg(frame, q), shape))
                for oname, options in PILLOW_OPTIONS:
                    for sub in ((0, 1, 2) if len(shape) == 3 else (None,)):
                        kw = dict(options, quality=q)
                        if sub is not None:
                            kw["subsampling"] = sub
                        cases.append(Case("%s-%s-q%d-pillow-%s-s%s" % (tag, kind, q, oname, sub), pillow_jpeg(frame, **kw),
                                          shape))
    return cases


_CORPUS = []


def corpus():
    """Built once per process, never changed."""
    if not _CORPUS:
        _CORPUS.extend(build())
    return _CORPUS


def expected(cases):
    """name -> Pillow's pixels [H][W][C]; computed once per call."""
    return {c.name: pillow_pixels(c.data) for c in cases}


# ----------------------------------------------------------------------------- files the device leaves to the host
def progressive(frame):
    return pillow_jpeg(frame, quality=90, progressive=True)


def cmyk(shape=(16, 24)):
    b = io.BytesIO()
    Image.fromarray(content("noise", shape + (4,), 3), "CMYK").save(b, "JPEG", quality=90)
    return b.getvalue()


def adobe_rgb(frame):
    """A three-component file whose Adobe APP14 segment says "no transform" (the components ARE R, G, B): the 4:4:4 file of
    Pillow with that segment put in front of its tables and JFIF's APP0 taken out."""
    data = pillow_jpeg(frame, quality=90, subsampling=0)
    assert data[2:4] == b"\xff\xe0"
    skip = 4 + (data[4] << 8 | data[5])
    app14 = b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00"
    return data[:2] + app14 + data[skip:]


def without_dht(data):
    """The file with its DHT segments cut out (a Motion-JPEG frame that relies on the Annex K tables)."""
    out, pos = bytearray(data[:2]), 2
    while True:
        m = data[pos + 1]
        length = data[pos + 2] << 8 | data[pos + 3]
        if m != 0xC4:
            out += data[pos:pos + 2 + length]
        pos += 2 + length
        if m == 0xDA:
            return bytes(out) + data[pos:]


def segment_boundaries(data):
    """Positions where a segment of the header starts or ends, up to the first byte of the scan."""
    cuts, pos = [0, 1, 2], 2
    while True:
        m = data[pos + 1]
        length = data[pos + 2] << 8 | data[pos + 3]
        cuts += [pos + 1, pos + 2, pos + 3, pos + 4, pos + 2 + length]
        pos += 2 + length
        if m == 0xDA:
            return sorted(set(cuts))


# ----------------------------------------------------------------------------- damaged files the device meets
def damaged(shape=(40, 64)):
    """name -> (file, a sound file of the same size): every file still parses as one the device takes, so the DEVICE has
    to notice.  flipped: one payload byte in the middle of an interval; cut: scan data cut short, EOI kept; unassigned: a
    DHT from which the code of a symbol the scan uses was taken away."""
    frame = content("noise", shape, 5)
    sound = jpeg_ref.encode_jpeg(frame, 90)
    info = J.parse_jpeg(sound)
    lo, hi = (int(v) for v in info.bounds[2])
    flipped = bytearray(sound)
    flipped[lo + 3] ^= 0x5A
    last_lo, last_hi = (int(v) for v in info.bounds[-1])
    cut = sound[:last_lo + (last_hi - last_lo) // 2] + b"\xff\xd9"
    # the AC table of the file, with EOB's code taken away
    at = sound.index(b"\xff\xc4")
    length = sound[at + 2] << 8 | sound[at + 3]
    body = bytearray(sound[at + 4:at + 2 + length])
    k = 0
    while body[k] != 0x10:                                   # class 1 (AC), table 0
        k += 17 + sum(body[k + 1:k + 17])
    count = sum(body[k + 1:k + 17])
    symbols = list(body[k + 17:k + 17 + count])
    used = symbols.index(0x00)                               # EOB: every block of noise at q90 that ends early uses it
    bits = list(body[k + 1:k + 17])
    # one code fewer of EOB's length: the codes after it move up, and the pattern of the last one stands for nothing
    sizes = [l + 1 for l in range(16) for _ in range(bits[l])]
    bits[sizes[used] - 1] -= 1
    del symbols[used]
    new_body = bytes(body[:k + 1]) + bytes(bits) + bytes(symbols) + bytes(body[k + 17 + count:])
    unassigned = sound[:at] + b"\xff\xc4" + bytes([(len(new_body) + 2) >> 8, (len(new_body) + 2) & 255]) + new_body + \
        sound[at + 2 + length:]
    return dict(flipped=bytes(flipped), cut=cut, unassigned=unassigned), sound
