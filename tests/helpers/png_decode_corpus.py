"""The PNG files the decoder tests read (tests/test_png_decode_cpu.py, tests/test_png_decode_gpu.py), generated with zlib,
numpy and Pillow at test time: nothing is committed but this code.  Every deflate block type, far and overlapping
matches, every filter type at every bytes-per-pixel, container oddities, formats that only the host decodes, and
malformed streams derived from good ones.

A file is a Case: name, data (the PNG bytes), shape (H, W, C) of the pixels, and for malformed ones `expect`, the set of
inflate::Status values (spnet_amd/csrc/inflate_core.h) the zlib stream may end with.
"""
import io
import struct
import zlib
from collections import namedtuple

import numpy as np
from PIL import Image

from spnet_amd import png as P

Case = namedtuple("Case", "name data shape expect")
OK, BAD_HEADER, BAD_BLOCK_TYPE, BAD_STORED_LEN, BAD_CODE, BAD_SYMBOL, BAD_DISTANCE, INPUT_EXHAUSTED, OUTPUT_OVERFLOW, \
    OUTPUT_SHORT, BAD_ADLER, BAD_FILTER = range(12)


# ----------------------------------------------------------------------------- filtering and the container
def filter_stream(img, ftypes):
    """PNG's scanline stream of img uint8 [H,W,C] with filter type ftypes[y] on row y (PNG specification, section 9)."""
    img = np.asarray(img, np.uint8)
    H, W, C = img.shape
    raw = img.reshape(H, W * C).astype(np.int32)
    up = np.vstack([np.zeros((1, W * C), np.int32), raw[:-1]])
    left = np.hstack([np.zeros((H, C), np.int32), raw[:, :-C]]) if W > 1 else np.zeros_like(raw)
    upleft = np.hstack([np.zeros((H, C), np.int32), up[:, :-C]]) if W > 1 else np.zeros_like(raw)
    p = left + up - upleft
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
    pred = [np.zeros_like(raw), left, up, (left + up) >> 1, paeth]
    out = np.zeros((H, 1 + W * C), np.uint8)
    for y in range(H):
        out[y, 0] = ftypes[y]
        out[y, 1:] = (raw[y] - pred[ftypes[y] if ftypes[y] < 5 else 0][y]) & 255
    return out.tobytes()


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(data) + c.flush()


def container(zstream, shape, cuts=None, before_idat=(), colour_type=None, bit_depth=8, interlace=0):
    """A PNG file around zstream, its IDAT data cut at the positions `cuts` (a chunk per piece, empty pieces included)."""
    H, W, C = shape
    ct = P.COLOUR_TYPE[C] if colour_type is None else colour_type
    out = [P.PNG_SIGNATURE, P._chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, ct, 0, 0, interlace))]
    out += [P._chunk(tag, body) for tag, body in before_idat]
    edges = [0] + sorted(cuts or []) + [len(zstream)]
    out += [P._chunk(b"IDAT", zstream[a:b]) for a, b in zip(edges[:-1], edges[1:])]
    out.append(P._chunk(b"IEND", b""))
    return b"".join(out)


def png_of(img, ftypes=None, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    ftypes = [0] * img.shape[0] if ftypes is None else ftypes
    return container(deflate(filter_stream(img, ftypes), level, strategy), img.shape)


# ----------------------------------------------------------------------------- images
def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def smooth(shape, seed=0):
    H, W, C = shape
    y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
    return ((x * 3 + y * 5 + c * 40 + seed) % 256).astype(np.uint8)


def textured(shape, seed):
    """Compressible, but not trivially: a ramp plus two bits of noise (matches and literals in every block)."""
    return ((smooth(shape, seed).astype(np.int32) + np.random.default_rng(seed).integers(0, 4, shape)) % 256).astype(np.uint8)


# ----------------------------------------------------------------------------- good files
BLOCK_SHAPE = (300, 256, 1)      # 300 * 257 = 77,100 bytes: more than one stored block
FAR_SHAPE = (130, 255, 1)        # rows of 256 stream bytes
FILTER_SHAPES = [(1, 1), (1, 9), (9, 1), (3, 513), (17, 31)]
SMALL = (17, 31, 3)


def block_type_files():
    shape = BLOCK_SHAPE
    n, s, t = noise(shape, 1), smooth(shape), textured(shape, 2)
    zeros = [0] * shape[0]
    runs = np.repeat(noise((shape[0], shape[1] // 8, 1), 3), 8, axis=1)        # runs of 8 equal bytes: Z_RLE matches
    cases = [("stored", deflate(filter_stream(n, zeros), 0)),
             ("fixed", deflate(filter_stream(t, zeros), 6, zlib.Z_FIXED)),
             ("huffman_only", deflate(filter_stream(n, zeros), 6, zlib.Z_HUFFMAN_ONLY)),
             ("rle", deflate(filter_stream(runs, zeros), 6, zlib.Z_RLE)),
             ("level9_smooth", deflate(filter_stream(s, zeros), 9)),
             ("level6_noise", deflate(filter_stream(n, zeros), 6)),
             ("level1_sub", deflate(filter_stream(t, [1] * shape[0]), 1))]
    stream = filter_stream(t, zeros)
    c = zlib.compressobj(6)
    parts = []
    for i in range(0, len(stream), 1000):
        parts += [c.compress(stream[i:i + 1000]), c.flush(zlib.Z_FULL_FLUSH)]
    cases.append(("full_flush", b"".join(parts) + c.flush()))
    assert len(filter_stream(n, zeros)) > 65535 and cases[0][1].count(b"\xff\xff\x00\x00") >= 1
    return [Case("block_" + name, container(z, shape), shape, None) for name, z in cases]


def far_match_file():
    """Rows 125 .. 129 repeat rows 0 .. 4 of random bytes: matches 125 * 256 = 32,000 bytes back.  zlib has emitted them
    if the five repeated rows cost far less than five rows of noise."""
    shape = FAR_SHAPE
    img = noise(shape, 5)
    img[125:130] = img[0:5]
    stream = filter_stream(img, [0] * shape[0])
    z = deflate(stream, 9)
    alone = deflate(stream[:125 * 256], 9)
    assert len(z) - len(alone) < 200, "zlib emitted no far matches (%d bytes for five repeated rows)" % (len(z) - len(alone))
    return Case("far_matches", container(z, shape), shape, None)


def window_edge_file():
    """Matches at the far edge of the window, which zlib never emits (its longest distance is 32,506): a stored block of
    32,768 bytes, then a fixed-Huffman block of three matches -- 258 bytes at distance 32,767, 258 at 32,600 and 252 at
    32,768.  In a 32 KiB ring the bytes such a match writes land on the slots of bytes it has yet to read."""
    shape = (131, 255, 1)
    head = bytearray(noise((32768,), 9).tobytes())
    head[::256] = bytes(128)                                   # the filter bytes of rows 0 .. 127
    head[1] = head[257] = head[680] = 0                        # copied onto the filter bytes of rows 128, 129, 130
    w = BitWriter()
    w.put(1, 1), w.put(1, 2)
    want = bytearray(head)
    for length, dist in ((258, 32767), (258, 32600), (252, 32768)):
        if length == 258:
            w.code(0xC5, 8)                                    # symbol 285
        else:
            w.code(0xC4, 8), w.put(length - 227, 5)            # symbol 284: 227 .. 257
        w.code(29, 5), w.put(dist - 24577, 13)
        for _ in range(length):
            want.append(want[-dist])
    w.code(0, 7)
    z = b"\x78\x01" + b"\x00" + struct.pack("<HH", 32768 & 0xffff, 32768 ^ 0xffff) + bytes(head) + w.bytes() \
        + struct.pack(">I", zlib.adler32(bytes(want)))
    assert zlib.decompress(z) == bytes(want) and len(want) == shape[0] * 256 and max(want[::256]) == 0
    return Case("window_edge_matches", container(z, shape), shape, None)


def filter_files():
    out = []
    for hw in FILTER_SHAPES:
        for C in (1, 2, 3, 4):
            shape = hw + (C,)
            img = textured(shape, 10 * C + hw[0])
            rng = np.random.default_rng(hw[1] + C)
            for ft in range(5):
                out.append(Case("filter%d_%dx%dx%d" % ((ft,) + shape), png_of(img, [ft] * hw[0]), shape, None))
            out.append(Case("filtermix_%dx%dx%d" % shape, png_of(img, [int(v) for v in rng.integers(0, 5, hw[0])]), shape, None))
    return out


def container_files():
    shape = SMALL
    img = textured(shape, 7)
    z = deflate(filter_stream(img, [4] * shape[0]), 6)
    rng = np.random.default_rng(11)
    text = [(b"tEXt", b"Comment\x00made for a test"), (b"gAMA", struct.pack(">I", 45455))]
    return [Case("idat_every_byte", container(z, shape, cuts=list(range(1, len(z)))), shape, None),
            Case("idat_random_cuts", container(z, shape, cuts=[int(v) for v in rng.integers(1, len(z), 7)]), shape, None),
            Case("ancillary_chunks", container(z, shape, before_idat=text), shape, None),
            Case("empty_idat", container(z, shape, cuts=[0, 5, 5]), shape, None)]


def pillow_files():
    """Files as Pillow writes them (its adaptive filter choice), every colour type the device takes."""
    out = []
    for C, mode in ((1, "L"), (2, "LA"), (3, "RGB"), (4, "RGBA")):
        shape = (17, 31, C)
        img = textured(shape, 20 + C)
        buf = io.BytesIO()
        Image.fromarray(img[:, :, 0] if C == 1 else img, mode).save(buf, "PNG")
        out.append(Case("pillow_" + mode, buf.getvalue(), shape, None))
    return out


def good_files():
    return block_type_files() + [far_match_file(), window_edge_file()] + filter_files() + container_files() + pillow_files()


# ----------------------------------------------------------------------------- formats only the host decodes
def host_only_files():
    H, W = 17, 31
    grey = textured((H, W, 1), 31)[:, :, 0]
    out = []

    def add(name, image, **kw):
        buf = io.BytesIO()
        image.save(buf, "PNG", **kw)
        out.append(Case(name, buf.getvalue(), (H, W, 1), None))

    add("palette", Image.fromarray(grey, "L").convert("P"))
    add("sixteen_bit", Image.fromarray(grey.astype(np.uint16) * 257))
    add("one_bit", Image.fromarray(grey, "L").convert("1"))
    add("grey_trns", Image.fromarray(grey, "L"), transparency=3)
    # Pillow does not write interlaced files: Adam7 passes of the grey frame by hand (filter 0 on every pass row)
    rows = []
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = grey[y0::dy, x0::dx]
        if sub.size:
            rows += [b"\x00" + r.tobytes() for r in sub]
    out.append(Case("interlaced", container(deflate(b"".join(rows)), (H, W, 1), interlace=1), (H, W, 1), None))
    return out


# ----------------------------------------------------------------------------- malformed streams
class BitWriter:
    def __init__(self):
        self.acc, self.n = 0, 0

    def put(self, value, nbits):              # least significant bit first (header fields, extra bits)
        self.acc |= value << self.n
        self.n += nbits

    def code(self, code, nbits):              # a Huffman code: most significant bit first
        self.put(P._reverse(code, nbits), nbits)

    def bytes(self):
        return self.acc.to_bytes((self.n + 7) // 8, "little")


def _zwrap(deflate_bytes, payload=b""):
    return b"\x78\x01" + deflate_bytes + struct.pack(">I", zlib.adler32(payload))


def malformed_files():
    shape = SMALL
    H, W, C = shape
    img = textured(shape, 41)
    stream = filter_stream(img, [1] * H)
    good = deflate(stream, 6)
    out = []

    def add(name, z, expect, shp=shape):
        out.append(Case("bad_" + name, container(z, shp), shp, frozenset(expect)))

    for k, cut in enumerate((len(good) // 4, len(good) // 2, len(good) - 3)):
        add("truncated_%d" % k, good[:cut], {INPUT_EXHAUSTED})
    w = BitWriter()                           # fixed block: literal 'a', then length 3 at distance 2 with one byte out
    w.put(1, 1), w.put(1, 2), w.code(0x30 + 0x61, 8), w.code(1, 7), w.code(1, 5), w.code(0, 7)
    add("distance_before_start", _zwrap(w.bytes()), {BAD_DISTANCE})
    add("block_type_3", _zwrap(b"\x07"), {BAD_BLOCK_TYPE})
    stored = bytearray(deflate(stream, 0))
    assert stored[2] == 1 and stored[3:5] == struct.pack("<H", len(stream))       # one final stored block
    stored[5] ^= 0x10
    add("len_nlen", bytes(stored), {BAD_STORED_LEN})
    w = BitWriter()                           # dynamic block whose 257 literal codes all have length 1
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(18 - 4, 4)
    cl = [0] * 19
    cl[1] = cl[18] = 1                        # code-length code: symbol 1 -> 0, symbol 18 -> 1
    for s in P._CL_ORDER[:18]:
        w.put(cl[s], 3)
    for _ in range(258):
        w.code(0, 1)
    add("oversubscribed", _zwrap(w.bytes() + b"\x00" * 8), {BAD_CODE})
    w = BitWriter()                           # dynamic block: only the end-of-block code (1 bit: 0); the data uses 1
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(18 - 4, 4)
    cl = [0] * 19
    cl[18], cl[0], cl[1] = 1, 2, 2            # 18 -> 0, 0 -> 10, 1 -> 11
    for s in P._CL_ORDER[:18]:
        w.put(cl[s], 3)
    w.code(0, 1), w.put(138 - 11, 7), w.code(0, 1), w.put(118 - 11, 7)            # 256 zeros
    w.code(3, 2), w.code(2, 2)                                                     # end of block: 1 bit; the distance code: 0
    w.put(1, 1)
    add("incomplete_used", _zwrap(w.bytes() + b"\x00" * 8), {BAD_SYMBOL})
    add("adler", good[:-1] + bytes([good[-1] ^ 0x40]), {BAD_ADLER})
    add("one_byte_more", deflate(stream + b"\x00", 6), {OUTPUT_OVERFLOW})
    add("one_byte_less", deflate(stream[:-1], 6), {OUTPUT_SHORT})
    bad_rows = [1] * H
    bad_rows[H // 2] = 5
    add("filter_5", deflate(filter_stream(img, bad_rows), 6), {OK})                # a valid stream: the unfilter rejects it
    return out


def bit_flip_files(count=200, seed=77):
    """Single-bit flips of one level-6 stream.  expect is None: zlib.decompress on the same bytes is the judge."""
    shape = SMALL
    z = deflate(filter_stream(textured(shape, 51), [0] * shape[0]), 6)
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        b = bytearray(z)
        i = int(rng.integers(0, len(b) * 8))
        b[i // 8] ^= 1 << (i % 8)
        out.append(Case("flip_%03d" % k, container(bytes(b), shape), shape, None))
    return out


def pillow_pixels(data):
    """Every channel as the file holds them, [H,W,C]."""
    a = np.asarray(Image.open(io.BytesIO(data)))
    return a.reshape(a.shape[0], a.shape[1], -1)


def load_one_pixels(data):
    from spnet_amd import utils as U
    return U._load_one(None, True, io.BytesIO(data), as_uint8=True)[:, :, 0]
