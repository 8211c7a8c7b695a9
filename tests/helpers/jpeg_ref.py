"""A numpy restatement of the device JPEG encoder (spnet_amd/csrc/jpeg.hip), following the recipe beside the prototypes in
include/spnet_hip.h literally: int64 arithmetic, the quantiser as the integer division it is defined as (no reciprocal), a
Python bit writer, byte stuffing and restart markers.  The tables of the standard (Annex K) and the header segments are
spnet_amd.jpeg's, which tests/test_jpeg_cpu.py holds against Pillow.  Also a small RIFF walker for the AVI files of
spnet_amd.jpeg.MjpegWriter."""
import struct

import numpy as np

from spnet_amd import jpeg as J

MAX_INTERVAL = 64


def dct_kernel():
    """K[u][x] = rint(2^12 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u > 0) = 1/2, as int64 [8][8]."""
    u = np.arange(8, dtype=np.float64)[:, None]
    x = np.arange(8, dtype=np.float64)[None, :]
    a = np.where(u == 0, np.sqrt(1.0 / 8.0), 0.5)
    return np.rint(4096.0 * a * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


K = dct_kernel()


def components(frame):
    """int64 [C][H][W] samples of a uint8 frame [H][W] (grey) or [H][W][3] (RGB -> YCbCr, 16-bit fixed point)."""
    f = np.asarray(frame).astype(np.int64)
    if f.ndim == 2 or f.shape[2] == 1:
        return f.reshape(1, f.shape[0], f.shape[1])
    r, g, b = f[..., 0], f[..., 1], f[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16
    return np.clip(np.stack([y, cb, cr]), 0, 255)


def pad_to_grid(plane):
    """Rows and columns up to the next multiple of 8, the last row and column replicated."""
    H, W = plane.shape
    return np.pad(plane, ((0, -H % 8), (0, -W % 8)), mode="edge")


def block_dct(s, info=None):
    """q [8][8] (row v, column u; 15 fractional bits) of samples s [8][8] (row y, column x).  info: a dict that collects the
    largest magnitudes of the two sums."""
    rows = (s - 128) @ K.T                       # [y][u] = sum_x K[u][x] (s[y][x] - 128)
    p = (rows + 256) >> 9
    q = K @ p                                    # [v][u] = sum_y K[v][y] p[y][u]
    if info is not None:
        info["rows"] = max(info.get("rows", 0), int(np.abs(rows).max()))
        info["p"] = max(info.get("p", 0), int(np.abs(p).max()))
        info["q"] = max(info.get("q", 0), int(np.abs(q).max()))
    return q


def quantise(q, Q):
    """sign(q) * ((|q| + (Q << 14)) // (Q << 15)): rounding half away from zero."""
    Q = np.asarray(Q, np.int64)
    return np.sign(q) * ((np.abs(q) + (Q << 14)) // (Q << 15))


def frame_coefficients(frame, quality, info=None):
    """int64 [mcu rows][mcu columns][C][64]: the quantised coefficients of every block, in zigzag order."""
    qt = J.quant_tables(quality).astype(np.int64).reshape(2, 8, 8)
    comps = [pad_to_grid(p) for p in components(frame)]
    mh, mw = comps[0].shape[0] // 8, comps[0].shape[1] // 8
    out = np.zeros((mh, mw, len(comps), 64), np.int64)
    zz = np.array(J.ZIGZAG)
    for c, plane in enumerate(comps):
        Q = qt[0 if c == 0 else 1]
        for my in range(mh):
            for mx in range(mw):
                coef = quantise(block_dct(plane[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8], info), Q)
                out[my, mx, c] = coef.reshape(64)[zz]
    return out


class BitWriter:
    """Bits fill bytes from the most significant bit; flush pads with 1-bits; stuffed() puts 0x00 behind every 0xFF."""

    def __init__(self):
        self.bits = []

    def put(self, value, nbits):
        for k in range(nbits - 1, -1, -1):
            self.bits.append((value >> k) & 1)

    def stuffed(self):
        bits = self.bits + [1] * (-len(self.bits) % 8)
        out = bytearray()
        for i in range(0, len(bits), 8):
            b = 0
            for v in bits[i:i + 8]:
                b = b << 1 | v
            out.append(b)
            if b == 0xFF:
                out.append(0)
        return bytes(out)


def _category(v):
    return int(abs(int(v))).bit_length()


def _value_bits(v, s):
    v = int(v)
    return (v if v >= 0 else v - 1) & ((1 << s) - 1)


def encode_block(w, coef, pred, dc_codes, ac_codes, stats):
    """One block's codes (T.81 F.1.2): returns its DC, the next block's predictor."""
    diff = int(coef[0]) - pred
    s = _category(diff)
    stats["dc_category"] = max(stats["dc_category"], s)
    w.put(*dc_codes[s])
    w.put(_value_bits(diff, s), s)
    run = 0
    for k in range(1, 64):
        c = int(coef[k])
        if c == 0:
            run += 1
            continue
        while run >= 16:
            w.put(*ac_codes[0xF0])
            stats["zrl"] += 1
            run -= 16
        s = _category(c)
        stats["ac_category"] = max(stats["ac_category"], s)
        w.put(*ac_codes[run << 4 | s])
        w.put(_value_bits(c, s), s)
        run = 0
    if run:
        w.put(*ac_codes[0x00])
        stats["eob"] += 1
    return int(coef[0])


def restart_interval(width):
    return min((width + 7) // 8, MAX_INTERVAL)


def encode_scan(frame, quality=90, info=None):
    """(scan bytes, interval sizes, stats) of one frame: the intervals of restart_interval(W) MCUs in raster order, RSTm
    between them.  stats: zrl / eob counts, the largest size categories, stuffed = number of FF 00 pairs."""
    coefs = frame_coefficients(frame, quality, info)
    mh, mw, C = coefs.shape[:3]
    flat = coefs.reshape(mh * mw, C, 64)
    ri = restart_interval(np.asarray(frame).shape[1])
    dc = [J.huffman_codes(J.DC_LUMINANCE), J.huffman_codes(J.DC_CHROMINANCE)]
    ac = [J.huffman_codes(J.AC_LUMINANCE), J.huffman_codes(J.AC_CHROMINANCE)]
    stats = dict(zrl=0, eob=0, dc_category=0, ac_category=0, stuffed=0)
    out = bytearray()
    sizes = []
    starts = list(range(0, mh * mw, ri))
    for i, m0 in enumerate(starts):
        w = BitWriter()
        pred = [0] * C
        for m in range(m0, min(m0 + ri, mh * mw)):
            for c in range(C):
                t = 0 if c == 0 else 1
                pred[c] = encode_block(w, flat[m, c], pred[c], dc[t], ac[t], stats)
        data = w.stuffed()
        stats["stuffed"] += data.count(b"\xff\x00")
        sizes.append(len(data))
        out += data
        if i < len(starts) - 1:
            out += bytes([0xFF, 0xD0 + (i & 7)])
    return bytes(out), np.array(sizes, np.uint32), stats


def encode_jpeg(frame, quality=90):
    """The whole file."""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    channels = 1 if frame.ndim == 2 else frame.shape[2]
    return J.jpeg_header(W, H, channels, quality) + encode_scan(frame, quality)[0] + J.JPEG_TRAILER


# ----------------------------------------------------------------------------- RIFF
def walk_riff(data):
    """The chunks of a RIFF file as nested lists: ("RIFF" | "LIST", form type, position, size, [children]) and (tag,
    position, size, payload) -- position: of the chunk's header.  Asserts that every size stays inside its parent and
    that chunks start on even positions."""
    def walk(lo, hi):
        out = []
        pos = lo
        while pos < hi:
            assert pos % 2 == 0 and pos + 8 <= hi, (pos, hi)
            tag = data[pos:pos + 4]
            size, = struct.unpack("<I", data[pos + 4:pos + 8])
            assert pos + 8 + size <= hi, (tag, pos, size, hi)
            if tag in (b"RIFF", b"LIST"):
                out.append((tag.decode(), data[pos + 8:pos + 12].decode(), pos, size, walk(pos + 12, pos + 8 + size)))
            else:
                out.append((tag.decode(), pos, size, data[pos + 8:pos + 8 + size]))
            pos += 8 + size + (size & 1)
        assert pos == hi or pos == hi + 1, (pos, hi)
        return out
    top = walk(0, len(data))
    assert len(top) == 1 and top[0][0] == "RIFF" and top[0][3] == len(data) - 8
    return top[0]


def parse_avi(data):
    """dict of an MjpegWriter file: avih / strh / strf fields, frames (the 00dc payloads in file order) and index (the
    idx1 entries: (flags, offset from the 'movi' tag, length)); asserts the layout on the way."""
    riff = walk_riff(data)
    assert riff[1] == "AVI "
    kids = riff[4]
    assert [k[0] for k in kids] == ["LIST", "LIST", "idx1"] and kids[0][1] == "hdrl" and kids[1][1] == "movi"
    hdrl, movi, idx1 = kids
    assert [k[0] for k in hdrl[4]] == ["avih", "LIST"] and hdrl[4][1][1] == "strl"
    avih = struct.unpack("<14I", hdrl[4][0][3])
    strl = hdrl[4][1][4]
    assert [k[0] for k in strl] == ["strh", "strf"]
    strh_raw, strf_raw = strl[0][3], strl[1][3]
    assert len(strh_raw) == 56 and len(strf_raw) == 40
    strh = struct.unpack("<IHHIIIIIIII4H", strh_raw[8:])
    strf = struct.unpack("<IiiHH4sIiiII", strf_raw)
    assert all(k[0] == "00dc" for k in movi[4])
    movi_tag = movi[2] + 8
    index = [struct.unpack("<4sIII", idx1[3][k:k + 16]) for k in range(0, idx1[2], 16)]
    return dict(usec_per_frame=avih[0], flags=avih[3], total_frames=avih[4], streams=avih[6], width=avih[8], height=avih[9],
                fcc_type=strh_raw[:4], handler=strh_raw[4:8], scale=strh[4], rate=strh[5], length=strh[7],
                bi_size=strf[0], bi_width=strf[1], bi_height=strf[2], bi_bits=strf[4], compression=strf[5],
                frames=[k[3] for k in movi[4]], chunk_at=[k[1] for k in movi[4]], movi_tag=movi_tag, index=index)
