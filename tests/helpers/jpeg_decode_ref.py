"""A numpy restatement of the device JPEG decoder (spnet_amd/csrc/jpeg_decode.hip), following the recipe beside the
prototypes in include/spnet_hip.h literally: its own marker walk, Huffman decoding bit by bit from the (BITS, HUFFVAL)
tables with the same rejection rules, dequantisation, the "islow" inverse DCT of libjpeg (jidctint.c), libjpeg's "fancy"
(triangle) chroma upsampling, its 16-bit fixed-point YCbCr -> RGB rule, the crop to the true size.  int64 arithmetic."""
import numpy as np

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63)

OK, BAD_CODE, BAD_INDEX, BAD_CATEGORY, INPUT_EXHAUSTED, TRAILING_BYTES, BAD_ARGS = range(7)


class Reject(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


# ----------------------------------------------------------------------------- container
def walk(data, default_tables=None):
    """dict(width, height, comps [(h, v, tq, td, ta)], quant {id: int64 [64] natural}, huff {(class, id): {(length, code):
    symbol}}, restart, intervals [(lo, hi)]) of a baseline file with one scan.  default_tables: the (class, id, (BITS,
    HUFFVAL)) tables of a file without DHT."""
    assert data[:2] == b"\xff\xd8"
    pos = 2
    quant, huff, restart, frame, have_dht = {}, {}, 0, None, False
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        length = data[pos + 2] << 8 | data[pos + 3]
        body = data[pos + 4:pos + 2 + length]
        pos += 2 + length
        if m == 0xDB:
            k = 0
            while k < len(body):
                assert body[k] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[list(ZIGZAG)] = list(body[k + 1:k + 65])
                quant[body[k] & 15] = t
                k += 65
        elif m == 0xC0:
            assert body[0] == 8
            height, width, nc = body[1] << 8 | body[2], body[3] << 8 | body[4], body[5]
            frame = [(body[7 + 3 * c] >> 4, body[7 + 3 * c] & 15, body[8 + 3 * c]) for c in range(nc)]
        elif m == 0xC4:
            have_dht = True
            k = 0
            while k < len(body):
                bits = body[k + 1:k + 17]
                vals = body[k + 17:k + 17 + sum(bits)]
                huff[(body[k] >> 4, body[k] & 15)] = code_table(bits, vals)
                k += 17 + sum(bits)
        elif m == 0xDD:
            restart = body[0] << 8 | body[1]
        elif m == 0xDA:
            nc = body[0]
            comps = [frame[c] + (body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(nc)]
            break
    if not have_dht and default_tables is not None:
        huff = {(cls, dest): code_table(*tab) for cls, dest, tab in default_tables}
    intervals = []
    lo = pos
    k = pos
    while True:
        k = data.index(b"\xff", k)
        nxt = data[k + 1]
        if nxt == 0:
            k += 2
            continue
        intervals.append((lo, k))
        if nxt == 0xD9:
            break
        assert 0xD0 <= nxt <= 0xD7
        lo = k = k + 2
    return dict(width=width, height=height, comps=comps, quant=quant, huff=huff, restart=restart, intervals=intervals)


def code_table(bits, vals):
    """{(length, code): symbol}: codes of one length are consecutive in HUFFVAL order (T.81 Annex C)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[(length, code)] = vals[k]
            code += 1
            k += 1
        code <<= 1
    return out


# ----------------------------------------------------------------------------- entropy decoding
class BitReader:
    """The bits of one restart interval, most significant first; FF 00 is the byte FF; an FF followed by anything else, or
    by nothing, ends the data."""

    def __init__(self, data):
        raw = bytearray()
        k = 0
        while k < len(data):
            b = data[k]
            if b == 0xFF:
                if k + 1 < len(data) and data[k + 1] == 0:
                    k += 1
                else:
                    break
            raw.append(b)
            k += 1
        self.left_unread = k < len(data)
        self.bits = np.unpackbits(np.frombuffer(bytes(raw), np.uint8)).tolist()
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.bits):
            raise Reject(INPUT_EXHAUSTED)
        v = 0
        for b in self.bits[self.at:self.at + n]:
            v = v << 1 | b
        self.at += n
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            if self.at >= len(self.bits):
                # the device looks ahead into zero bits: a code it finds there is "bits missing", none is "no code"
                rest = code
                for l2 in range(length, 17):
                    rest <<= 1
                    if (l2, rest) in table:
                        raise Reject(INPUT_EXHAUSTED)
                raise Reject(BAD_CODE)
            code = code << 1 | self.bits[self.at]
            self.at += 1
            if (length, code) in table:
                return table[(length, code)]
        raise Reject(BAD_CODE)

    def finished(self):
        return not self.left_unread and len(self.bits) - self.at < 8


def extend(v, s):
    return v if s == 0 or v >> (s - 1) else v - (1 << s) + 1


def decode_block(r, dc_table, ac_table, pred):
    """(coefficients int64 [64] in natural order, the DC) of the next block."""
    coef = np.zeros(64, np.int64)
    s = r.symbol(dc_table)
    if s > 11:
        raise Reject(BAD_CATEGORY)
    pred += extend(r.take(s), s)
    coef[0] = ((pred + 32768) & 65535) - 32768                    # the workspace holds int16
    k = 1
    while k < 64:
        rs = r.symbol(ac_table)
        run, s = rs >> 4, rs & 15
        if s == 0:
            if run != 15:
                break                                              # EOB
            k += 16                                                # ZRL
            if k > 64:
                raise Reject(BAD_INDEX)
            continue
        if s > 10:
            raise Reject(BAD_CATEGORY)
        k += run
        if k > 63:
            raise Reject(BAD_INDEX)
        coef[ZIGZAG[k]] = extend(r.take(s), s)
        k += 1
    return coef, pred


def decode_coefficients(data, info):
    """(status, [component] int64 [block rows][block columns][64]): the first non-zero status of an interval is the file's."""
    comps = info["comps"]
    hs, vs = (comps[0][0], comps[0][1]) if len(comps) == 3 else (1, 1)
    mw = -(-info["width"] // (8 * hs))
    mh = -(-info["height"] // (8 * vs))
    samp = [(hs, vs)] + [(1, 1)] * (len(comps) - 1)
    planes = [np.zeros((mh * v, mw * h, 64), np.int64) for h, v in samp]
    ri = info["restart"] or mw * mh
    status = OK
    for i, (lo, hi) in enumerate(info["intervals"]):
        r = BitReader(data[lo:hi])
        pred = [0] * len(comps)
        try:
            for m in range(i * ri, min((i + 1) * ri, mw * mh)):
                my, mx = divmod(m, mw)
                for c, (h, v) in enumerate(samp):
                    for by in range(v):
                        for bx in range(h):
                            coef, pred[c] = decode_block(r, info["huff"].get((0, comps[c][3]), {}),
                                                         info["huff"].get((1, comps[c][4]), {}), pred[c])
                            planes[c][my * v + by, mx * h + bx] = coef
            if not r.finished():
                raise Reject(TRAILING_BYTES)
        except Reject as e:
            status = status or e.status
    return status, planes


# ----------------------------------------------------------------------------- pixels
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _idct_1d(x, shift):
    """libjpeg's jidctint.c butterfly on the FIRST axis of x (int64 [8][...]), descaled by `shift`."""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * F_0_541
    tmp2 = z1 - z3 * F_1_847
    tmp3 = z1 + z2 * F_0_765
    tmp0 = (x[0] + x[4]) << 13
    tmp1 = (x[0] - x[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F_1_175
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F_0_298, tmp1 * F_2_053, tmp2 * F_3_072, tmp3 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2,
                    tmp10 - tmp3])
    return (out + (1 << (shift - 1))) >> shift


def idct_islow(coef, quant):
    """Samples int64 [...][8][8] of coefficients [...][64] (natural order): dequantise, columns (CONST_BITS 13, PASS1_BITS 2:
    descale by 11), rows (descale by 18), + 128, clamp to 0 .. 255."""
    c = (np.asarray(coef, np.int64) * quant).reshape(coef.shape[:-1] + (8, 8))
    c = np.moveaxis(c, -2, 0)                       # rows (vertical frequency) first: the column pass
    ws = _idct_1d(c, 11)                            # [y][...][u]
    ws = np.moveaxis(ws, -1, 0)                     # [u][y][...]
    out = _idct_1d(ws, 18)                          # [x][y][...]
    out = np.moveaxis(np.moveaxis(out, 0, -1), 0, -2)
    return np.clip(out + 128, 0, 255)


def plane_of(blocks):
    """[block rows][block columns][8][8] -> [rows][columns]."""
    bh, bw = blocks.shape[:2]
    return blocks.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def upsample_h2v1(p, dw):
    """Columns doubled with libjpeg's triangle filter, over the component's dw = ceil(W / 2) true columns, edges
    replicated: out[2i] = (3 p[i] + p[i-1] + 1) >> 2, out[2i+1] = (3 p[i] + p[i+1] + 2) >> 2."""
    p = p[:, :dw]
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((p.shape[0], 2 * dw), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    return out


def upsample_h2v2(p, dw, dh):
    """Rows first (3 near + far, unscaled; rows replicated at the top and bottom of the dh = ceil(H / 2) true rows), then
    columns: out[2i] = (3 this + left + 8) >> 4, out[2i+1] = (3 this + right + 7) >> 4."""
    p = p[:dh, :dw]
    above = np.concatenate([p[:1], p[:-1]])
    below = np.concatenate([p[1:], p[-1:]])
    rows = np.empty((2 * dh, dw), np.int64)
    rows[0::2] = 3 * p + above
    rows[1::2] = 3 * p + below
    left = np.concatenate([rows[:, :1], rows[:, :-1]], axis=1)
    right = np.concatenate([rows[:, 1:], rows[:, -1:]], axis=1)
    out = np.empty((2 * dh, 2 * dw), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out


def pixels(planes, info):
    """uint8 [H][W] (one component) or [H][W][3] (RGB)."""
    H, W = info["height"], info["width"]
    comps = info["comps"]
    samples = [plane_of(idct_islow(planes[c], info["quant"][comps[c][2]])) for c in range(len(comps))]
    y = samples[0][:H, :W]
    if len(comps) == 1:
        return y.astype(np.uint8)
    hs, vs = comps[0][0], comps[0][1]
    chroma = []
    for p in samples[1:]:
        if (hs, vs) == (2, 1):
            p = upsample_h2v1(p, -(-W // 2))
        elif (hs, vs) == (2, 2):
            p = upsample_h2v2(p, -(-W // 2), -(-H // 2))
        chroma.append(p[:H, :W] - 128)
    cb, cr = chroma
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def decode(data, default_tables=None):
    """(status, pixels or None)."""
    info = walk(data, default_tables)
    status, planes = decode_coefficients(data, info)
    return status, (pixels(planes, info) if status == OK else None)
