"""The PNG encoder of spnet_amd/png.py + csrc/png.hip restated in numpy and plain Python, bit by bit: filtered stream,
histogram, Adler-32, prefix codes, block header, bit packer and container.  It imports nothing from spnet_amd: it is the
specification the device bytes are compared with, and zlib / Pillow are what IT is checked against (tests/test_png_cpu.py).

A stream is built as an explicit array of bits in stream order and only then packed into bytes, least significant bit of
every byte first -- no shifting accumulator, no words, no notion of threads.

The code construction (what makes the bytes unique; any other valid choice would decode to the same pixels):
  lengths   Huffman, merging the two smallest of (count, order), where a symbol's order is its index and a merged node comes
            after every symbol and after every node merged before it; only the NUMBER of codes of each depth is kept; depths
            beyond the limit are folded into the limit and the Kraft sum is repaired one unit at a time (remove one code of
            the limit length, replace the deepest shorter code by two of the next length); the lengths, shortest first, go to
            the symbols ordered by (count descending, index ascending)
  codes     RFC 1951 section 3.2.2
  header    BFINAL 1, BTYPE 2, HLIT 0, HDIST 0 (one distance code of zero bits), lengths of the 257 symbols and of the one
            distance code run-length coded greedily as one sequence, code-length code by the same construction, limit 7
"""
import struct
import zlib

import numpy as np

ADLER_MOD = 65521
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
COLOUR_TYPE = {1: 0, 3: 2}


def filtered_stream(frame):
    """uint8 [H,W] or [H,W,C] -> the scanline stream with filter type 0 in front of every row, as a uint8 array."""
    frame = np.asarray(frame, dtype=np.uint8)
    rows = frame.reshape(frame.shape[0], -1)
    return np.concatenate([np.zeros((rows.shape[0], 1), np.uint8), rows], axis=1).reshape(-1)


def histogram(stream):
    return np.bincount(stream, minlength=256).astype(np.uint32)


def adler32(stream):
    """The definition: a runs over 1 + the bytes so far, b over the values of a."""
    a = 1 + np.cumsum(stream.astype(np.int64))
    return (int(a.sum() % ADLER_MOD) << 16) | int(a[-1] % ADLER_MOD) if len(stream) else 1


def code_lengths(freq, limit):
    """Two-queue Huffman (sorted leaves, merged nodes in the order they were made; a leaf wins a tie), then the limiter."""
    freq = [int(f) for f in freq]
    used = [s for s in range(len(freq)) if freq[s] > 0]
    out = [0] * len(freq)
    if len(used) < 2:
        for s in used:
            out[s] = 1
        return out
    leaves = sorted(used, key=lambda s: (freq[s], s))
    weight = [freq[s] for s in leaves]          # nodes 0 .. len(leaves)-1 are leaves, the rest merged
    kids = {}
    li, mi = 0, len(leaves)                     # heads of the two queues

    def take():
        nonlocal li, mi
        if li < len(leaves) and (mi >= len(weight) or weight[li] <= weight[mi]):
            li += 1
            return li - 1
        mi += 1
        return mi - 1

    for _ in range(len(leaves) - 1):
        x = take()
        y = take()
        kids[len(weight)] = (x, y)
        weight.append(weight[x] + weight[y])
    depth_count = {}
    stack = [(len(weight) - 1, 0)]
    while stack:
        node, d = stack.pop()
        if node in kids:
            stack += [(kids[node][0], d + 1), (kids[node][1], d + 1)]
        else:
            depth_count[d] = depth_count.get(d, 0) + 1
    count = [0] * (limit + 1)
    for d, c in depth_count.items():
        count[min(d, limit)] += c
    kraft = sum(count[d] * 2 ** (limit - d) for d in range(1, limit + 1))
    while kraft > 2 ** limit:
        count[limit] -= 1
        d = max(e for e in range(1, limit) if count[e] > 0)
        count[d] -= 1
        count[d + 1] += 2
        kraft -= 1
    by_rank = sorted(used, key=lambda s: (-freq[s], s))
    shortest_first = [d for d in range(1, limit + 1) for _ in range(count[d])]
    for s, d in zip(by_rank, shortest_first):
        out[s] = d
    return out


def literal_lengths(hist):
    return code_lengths([int(c) for c in hist] + [1], 15)


def canonical(lengths):
    """Codes in (length, symbol) order count upwards; a longer code continues from the previous one shifted left."""
    codes = [0] * len(lengths)
    code, prev = 0, 0
    for d, s in sorted((d, s) for s, d in enumerate(lengths) if d > 0):
        code <<= d - prev
        codes[s] = code
        code += 1
        prev = d
    return codes


def lsb_first(value, nbits):
    return [(value >> k) & 1 for k in range(nbits)]


def msb_first(code, nbits):
    return [(code >> (nbits - 1 - k)) & 1 for k in range(nbits)]


def run_length(seq):
    """[(symbol, extra bit count, extra value)]."""
    out = []
    pos = 0
    while pos < len(seq):
        v = seq[pos]
        run = 1
        while pos + run < len(seq) and seq[pos + run] == v:
            run += 1
        pos += run
        if v == 0:
            while run >= 11:
                take = min(run, 138)
                out.append((18, 7, take - 11))
                run -= take
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
            out += [(0, 0, 0)] * run
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                take = min(run, 6)
                out.append((16, 2, take - 3))
                run -= take
            out += [(v, 0, 0)] * run
    return out


def header_bit_list(lengths):
    assert len(lengths) == 257
    items = run_length(list(lengths) + [0])
    cl_freq = [sum(1 for it in items if it[0] == s) for s in range(19)]
    cl_len = code_lengths(cl_freq, 7)
    cl_code = canonical(cl_len)
    hclen = max(4, 1 + max(k for k in range(19) if cl_len[CL_ORDER[k]] > 0))
    bits = [1] + lsb_first(2, 2) + lsb_first(0, 5) + lsb_first(0, 5) + lsb_first(hclen - 4, 4)
    for k in range(hclen):
        bits += lsb_first(cl_len[CL_ORDER[k]], 3)
    for sym, nextra, extra in items:
        bits += msb_first(cl_code[sym], cl_len[sym]) + lsb_first(extra, nextra)
    return bits


def literal_bits(stream, lengths, codes):
    """Bits of every byte's code, most significant code bit first, as one uint8 array."""
    ln = np.asarray(lengths[:256], np.int32)[stream]
    cd = np.asarray(codes[:256], np.int32)[stream]
    shift = ln[:, None] - 1 - np.arange(15, dtype=np.int32)[None, :]
    return ((cd[:, None] >> np.maximum(shift, 0)) & 1)[shift >= 0].astype(np.uint8)


def zlib_stream(frame):
    """(the zlib stream as bytes, dict of the intermediate values)."""
    stream = filtered_stream(frame)
    hist = histogram(stream)
    lengths = literal_lengths(hist)
    codes = canonical(lengths)
    head = header_bit_list(lengths)
    bits = np.concatenate([np.array(head, np.uint8), literal_bits(stream, lengths, codes),
                           np.array(msb_first(codes[256], lengths[256]), np.uint8)])
    adler = adler32(stream)
    data = b"\x78\x01" + np.packbits(bits, bitorder="little").tobytes() + struct.pack(">I", adler)
    return data, dict(stream=stream, hist=hist, lengths=lengths, codes=codes, header_bits=head, adler=adler,
                      nbits=int(bits.size))


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))


def png_bytes(frame, zstream=None):
    frame = np.asarray(frame, dtype=np.uint8)
    channels = 1 if frame.ndim == 2 else frame.shape[2]
    if zstream is None:
        zstream = zlib_stream(frame)[0]
    ihdr = struct.pack(">IIBBBBB", frame.shape[1], frame.shape[0], 8, COLOUR_TYPE[channels], 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", bytes(zstream)) + chunk(b"IEND", b"")


def read_chunks(png):
    """[(tag, data, stored crc)] of a PNG byte string; raises on a broken layout."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    out, pos = [], 8
    while pos < len(png):
        (n,) = struct.unpack(">I", png[pos:pos + 4])
        tag, data = png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", png[pos + 8 + n:pos + 12 + n])
        out.append((tag, data, crc))
        pos += 12 + n
    assert pos == len(png)
    return out


# ----------------------------------------------------------------------------- the frames of the tests
def fibonacci_frame(height=134, width=133, levels=20):
    """Grey frame of `levels` grey values with Fibonacci pixel counts 1, 1, 2, 3, ... (alone: a Huffman tree of depth levels - 1
    = 19).  The stream also holds the end-of-block symbol (count 1) and the filter bytes, and extra small counts split the
    Fibonacci chain in two and halve the depth; so the first level IS grey 0, the filter bytes' symbol, and takes the pixels
    the 20 counts leave over: the stream's counts are then 1 (end of block), 1, 2, 3, ... 6765 and 247 for symbol 0, and the
    unlimited tree is 16 deep (tests/test_png_cpu.py asserts it).  Shuffled."""
    fib = [1, 1]
    while len(fib) < levels:
        fib.append(fib[-1] + fib[-2])
    assert sum(fib) <= height * width
    fib[0] += height * width - sum(fib)
    vals = np.concatenate([np.full(c, 0 if k == 0 else 10 + 3 * k, np.uint8) for k, c in enumerate(fib)])
    np.random.RandomState(5).shuffle(vals)
    return vals.reshape(height, width)


def small_frames():
    """name -> frame: the smallest frames that can still break the packer."""
    r = np.random.RandomState(11)
    two = np.where(r.rand(16, 16) < 0.3, 7, 250).astype(np.uint8)
    return {
        "grey_1x1": np.array([[173]], np.uint8),
        "grey_7x13": r.randint(0, 256, (7, 13)).astype(np.uint8),
        "rgb_3x5": r.randint(0, 256, (3, 5, 3)).astype(np.uint8),
        "grey_16x16_zeros": np.zeros((16, 16), np.uint8),
        "grey_16x16_two_values": two,
        "grey_64x48_uniform": r.randint(0, 256, (64, 48)).astype(np.uint8),
        "grey_134x133_fibonacci": fibonacci_frame(),
    }


def batch_of(frame, n=5, seed=3):
    """n frames of frame's shape with different contents (frame itself is number 2): rolled, reversed, thinned out and noise,
    so that histograms, code lengths, stream lengths and bit tails all differ."""
    r = np.random.RandomState(seed)
    flat = frame.reshape(-1)
    others = [np.roll(flat, 1) // 2, flat[::-1] | 1, frame.reshape(-1).copy(), np.where(r.rand(flat.size) < 0.5, flat, 0),
              r.randint(0, 256, flat.size)]
    return np.stack([o.astype(np.uint8).reshape(frame.shape) for o in others[:n]])
