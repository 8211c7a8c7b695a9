"""The LZ77 stage of the device PNG encoder (spnet_amd/csrc/png_lz.hip + spnet_amd/png.py, lz77=True) restated in numpy and
plain Python from the documented token rule ("PNG output: the LZ77 stage"): tokens, the two histograms, the two
prefix codes, the block header and the bits.  It imports nothing from spnet_amd; the Huffman construction, the run-length
coder and the container are tests/helpers/png_ref.py's, which is the specification of the literal-only encoder already.

The rule speaks of stream positions only -- no threads, no waves, no tables:

  S            the filtered stream (filter type 0 in front of every row), L bytes; c = bytes per pixel, rb = W * c
  segment      positions k * 1024 .. k * 1024 + 1023 (cut at L); its LANE is k mod 16
  key(q)       ((S[q] | S[q+1] << 8 | S[q+2] << 16) * 0x9E3779B1 mod 2^32) >> 23, for q + 3 <= L (9 bits)
  candidates   of position p, in this order: distance 1; c, 2c .. 8c; rb + 1; the LANE one: p - q for the largest q with
               q + 3 <= L, q's segment on the same lane as p's, q < 64 * (p // 64) and key(q) == key(p); the NEIGHBOUR
               one: p - q for the largest q of the segment before p's with q + 3 <= L and key(q) == key(p) (both need
               p + 3 <= L; each is that ONE q, whatever its distance turns out to be)
  length       of a candidate d with 1 <= d <= min(p, 32768): the number of i < min(258, segment end - p) with
               S[p + i] == S[p - d + i] from i = 0 without a gap; the candidate counts if the length is >= 4, or 3 with
               d <= 1024
  match(p)     the counting candidate of the greatest length, the first in the order above among equals
  parse        greedy from the start of every segment: a match where match(p) exists (p += length), else a literal
"""
import struct

import numpy as np

from tests.helpers import png_ref as R

SEGMENT = 1024
LANES = 16
GROUP = 64
KEY_BITS = 9
KEY_MUL = 0x9E3779B1
PIXEL_MULTIPLES = 8
WINDOW = 32768
MAX_LEN = 258
NEAR = 1024

LENGTH_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LENGTH_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def _keys(S):
    L = S.size
    if L < 3:
        return np.zeros(0, np.int64)
    s = S.astype(np.int64)
    word = s[:L - 2] | (s[1:L - 1] << 8) | (s[2:] << 16)
    return ((word * KEY_MUL) & 0xFFFFFFFF) >> (32 - KEY_BITS)


def _keyed_source(S):
    """q of the keyed candidate of every position (-1: none)."""
    L = S.size
    out = np.full(L, -1, np.int64)
    key = _keys(S)
    n = key.size
    if n == 0:
        return out
    pos = np.arange(n, dtype=np.int64)
    lane = (pos // SEGMENT) % LANES
    tag = ((lane << KEY_BITS) | key) << 32                       # equal tag <=> same lane and same key
    order = np.argsort(tag | pos, kind="stable")
    table = (tag | pos)[order]
    ask = tag | (pos // GROUP * GROUP)                           # the first entry >= (tag, start of p's group of 64) ...
    at = np.searchsorted(table, ask) - 1                         # ... and the one before it
    ok = (at >= 0) & ((table[np.maximum(at, 0)] >> 32) == (tag >> 32))
    out[:n] = np.where(ok, table[np.maximum(at, 0)] & 0xFFFFFFFF, -1)
    return out


def _neighbour_source(S):
    """q of the neighbour candidate of every position (-1: none)."""
    L = S.size
    out = np.full(L, -1, np.int64)
    key = _keys(S)
    n = key.size
    if n == 0:
        return out
    pos = np.arange(n, dtype=np.int64)
    seg = pos // SEGMENT
    table = np.sort((((seg << KEY_BITS) | key) << 32) | pos)
    ask = (((seg - 1) << KEY_BITS) | key) << 32                  # the last entry of (segment before, key), if there is one
    at = np.searchsorted(table, ask | 0xFFFFFFFF, side="right") - 1
    ok = (seg >= 1) & (at >= 0) & ((table[np.maximum(at, 0)] >> 32) == (ask >> 32))
    out[:n] = np.where(ok, table[np.maximum(at, 0)] & 0xFFFFFFFF, -1)
    return out


def _run_lengths(S, p, q, cap):
    """For the pairs (p[k], q[k]): how many bytes agree from there on, at most cap[k]."""
    n = np.zeros(p.size, np.int64)
    live = np.nonzero(cap > 0)[0]
    while live.size:
        same = S[p[live] + n[live]] == S[q[live] + n[live]]
        live = live[same]
        n[live] += 1
        live = live[n[live] < cap[live]]
    return n


def matches(S, channels, rb):
    """(length [L], distance [L]) of match(p) for every p; length 0 where there is none."""
    L = S.size
    p = np.arange(L, dtype=np.int64)
    cap = np.minimum(MAX_LEN, np.minimum(L, (p // SEGMENT + 1) * SEGMENT) - p)
    best_n = np.zeros(L, np.int64)
    best_d = np.zeros(L, np.int64)

    def offer(d, valid):
        d = np.broadcast_to(np.asarray(d, np.int64), (L,))
        valid = valid & (d >= 1) & (d <= np.minimum(p, WINDOW))
        idx = np.nonzero(valid)[0]
        n = np.zeros(L, np.int64)
        n[idx] = _run_lengths(S, idx, idx - d[idx], cap[idx])
        counts = (n >= 4) | ((n == 3) & (d <= NEAR))
        better = counts & (n > best_n)
        best_n[better] = n[better]
        best_d[better] = d[better]

    everywhere = np.ones(L, bool)
    for d in [1] + [channels * k for k in range(1, PIXEL_MULTIPLES + 1)] + [rb + 1]:
        offer(d, everywhere)
    for q in (_keyed_source(S), _neighbour_source(S)):
        offer(p - q, q >= 0)
    return best_n, best_d


def tokens(frame):
    """[(position, length, distance)] in stream order; a literal has length 0 and distance 0."""
    frame = np.asarray(frame, np.uint8)
    S = R.filtered_stream(frame)
    channels = 1 if frame.ndim == 2 else frame.shape[2]
    n, d = matches(S, channels, frame.shape[1] * channels)
    n, d = n.tolist(), d.tolist()
    out = []
    L = S.size
    for start in range(0, L, SEGMENT):
        end = min(L, start + SEGMENT)
        p = start
        while p < end:
            if n[p]:
                assert p + n[p] <= end and d[p] <= p
                out.append((p, n[p], d[p]))
                p += n[p]
            else:
                out.append((p, 0, 0))
                p += 1
    return out


def length_symbol(n):
    k = max(j for j in range(29) if LENGTH_BASE[j] <= n)
    return 257 + k, LENGTH_EXTRA[k], n - LENGTH_BASE[k]


def distance_symbol(d):
    k = max(j for j in range(30) if DIST_BASE[j] <= d)
    return k, DIST_EXTRA[k], d - DIST_BASE[k]


_LEN_SYM = [None] * 3 + [length_symbol(n) for n in range(3, MAX_LEN + 1)]


def histograms(S, toks):
    """(literal/length counts [286] with the end of block counted once, distance counts [30])."""
    lh = np.zeros(286, np.int64)
    dh = np.zeros(30, np.int64)
    pos = np.array([t[0] for t in toks], np.int64)
    ln = np.array([t[1] for t in toks], np.int64)
    lh[:256] = np.bincount(S[pos[ln == 0]], minlength=256)
    for n, count in zip(*np.unique(ln[ln > 0], return_counts=True)):
        lh[_LEN_SYM[int(n)][0]] += count
    for d, count in zip(*np.unique(np.array([t[2] for t in toks if t[1]], np.int64), return_counts=True)):
        dh[distance_symbol(int(d))[0]] += count
    lh[256] = 1
    return lh, dh


def code_sets(lh, dh):
    """(literal/length lengths [286], distance lengths [30]): both limited to 15 bits; one used distance symbol gets one
    bit, none leaves all thirty at zero (RFC 1951, section 3.2.7)."""
    return R.code_lengths(lh, 15), R.code_lengths(dh, 15)


def header_bit_list(ll, dl):
    nl = max(257, 1 + max(s for s in range(286) if ll[s]))
    nd = max([1] + [1 + s for s in range(30) if dl[s]])
    items = R.run_length(list(ll[:nl]) + list(dl[:nd]))
    cl_freq = [sum(1 for it in items if it[0] == s) for s in range(19)]
    cl_len = R.code_lengths(cl_freq, 7)
    cl_code = R.canonical(cl_len)
    hclen = max(4, 1 + max(k for k in range(19) if cl_len[R.CL_ORDER[k]] > 0))
    bits = [1] + R.lsb_first(2, 2) + R.lsb_first(nl - 257, 5) + R.lsb_first(nd - 1, 5) + R.lsb_first(hclen - 4, 4)
    for k in range(hclen):
        bits += R.lsb_first(cl_len[R.CL_ORDER[k]], 3)
    for sym, nextra, extra in items:
        bits += R.msb_first(cl_code[sym], cl_len[sym]) + R.lsb_first(extra, nextra)
    return bits


def _field_bits(value, nbits, msb):
    """Bits of many fields at once: field k holds nbits[k] bits of value[k], most significant first where msb[k]."""
    value, nbits, msb = (np.asarray(a, np.int64) for a in (value, nbits, msb))
    col = np.arange(15, dtype=np.int64)[None, :]
    shift = np.where(msb[:, None] != 0, nbits[:, None] - 1 - col, col)
    keep = col < nbits[:, None]
    return ((value[:, None] >> np.clip(shift, 0, 62)) & 1)[keep].astype(np.uint8)


def token_bits(S, toks, ll, lc, dl, dc):
    """Four fields per token (length or literal code, length extra, distance code, distance extra), empty where unused."""
    T = len(toks)
    value = np.zeros((T, 4), np.int64)
    nbits = np.zeros((T, 4), np.int64)
    for k, (p, n, d) in enumerate(toks):
        if n == 0:
            s = int(S[p])
            value[k, 0], nbits[k, 0] = lc[s], ll[s]
        else:
            s, eb, ev = _LEN_SYM[n]
            value[k, 0], nbits[k, 0] = lc[s], ll[s]
            value[k, 1], nbits[k, 1] = ev, eb
            s, eb, ev = distance_symbol(d)
            value[k, 2], nbits[k, 2] = dc[s], dl[s]
            value[k, 3], nbits[k, 3] = ev, eb
    msb = np.tile(np.array([1, 0, 1, 0], np.int64), T)
    return _field_bits(value.reshape(-1), nbits.reshape(-1), msb)


def assemble(S, toks, ll, lc, dl, dc, head):
    """The zlib stream from its parts: header bits, token bits, end of block, padding, Adler-32."""
    bits = np.concatenate([np.array(head, np.uint8), token_bits(S, toks, ll, lc, dl, dc),
                           np.array(R.msb_first(lc[256], ll[256]), np.uint8)])
    return b"\x78\x01" + np.packbits(bits, bitorder="little").tobytes() + struct.pack(">I", R.adler32(S)), int(bits.size)


def lz_stream(frame):
    """(the zlib stream with matches as bytes, dict of the intermediate values)."""
    S = R.filtered_stream(frame)
    toks = tokens(frame)
    lh, dh = histograms(S, toks)
    ll, dl = code_sets(lh, dh)
    lc, dc = R.canonical(ll), R.canonical(dl)
    head = header_bit_list(ll, dl)
    data, nbits = assemble(S, toks, ll, lc, dl, dc, head)
    return data, dict(stream=S, tokens=toks, lhist=lh.astype(np.uint32), dhist=dh.astype(np.uint32), ll=ll, dl=dl, nbits=nbits,
                      header_bits=head)


def chosen_stream(frame):
    """(bytes, took the LZ stream, the LZ stream's intermediate values): the shorter of the two streams of a frame, the
    literal-only one where they are equally long."""
    lz, info = lz_stream(frame)
    lit = R.zlib_stream(frame)[0]
    return (lz, True, info) if len(lz) < len(lit) else (lit, False, info)


# ----------------------------------------------------------------------------- the frames of the tests
def far_frame(distance, length=200, seed=21):
    """Grey 40 x 1024 noise (rows of 1025 stream bytes) in which `length` pixels of row 2 come again `distance` stream bytes
    later, inside one row: source stream position 2150, target 2150 + distance."""
    frame = np.random.RandomState(seed).randint(0, 256, (40, 1024)).astype(np.uint8)
    src, dst = 2150, 2150 + distance
    r0, c0 = divmod(src, 1025)
    r1, c1 = divmod(dst, 1025)
    assert c0 >= 1 and c1 >= 1 and c0 + length <= 1025 and c1 + length <= 1025
    frame[r1, c1 - 1:c1 - 1 + length] = frame[r0, c0 - 1:c0 - 1 + length]
    return frame


def tile_repeat_frame(seed=22):
    """Grey 17 x 999 noise (17,000 stream bytes): the stream from byte 16,384 on, the second tile of 16 segments, repeats the
    stream from byte 0 on (616 bytes: row 0's filter byte and its first 615 pixels)."""
    frame = np.random.RandomState(seed).randint(1, 256, (17, 999)).astype(np.uint8)
    frame[16, 383] = 0
    frame[16, 384:] = frame[0, :615]
    S = R.filtered_stream(frame)
    assert S.size == 17000 and np.array_equal(S[16384:], S[:616])
    return frame


def lz_frames():
    """name -> frame: the smallest frames that can still break the LZ stage."""
    r = np.random.RandomState(17)
    small = R.small_frames()
    grey = r.randint(0, 256, (16, 24)).astype(np.uint8)
    k = np.arange(7 * 13)
    return {
        "grey_1x1": small["grey_1x1"],
        "rgb_3x5": small["rgb_3x5"],
        "zeros_64x64": np.zeros((64, 64), np.uint8),
        "period2_7x13": (5 + 37 * (k % 2)).astype(np.uint8).reshape(7, 13),
        "period3_7x13": (9 + 50 * (k % 3)).astype(np.uint8).reshape(7, 13),
        "replicated_16x24x3": np.stack([grey] * 3, axis=2),
        "far_32768": far_frame(32768),
        "far_32769": far_frame(32769),
        "tile_repeat_17000": tile_repeat_frame(),
        "fibonacci": R.fibonacci_frame(),
    }


def forced_lengths(n, deepest):
    """A complete prefix code over n symbols in which symbol `deepest` has 15 bits: lengths of the counts 1, 1, 2, 4 .. 2^13
    (a chain fifteen deep) and 2^14 for every other symbol."""
    other = [s for s in range(n) if s != deepest]
    freq = [1 << 14] * n
    freq[deepest] = 1
    freq[other[-1]] = 1
    for k, s in enumerate(other[-15:-1]):
        freq[s] = 2 << k
    out = R.code_lengths(freq, 15)
    assert out[deepest] == 15
    return out
