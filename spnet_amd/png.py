"""PNG files from uint8 frames that are already in device memory (csrc/png.hip): the GPU writes each frame's zlib stream as
one dynamic-Huffman deflate block of literals, the host supplies what is tiny (code lengths, header bits, offsets) and wraps
the streams as PNG.  Additive and opt-in (--device_png of gen_fake_espi.py, augment_preproc.py, predict_spnet.py and
evaluate_spnet.py); the default writers are Pillow's.

By default there is no LZ77 stage: a frame of sensor noise comes out close to Pillow's size, a smooth image several times
larger.  lz77=True (--device_png_lz; csrc/png_lz.hip) adds one: spnet_png_lz_scan cuts every frame's stream into literals and
(length, distance) matches by a fixed rule (a function of the stream alone, written down in that file's header and in
DESIGN.md) and returns the literal/length and distance histograms; the host builds both codes, the header with real HLIT /
HDIST and the exact size, and KEEPS, PER FRAME, THE SMALLER of that stream and the literal-only one (equal: literal-only) --
both sizes are known before anything is packed.  spnet_png_lz_pack writes the frames that took LZ, spnet_png_pack the rest,
into the same zeroed buffer.  lz77=False writes the bytes it always wrote.

Per batch: spnet_png_hist -> D2H of the histograms -> code lengths / header / exact sizes on the host -> one H2D of the plan
-> spnet_png_pack -> D2H of the compressed bytes (each stream ends in its Adler-32).  The two D2H copies are the only
synchronisations.

The code construction is fixed, so that an independent restatement (tests/helpers/png_ref.py) gives the same bytes:
  lengths   Huffman over (count, order) with order = symbol for a leaf and n + k for the k-th merged node, the two smallest
            merged first; the number of codes of each depth is kept, depths beyond max_len are folded into max_len and the
            Kraft sum repaired one unit at a time (drop one max_len code, split the deepest shorter one); the lengths, shortest
            first, then go to the symbols ordered by (count descending, symbol ascending)
  codes     RFC 1951 section 3.2.2
  header    BFINAL 1, BTYPE 2, HLIT 0 (257 codes), HDIST 0 (one distance code, of zero bits: RFC 1951's all-literals case),
            the 258 lengths run-length coded greedily as ONE sequence (zeros: 18 while >= 11 remain, then 17 for 3 .. 10, else
            literal zeros; other values: the value, then 16 while >= 3 repeats remain, then the value), the code-length code
            built by the same procedure with max_len 7

Reading (csrc/png_decode.hip, csrc/inflate_core.h; opt-in --device_decode): parse_png takes the container apart on the host,
decode_png_device / read_png_device upload the zlib streams as they are, inflate and unfilter them on the GPU (any deflate
stream; 8-bit non-interlaced colour types 0 / 2 / 4 / 6) and leave every other file, and every file the kernels reject, to
the default path's Pillow call.
"""
import heapq
import struct
import zlib

import numpy as np

from .codec_host import MAX_THREADS, decode_batch, map_pool, read_file, stage, write_files

NSYM = 257                      # 256 literals + end of block
EOB = 256
HEADER_WORDS = 64               # spnet_png_pack's header stride: 2048 bits >= 3 + 14 + 19 * 3 + 258 * 7
NLL = 286                       # literal / length alphabet of the LZ77 stage
NDIST = 30                      # distance alphabet
LZ_HEADER_WORDS = 72            # spnet_png_lz_pack's header stride: 2304 bits >= 3 + 14 + 19 * 3 + 316 * 7
LENGTH_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)        # symbols 257 .. 285
DIST_EXTRA = tuple(max(0, k // 2 - 1) for k in range(NDIST))
PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"
COLOUR_TYPE = {1: 0, 2: 4, 3: 2, 4: 6}       # channels -> PNG colour type, 8 bits per sample
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


# ----------------------------------------------------------------------------- prefix codes
def _limited_lengths(freq, max_len):
    """Code length of every symbol of `freq` (0 where the count is 0): optimal where the Huffman tree is no deeper than
    max_len, a complete prefix code within max_len otherwise."""
    n = len(freq)
    used = [s for s in range(n) if freq[s] > 0]
    lengths = [0] * n
    if len(used) <= 1:
        for s in used:
            lengths[s] = 1
        return lengths
    if len(used) > (1 << max_len):
        raise ValueError("png: %d symbols do not fit a code of at most %d bits" % (len(used), max_len))
    parent = {}
    heap = [(int(freq[s]), s) for s in used]
    heapq.heapify(heap)
    node = n
    while len(heap) > 1:
        wa, a = heapq.heappop(heap)
        wb, b = heapq.heappop(heap)
        parent[a] = parent[b] = node
        heapq.heappush(heap, (wa + wb, node))
        node += 1
    depth = {node - 1: 0}
    for k in range(node - 2, n - 1, -1):          # merged nodes, children after parents
        depth[k] = depth[parent[k]] + 1
    count = [0] * (max(max_len, len(used)) + 2)
    for s in used:
        count[depth[parent[s]] + 1] += 1
    for d in range(max_len + 1, len(count)):      # too deep: fold into max_len, then repair the Kraft sum
        count[max_len] += count[d]
        count[d] = 0
    total = sum(count[d] << (max_len - d) for d in range(1, max_len + 1))
    while total > (1 << max_len):
        count[max_len] -= 1
        for d in range(max_len - 1, 0, -1):
            if count[d]:
                count[d] -= 1
                count[d + 1] += 2
                break
        total -= 1
    ranked = sorted(used, key=lambda s: (-int(freq[s]), s))
    i = 0
    for d in range(1, max_len + 1):
        for s in ranked[i:i + count[d]]:
            lengths[s] = d
        i += count[d]
    return lengths


def huffman_code_lengths(hist, max_len=15):
    """Lengths [257] of the literal / end-of-block code of a filtered stream with byte histogram hist [256]; the end-of-block
    symbol 256 has count 1, unused symbols get 0."""
    hist = np.asarray(hist).reshape(-1)
    if hist.shape[0] != 256:
        raise ValueError("png: a byte histogram has 256 bins")
    return np.array(_limited_lengths([int(c) for c in hist] + [1], max_len), dtype=np.int64)


def canonical_codes(lengths):
    """RFC 1951 section 3.2.2: codes of one length are consecutive in symbol order, shorter codes come first."""
    lengths = [int(v) for v in lengths]
    top = max(lengths) if lengths else 0
    bl_count = [0] * (top + 2)
    for v in lengths:
        if v:
            bl_count[v] += 1
    next_code = [0] * (top + 2)
    code = 0
    for bits in range(1, top + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    codes = [0] * len(lengths)
    for s, v in enumerate(lengths):
        if v:
            codes[s] = next_code[v]
            next_code[v] += 1
    return np.array(codes, dtype=np.int64)


def _reverse(code, nbits):
    r = 0
    for _ in range(nbits):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _run_length_code(seq):
    """[(code-length symbol, extra bits, extra value)] of a sequence of code lengths."""
    out = []
    i = 0
    while i < len(seq):
        v = seq[i]
        j = i
        while j < len(seq) and seq[j] == v:
            j += 1
        run = j - i
        i = j
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, 7, r - 11))
                run -= r
            if run >= 3:
                out.append((17, 3, run - 3))
                run = 0
        else:
            out.append((v, 0, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, 2, r - 3))
                run -= r
        out += [(v, 0, 0)] * run
    return out


def _dynamic_header(hlit, hdist, lengths):
    """(bits as a Python int, bit i of the stream = bit i of the int; bit count) of a dynamic block's header whose
    257 + hlit literal / length and 1 + hdist distance code lengths are `lengths`, run-length coded as one sequence."""
    rle = _run_length_code(lengths)
    cl_freq = [0] * 19
    for sym, _, _ in rle:
        cl_freq[sym] += 1
    cl_len = _limited_lengths(cl_freq, 7)
    cl_code = canonical_codes(cl_len)
    hclen = max(4, max(k + 1 for k, s in enumerate(_CL_ORDER) if cl_len[s]))
    acc, n = 0, 0

    def put(value, nbits):
        nonlocal acc, n
        acc |= value << n
        n += nbits

    put(1, 1)                 # BFINAL
    put(2, 2)                 # BTYPE = 10, dynamic Huffman
    put(hlit, 5)
    put(hdist, 5)
    put(hclen - 4, 4)
    for s in _CL_ORDER[:hclen]:
        put(cl_len[s], 3)
    for sym, nextra, extra in rle:
        put(_reverse(int(cl_code[sym]), cl_len[sym]), cl_len[sym])
        if nextra:
            put(extra, nextra)
    return acc, n


def block_header(lengths):
    """The literal-only block's header: HLIT 0 (257 literal / length codes), HDIST 0 (one distance code, of zero bits)."""
    lengths = [int(v) for v in lengths]
    if len(lengths) != NSYM:
        raise ValueError("png: the literal code has 257 lengths")
    return _dynamic_header(0, 0, lengths + [0])


def lz_block_header(ll, dl):
    """The LZ block's header from the literal / length lengths [286] and the distance lengths [30]: trailing unused symbols
    are not sent (HLIT, HDIST); no distance symbol used: one distance code of zero bits; one used: its length is 1 (RFC
    1951 section 3.2.7)."""
    ll, dl = [int(v) for v in ll], [int(v) for v in dl]
    if len(ll) != NLL or len(dl) != NDIST:
        raise ValueError("png: the LZ codes have 286 and 30 lengths")
    nl = max([NSYM] + [s + 1 for s in range(NSYM, NLL) if ll[s]])
    nd = max([1] + [s + 1 for s in range(NDIST) if dl[s]])
    return _dynamic_header(nl - 257, nd - 1, ll[:nl] + dl[:nd])


def _header_row(header, words):
    """A (bits as a Python int, bit count) header as a kernel reads it: uint32 [words] (bit i in bit i % 32 of word i // 32)
    and the bit count."""
    acc, n = header
    return np.frombuffer(acc.to_bytes(words * 4, "little"), dtype="<u4").astype(np.uint32), n


def header_words(lengths):
    """The header as spnet_png_pack reads it: uint32 [64] and its bit count."""
    return _header_row(block_header(lengths), HEADER_WORDS)


def _code_set(counts):
    """(lengths int64, codes uint32 as the kernels read them: canonical code | length << 16) of a symbol histogram."""
    ln = np.array(_limited_lengths([int(c) for c in counts], 15), dtype=np.int64)
    return ln, (canonical_codes(ln) | (ln << 16)).astype(np.uint32)


def _zlib_size(bits):
    """Bytes of a zlib stream whose one deflate block has `bits` bits: 2 of header, the block, 4 of Adler-32."""
    return 2 + (int(bits) + 7) // 8 + 4


def plan_frames(hist):
    """Everything spnet_png_pack needs beyond the pixels, from the histograms [N][256] of the filtered streams: lengths
    [N][257], codes [N][257] uint32 (canonical code | length << 16), header [N][64] uint32, header_bits [N] int32, offsets
    [N + 1] int64 (frame n's zlib stream is bytes offsets[n] .. offsets[n+1] - 1: exact, nothing is guessed)."""
    hist = np.asarray(hist).reshape(-1, 256).astype(np.int64)
    N = hist.shape[0]
    lengths = np.zeros((N, NSYM), np.int64)
    codes = np.zeros((N, NSYM), np.uint32)
    header = np.zeros((N, HEADER_WORDS), np.uint32)
    header_bits = np.zeros(N, np.int32)
    offsets = np.zeros(N + 1, np.int64)
    for n in range(N):
        ln, codes[n] = _code_set(list(hist[n]) + [1])                    # the end of block, once
        lengths[n] = ln
        header[n], header_bits[n] = header_words(ln)
        bits = int(header_bits[n]) + int((hist[n] * ln[:256]).sum()) + int(ln[EOB])
        offsets[n + 1] = offsets[n] + _zlib_size(bits)
    return dict(lengths=lengths, codes=codes, header=header, header_bits=header_bits, offsets=offsets)


def plan_frames_lz(hist, lhist, dhist):
    """The plan of a batch with the LZ77 stage on, from the byte histograms [N][256], the literal / length histograms
    [N][286] (end of block counted) and the distance histograms [N][30]: the literal-only plan (`literal`: plan_frames'
    dict), both LZ code sets (lcodes [N][286], dcodes [N][30]: code | length << 16; llengths, dlengths), lz_header
    [N][72], lz_header_bits [N] int32 (-1 for a frame that stays literal-only: spnet_png_lz_pack skips it), the exact sizes
    of both streams (lz_sizes, literal_sizes), use_lz [N] (the LZ stream is strictly smaller) and offsets [N + 1] of the
    chosen streams."""
    hist = np.asarray(hist).reshape(-1, 256).astype(np.int64)
    lhist = np.asarray(lhist).reshape(-1, NLL).astype(np.int64)
    dhist = np.asarray(dhist).reshape(-1, NDIST).astype(np.int64)
    N = hist.shape[0]
    if lhist.shape[0] != N or dhist.shape[0] != N:
        raise ValueError("png: histograms of %d, %d and %d frames" % (N, lhist.shape[0], dhist.shape[0]))
    literal = plan_frames(hist)
    literal_sizes = np.diff(literal["offsets"])
    llengths = np.zeros((N, NLL), np.int64)
    dlengths = np.zeros((N, NDIST), np.int64)
    lcodes = np.zeros((N, NLL), np.uint32)
    dcodes = np.zeros((N, NDIST), np.uint32)
    header = np.zeros((N, LZ_HEADER_WORDS), np.uint32)
    header_bits = np.zeros(N, np.int32)
    lz_sizes = np.zeros(N, np.int64)
    lextra = np.array(LENGTH_EXTRA, np.int64)
    dextra = np.array(DIST_EXTRA, np.int64)
    for n in range(N):
        ll, lcodes[n] = _code_set(lhist[n])
        dl, dcodes[n] = _code_set(dhist[n])
        llengths[n], dlengths[n] = ll, dl
        header[n], header_bits[n] = _header_row(lz_block_header(ll, dl), LZ_HEADER_WORDS)
        bits = (int(header_bits[n]) + int((lhist[n] * ll).sum()) + int((dhist[n] * dl).sum())
                + int((lhist[n, NSYM:] * lextra).sum()) + int((dhist[n] * dextra).sum()))
        lz_sizes[n] = _zlib_size(bits)
    use_lz = lz_sizes < literal_sizes
    offsets = np.zeros(N + 1, np.int64)
    np.cumsum(np.where(use_lz, lz_sizes, literal_sizes), out=offsets[1:])
    return dict(literal=literal, llengths=llengths, dlengths=dlengths, lcodes=lcodes, dcodes=dcodes, lz_header=header,
                lz_header_bits=np.where(use_lz, header_bits, -1).astype(np.int32), lz_sizes=lz_sizes,
                literal_sizes=literal_sizes, use_lz=use_lz, offsets=offsets)


# ----------------------------------------------------------------------------- container
def _chunk_head(tag, data_len):
    return struct.pack(">I", data_len) + tag


def _chunk(tag, data):
    return _chunk_head(tag, len(data)) + data + struct.pack(">I", zlib.crc32(data, zlib.crc32(tag)))


def png_pieces(zstream, width, height, channels):
    """The file as three byte strings (everything before the IDAT data, the data, everything after): signature, IHDR, one
    IDAT holding the zlib stream, IEND."""
    ihdr = struct.pack(">IIBBBBB", width, height, 8, COLOUR_TYPE[channels], 0, 0, 0)
    crc = zlib.crc32(zstream, zlib.crc32(b"IDAT"))
    return (PNG_SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk_head(b"IDAT", len(zstream)), zstream,
            struct.pack(">I", crc) + _chunk(b"IEND", b""))


def png_container(zstream, width, height, channels):
    return b"".join(png_pieces(zstream, width, height, channels))


# ----------------------------------------------------------------------------- device
def _frames_shape(frames):
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8):
        raise ValueError("png: frames must be a uint8 tensor in device memory (there is no CPU encoder here)")
    if frames.dim() == 3:
        channels = 1
    elif frames.dim() == 4 and int(frames.shape[3]) in COLOUR_TYPE:
        channels = int(frames.shape[3])
    else:
        raise ValueError("png: frames are [N,H,W] or [N,H,W,C] with C in 1..4, got %s" % (tuple(frames.shape),))
    N, H, W = (int(v) for v in frames.shape[:3])
    if N and (H < 1 or W < 1):
        raise ValueError("png: empty frames")
    return N, H, W, channels


def frame_statistics(frames):
    """(hist [N][256] as a host uint32 array, adler [N] as a DEVICE int32 tensor) of the filtered streams: one launch, one
    D2H copy."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    hist = torch.empty((N, 256), dtype=torch.int32, device=frames.device)
    adler = torch.empty((N,), dtype=torch.int32, device=frames.device)
    with torch.cuda.device(frames.device):
        L.spnet_png_hist(frames.data_ptr(), N, H, W, channels, hist.data_ptr(), adler.data_ptr(), L.current_stream())
    return hist.cpu().numpy().view(np.uint32), adler


def _upload(arrays, device):
    """The arrays as ONE host-to-device copy (pageable, blocking), every one 16-byte aligned: (the device tensor that owns
    the bytes, the device pointer of every array)."""
    dev, starts, _ = stage(arrays, device, pinned=False, align=16)
    return dev, [dev.data_ptr() + s for s in starts]


def pack_frames(frames, plan, adler, out=None, base=0):
    """Runs spnet_png_pack: the zlib streams of `frames` into `out` (a ZEROED uint8 device tensor whose size is a multiple of
    4; None: allocated exactly, rounded up to a whole word) from byte `base` on.  Returns out."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    offsets = (plan["offsets"] + int(base)).astype(np.int64)
    if out is None:
        out = torch.zeros(((int(offsets[-1]) + 3) // 4 * 4,), dtype=torch.uint8, device=frames.device)
    dev, (p_off, p_codes, p_header, p_bits) = _upload([offsets, plan["codes"], plan["header"], plan["header_bits"]],
                                                      frames.device)
    with torch.cuda.device(frames.device):
        L.spnet_png_pack(frames.data_ptr(), N, H, W, channels, p_codes, p_header, p_bits, p_off, adler.data_ptr(),
                         out.data_ptr(), int(out.numel()), L.current_stream())
    return out


def lz_statistics(frames):
    """(lhist [N][286], dhist [N][30]) of the frames' tokens (spnet_png_lz_scan), as host uint32 arrays: one launch, one D2H
    copy."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    both = torch.empty((N * (NLL + NDIST),), dtype=torch.int32, device=frames.device)
    with torch.cuda.device(frames.device):
        L.spnet_png_lz_scan(frames.data_ptr(), N, H, W, channels, both.data_ptr(), both.data_ptr() + 4 * NLL * N,
                            L.current_stream())
    host = both.cpu().numpy().view(np.uint32)
    return host[:N * NLL].reshape(N, NLL), host[N * NLL:].reshape(N, NDIST)


def pack_frames_lz(frames, plan, adler, out=None, base=0):
    """pack_frames for a plan_frames_lz plan: spnet_png_lz_pack writes the frames that took the LZ stream, spnet_png_pack
    every run of neighbouring frames that stayed literal-only, into the same ZEROED buffer."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    offsets = (plan["offsets"] + int(base)).astype(np.int64)
    if out is None:
        out = torch.zeros(((int(offsets[-1]) + 3) // 4 * 4,), dtype=torch.uint8, device=frames.device)
    lit = plan["literal"]
    dev, (p_off, p_lc, p_dc, p_lh, p_lb, p_c, p_h, p_b) = _upload(
        [offsets, plan["lcodes"], plan["dcodes"], plan["lz_header"], plan["lz_header_bits"], lit["codes"], lit["header"],
         lit["header_bits"]], frames.device)
    use = plan["use_lz"]
    frame_bytes = H * W * channels
    with torch.cuda.device(frames.device):
        if use.any():
            L.spnet_png_lz_pack(frames.data_ptr(), N, H, W, channels, p_lc, p_dc, p_lh, p_lb, p_off, adler.data_ptr(),
                                out.data_ptr(), int(out.numel()), L.current_stream())
        lo = 0
        while lo < N:
            if use[lo]:
                lo += 1
                continue
            hi = lo
            while hi < N and not use[hi]:
                hi += 1
            L.spnet_png_pack(frames.data_ptr() + lo * frame_bytes, hi - lo, H, W, channels, p_c + 4 * NSYM * lo,
                             p_h + 4 * HEADER_WORDS * lo, p_b + 4 * lo, p_off + 8 * lo, adler.data_ptr() + 4 * lo,
                             out.data_ptr(), int(out.numel()), L.current_stream())
            lo = hi
    return out


def zlib_streams_device(frames, lz77=False):
    """The zlib stream of every frame, as views of one host array.  lz77: with the LZ77 stage (per frame the smaller of the
    LZ stream and the literal-only one)."""
    N = _frames_shape(frames)[0]
    if N == 0:
        return []
    hist, adler = frame_statistics(frames)
    if lz77:
        lhist, dhist = lz_statistics(frames)
        plan = plan_frames_lz(hist, lhist, dhist)
        out = pack_frames_lz(frames, plan, adler).cpu().numpy()
    else:
        plan = plan_frames(hist)
        out = pack_frames(frames, plan, adler).cpu().numpy()
    off = plan["offsets"]
    return [out[int(off[n]):int(off[n + 1])] for n in range(N)]


def encode_png_device(frames, threads=MAX_THREADS, lz77=False):
    """PNG files of uint8 device frames [N,H,W] (grey) or [N,H,W,C] (C = 3: RGB), as a list of bytes.  lz77: see
    zlib_streams_device."""
    N, H, W, channels = _frames_shape(frames)
    streams = zlib_streams_device(frames, lz77=lz77)
    return map_pool(lambda z: png_container(z, W, H, channels), streams, threads)      # zlib.crc32 runs without the lock


def write_png_device(frames, paths, threads=MAX_THREADS, pool=None, lz77=False):
    """encode_png_device, written to `paths` by a thread pool of this process (at most 16 threads; nothing is forked).  pool:
    a caller's ThreadPoolExecutor to use instead.  Returns the size of every file."""
    N, H, W, channels = _frames_shape(frames)

    def encode():
        streams = zlib_streams_device(frames, lz77=lz77)
        return lambda k: png_pieces(streams[k], W, H, channels)

    return write_files(paths, N, encode, threads, pool, "png")


# ----------------------------------------------------------------------------- reading: container
MAX_STREAM = 1 << 27            # spnet_png_inflate: L = H * (1 + W * channels)
MAX_ROW = 32768                 # spnet_png_unfilter: W * channels
MAX_ZSTREAM = 1 << 30           # spnet_png_inflate: compressed bytes of one file
CHANNELS = {0: 1, 4: 2, 2: 3, 6: 4}          # PNG colour type -> channels, 8 bits per sample
STATUS_NAMES = ("ok", "bad zlib header", "reserved block type", "LEN/NLEN mismatch", "over-subscribed or incomplete code",
                "invalid symbol", "distance too far", "input exhausted", "output longer than expected",
                "output shorter than expected", "Adler-32 mismatch", "filter type above 4", "extent outside the blob")


class PngInfo:
    """What parse_png found.  width, height, bit_depth, colour_type, interlace: IHDR's (None where IHDR could not be
    read); trns: a tRNS chunk was seen; zstream: the IDAT payloads, concatenated; channels: bytes per pixel of a file the
    device takes; host_reason: None for a file the device decodes, else why the host has to (str)."""
    __slots__ = ("width", "height", "bit_depth", "colour_type", "interlace", "trns", "zstream", "channels", "host_reason")

    def __init__(self):
        self.width = self.height = self.bit_depth = self.colour_type = self.interlace = self.channels = None
        self.trns = False
        self.zstream = b""
        self.host_reason = None

    @property
    def device(self):
        return self.host_reason is None


def parse_png(data):
    """The container reader, the inverse of png_pieces: signature, IHDR, the payloads of all IDAT chunks in order, the CRC
    of every chunk (the content of ancillary chunks is skipped), up to IEND.  Raises nothing: a file the device cannot take
    (8 bits, colour type 0 / 2 / 4 / 6, not interlaced, no tRNS, within the kernels' sizes is what it takes), a damaged
    container included, comes back with host_reason set and is left to the host decoder, which decides what it is."""
    info = PngInfo()
    data = memoryview(data)
    n = len(data)
    if n < 8 or bytes(data[:8]) != PNG_SIGNATURE:
        info.host_reason = "no PNG signature"
        return info
    pos = 8
    idat = []
    ended = False
    first = True
    while pos + 12 <= n:
        length, = struct.unpack(">I", data[pos:pos + 4])
        tag = bytes(data[pos + 4:pos + 8])
        if pos + 12 + length > n:
            info.host_reason = "chunk %r runs past the end of the file" % tag
            return info
        body = data[pos + 8:pos + 8 + length]
        critical = not (tag[0] & 0x20)
        crc, = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        if zlib.crc32(body, zlib.crc32(tag)) != crc:           # (of an ancillary chunk too: the default decoder raises on it)
            info.host_reason = "CRC of chunk %r" % tag
            return info
        pos += 12 + length
        if first != (tag == b"IHDR"):
            info.host_reason = "IHDR is not the first chunk" if first else "a second IHDR"
            return info
        first = False
        if tag == b"IHDR":
            if length != 13:
                info.host_reason = "IHDR of %d bytes" % length
                return info
            (info.width, info.height, info.bit_depth, info.colour_type, compression, filt,
             info.interlace) = struct.unpack(">IIBBBBB", body)
            if compression or filt:
                info.host_reason = "compression / filter method %d / %d" % (compression, filt)
        elif tag == b"IDAT":
            idat.append(body)
        elif tag == b"tRNS":
            info.trns = True
        elif tag == b"IEND":
            ended = True
            break
        elif critical and tag != b"PLTE":        # (a palette may accompany colour types 2 and 6 as a suggestion)
            info.host_reason = info.host_reason or "critical chunk %r" % tag
    info.zstream = idat[0] if len(idat) == 1 else b"".join(idat)
    if info.host_reason is not None:
        return info
    if info.width is None or not ended:
        info.host_reason = "no IEND"
    elif info.bit_depth != 8:
        info.host_reason = "bit depth %d" % info.bit_depth
    elif info.colour_type not in CHANNELS:
        info.host_reason = "colour type %d" % info.colour_type
    elif info.interlace:
        info.host_reason = "interlaced"
    elif info.trns:
        info.host_reason = "tRNS"
    elif info.width < 1 or info.height < 1:
        info.host_reason = "empty image"
    else:
        info.channels = CHANNELS[info.colour_type]
        if info.width * info.channels > MAX_ROW or info.height * (1 + info.width * info.channels) > MAX_STREAM:
            info.host_reason = "larger than the device decoder's budget"
        elif len(info.zstream) > MAX_ZSTREAM:
            info.host_reason = "compressed stream larger than the device decoder's budget"
    return info


# ----------------------------------------------------------------------------- reading: device
def inflate_unfilter_device(blob, offsets, N, H, W, channels, first=None, full=None):
    """The two launches on uploaded streams: blob (uint8 device tensor), offsets (int64 device tensor [N + 1], positions in
    blob).  first [N,H,W] / full [N,H,W,channels]: uint8 device tensors to fill (either may be None).  Returns status, an
    int32 DEVICE tensor [N]; nothing is synchronised."""
    import torch
    from . import _lib as L
    length = H * (1 + W * channels)
    inflated = torch.empty((N, length), dtype=torch.uint8, device=blob.device)
    status = torch.empty((N,), dtype=torch.int32, device=blob.device)
    with torch.cuda.device(blob.device):
        L.spnet_png_inflate(blob.data_ptr(), int(blob.numel()), offsets.data_ptr(), N, length, length, inflated.data_ptr(),
                            status.data_ptr(), L.current_stream())
        L.spnet_png_unfilter(inflated.data_ptr(), length, N, H, W, channels, 0 if first is None else first.data_ptr(),
                             0 if full is None else full.data_ptr(), status.data_ptr(), L.current_stream())
    return status


def decode_parsed_png(infos, sources, device=None, channels="first", return_info=False):
    """decode_png_device of files that are already parsed: infos[k] = parse_png of the file sources[k] (bytes, or a path
    for the host decoder to open)."""
    import torch

    def launch(idx, shape, out, device):
        H, W = shape[:2]
        groups = {}                                  # bytes per pixel -> files: one pair of launches each
        for k in idx:
            groups.setdefault(infos[k].channels, []).append(k)
        pending = []
        for bpp, ks in groups.items():
            n = len(ks)
            streams = [np.frombuffer(infos[k].zstream, np.uint8) for k in ks]
            offsets = np.zeros(n + 1, np.int64)      # relative to the start of the streams
            np.cumsum([v.size for v in streams], out=offsets[1:])
            # one pinned upload: the offsets (64-bit) first, then the streams back to back
            dev, _, staging = stage([offsets] + streams, device, pinned=True, align=1)
            head = 8 * (n + 1)
            got = out if n == len(out) else torch.empty((n,) + shape, dtype=torch.uint8, device=device)
            st = inflate_unfilter_device(dev[head:], dev[:head].view(torch.int64), n, H, W, bpp,
                                         **{"first" if channels == "first" else "full": got})
            pending.append((ks, st, got, staging))
        return pending, ()

    return decode_batch(infos, sources, device, channels, return_info, "png", lambda info: info.channels, launch)


def decode_png_device(datas, device=None, channels="first", return_info=False, threads=MAX_THREADS):
    """PNG files (a list of bytes) -> a uint8 DEVICE tensor [N,H,W] holding channel 0 of every pixel (what
    utils._load_one(..., as_uint8=True) keeps: the grey level, or R), or [N,H,W,C] with channels="all".  The compressed
    bytes are uploaded as they are and inflated and unfiltered on the GPU.  Files the device does not take (see parse_png)
    and files it rejects (status != 0) are decoded by the default path's Pillow call and uploaded into their place, so the
    pixels are the default path's in every case and a corrupt file raises what it raises there.  All files of a call
    have one size (ValueError otherwise).  return_info: also the status array (inflate_core.h's codes, STATUS_NAMES) and
    the sorted indices of the files the host decoded."""
    datas = list(datas)
    return decode_parsed_png(map_pool(parse_png, datas, threads), datas, device, channels, return_info)  # crc32: no lock


def parse_png_file(path):
    return parse_png(read_file(path))


def read_png_device(paths, threads=MAX_THREADS, device=None, channels="first", return_info=False):
    """decode_png_device of files on disk, read and parsed by a thread pool of this process (at most 16 threads; nothing
    is forked)."""
    paths = list(paths)
    return decode_parsed_png(map_pool(parse_png_file, paths, threads), paths, device, channels, return_info)
