"""PNG files from uint8 frames that are already in device memory (csrc/png.hip): the GPU writes each frame's zlib stream as
one dynamic-Huffman deflate block of literals, the host supplies what is tiny (code lengths, header bits, offsets) and wraps
the streams as PNG.  Additive and opt-in (--device_png of gen_fake_espi.py, augment_preproc.py, predict_spnet.py and
evaluate_spnet.py); the default writers are Pillow's.

There is no LZ77 stage: a frame of sensor noise comes out close to Pillow's size, a smooth image several times larger.

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
"""
import heapq
import struct
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

NSYM = 257                      # 256 literals + end of block
EOB = 256
HEADER_WORDS = 64               # spnet_png_pack's header stride: 2048 bits >= 3 + 14 + 19 * 3 + 258 * 7
MAX_THREADS = 16
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


def block_header(lengths):
    """(bits as a Python int, bit i of the stream = bit i of the int; bit count) of the dynamic block's header."""
    lengths = [int(v) for v in lengths]
    if len(lengths) != NSYM:
        raise ValueError("png: the literal code has 257 lengths")
    rle = _run_length_code(lengths + [0])            # + the one distance code, of zero bits
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
    put(0, 5)                 # HLIT: 257 literal / length codes
    put(0, 5)                 # HDIST: 1 distance code
    put(hclen - 4, 4)
    for s in _CL_ORDER[:hclen]:
        put(cl_len[s], 3)
    for sym, nextra, extra in rle:
        put(_reverse(int(cl_code[sym]), cl_len[sym]), cl_len[sym])
        if nextra:
            put(extra, nextra)
    return acc, n


def header_words(lengths):
    """The header as spnet_png_pack reads it: uint32 [64] (bit i in bit i % 32 of word i // 32) and its bit count."""
    acc, n = block_header(lengths)
    return np.frombuffer(acc.to_bytes(HEADER_WORDS * 4, "little"), dtype="<u4").astype(np.uint32), n


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
        ln = huffman_code_lengths(hist[n])
        lengths[n] = ln
        codes[n] = (canonical_codes(ln) | (ln << 16)).astype(np.uint32)
        header[n], header_bits[n] = header_words(ln)
        bits = int(header_bits[n]) + int((hist[n] * ln[:256]).sum()) + int(ln[EOB])
        offsets[n + 1] = offsets[n] + 2 + (bits + 7) // 8 + 4
    return dict(lengths=lengths, codes=codes, header=header, header_bits=header_bits, offsets=offsets)


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


def pack_frames(frames, plan, adler, out=None, base=0):
    """Runs spnet_png_pack: the zlib streams of `frames` into `out` (a ZEROED uint8 device tensor whose size is a multiple of
    4; None: allocated exactly, rounded up to a whole word) from byte `base` on.  Returns out."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    offsets = plan["offsets"] + int(base)
    if out is None:
        out = torch.zeros(((int(offsets[-1]) + 3) // 4 * 4,), dtype=torch.uint8, device=frames.device)
    # one upload: offsets (64-bit) first, then the 32-bit arrays
    blob = np.concatenate([offsets.astype(np.int64).view(np.uint8), plan["codes"].reshape(-1).view(np.uint8),
                           plan["header"].reshape(-1).view(np.uint8), plan["header_bits"].view(np.uint8)])
    dev = torch.from_numpy(blob).to(frames.device)
    p = dev.data_ptr()
    p_codes = p + 8 * (N + 1)
    p_header = p_codes + 4 * NSYM * N
    p_bits = p_header + 4 * HEADER_WORDS * N
    with torch.cuda.device(frames.device):
        L.spnet_png_pack(frames.data_ptr(), N, H, W, channels, p_codes, p_header, p_bits, p, adler.data_ptr(), out.data_ptr(),
                         int(out.numel()), L.current_stream())
    return out


def zlib_streams_device(frames):
    """The zlib stream of every frame, as views of one host array."""
    N = _frames_shape(frames)[0]
    if N == 0:
        return []
    hist, adler = frame_statistics(frames)
    plan = plan_frames(hist)
    out = pack_frames(frames, plan, adler).cpu().numpy()
    off = plan["offsets"]
    return [out[int(off[n]):int(off[n + 1])] for n in range(N)]


def _pool_size(threads, jobs):
    return max(1, min(MAX_THREADS, int(threads), jobs))


def encode_png_device(frames, threads=MAX_THREADS):
    """PNG files of uint8 device frames [N,H,W] (grey) or [N,H,W,C] (C = 3: RGB), as a list of bytes."""
    N, H, W, channels = _frames_shape(frames)
    streams = zlib_streams_device(frames)
    if not streams:
        return []
    with ThreadPoolExecutor(max_workers=_pool_size(threads, N)) as pool:       # zlib.crc32 runs without the interpreter lock
        return list(pool.map(lambda z: png_container(z, W, H, channels), streams))


def _write_pieces(path, pieces):
    with open(path, "wb") as f:
        for piece in pieces:
            f.write(piece)
    return sum(len(piece) for piece in pieces)


def write_png_device(frames, paths, threads=MAX_THREADS, pool=None):
    """encode_png_device, written to `paths` by a thread pool of this process (at most 16 threads; nothing is forked).  pool:
    a caller's ThreadPoolExecutor to use instead.  Returns the size of every file."""
    N, H, W, channels = _frames_shape(frames)
    paths = list(paths)
    if len(paths) != N:
        raise ValueError("png: %d frames, %d paths" % (N, len(paths)))
    streams = zlib_streams_device(frames)
    if not streams:
        return []

    def job(k):
        return _write_pieces(paths[k], png_pieces(streams[k], W, H, channels))

    if pool is not None:
        return list(pool.map(job, range(N)))
    with ThreadPoolExecutor(max_workers=_pool_size(threads, N)) as own:
        return list(own.map(job, range(N)))
