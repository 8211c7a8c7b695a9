"""JPEG files and a Motion-JPEG movie from uint8 frames that are already in device memory (csrc/jpeg.hip).  Additive and
opt-in (--device_jpeg / --movie of predict_spnet.py and evaluate_spnet.py); every default writer stays Pillow / PNG, and the
data-set writers stay lossless (the loaders glob *.png).

Format: baseline sequential DCT (SOF0), 8 bit, JFIF APP0; one component for grey frames, YCbCr 4:4:4 (three components,
interleaved MCUs of Y, Cb, Cr, no subsampling) for RGB frames.  Quantisation tables: the Annex K base tables scaled by the
libjpeg quality rule (quant_tables).  Huffman tables: the four Annex K "typical" tables, written into every file's DHT; they
are fixed, so nothing but ONE array of sizes crosses to the host between the two launches.

The scan is cut into restart intervals of restart_interval(width, channels) = min(ceil(width / 8), 64) MCUs (a DRI segment;
RSTm between intervals, m counting mod 8, none after the last).  An interval is byte aligned and resets the DC predictors:
the unit of parallel work (one wave per interval, one lane per MCU).  The arithmetic (colour transform, DCT, quantisation)
is integer only and written down once, beside the prototypes in include/spnet_hip.h and in DESIGN.md section 5e;
tests/helpers/jpeg_ref.py restates it in numpy and the device's bytes equal its bytes.

Per batch: spnet_jpeg_scan -> D2H of the interval sizes -> per-frame offsets (exact) -> spnet_jpeg_pack (which recomputes
the coefficients: no HBM workspace) -> D2H of the scans.  The host wraps each scan in the header (SOI, APP0, DQT, SOF0, DHT,
DRI, SOS; the same for every frame of a batch) and the trailer (EOI).

MjpegWriter streams such files into a plain RIFF AVI (hdrl / movi of 00dc chunks / idx1; 32-bit sizes, below 2 GiB).
"""
import struct
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np

MAX_THREADS = 16
MAX_DIM = 65535                 # SOF0 holds 16-bit sizes
MAX_INTERVAL = 64               # MCUs of a restart interval: one lane of a wave each

# ----------------------------------------------------------------------------- tables of the standard (ITU-T T.81 Annex K)
# natural (row-major) order, v * 8 + u
LUMINANCE_BASE = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                  14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
CHROMINANCE_BASE = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                    47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
# ZIGZAG[k] = natural index of the k-th coefficient of the zigzag sequence
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
          54, 47, 55, 62, 63)
# (BITS: number of codes of length 1 .. 16; HUFFVAL: the symbols in code order)
DC_LUMINANCE = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMINANCE = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMINANCE = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d), tuple(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMINANCE = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77), tuple(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))
# (table class: 0 DC, 1 AC; destination: 0 luminance, 1 chrominance; the table)
HUFFMAN_TABLES = ((0, 0, DC_LUMINANCE), (1, 0, AC_LUMINANCE), (0, 1, DC_CHROMINANCE), (1, 1, AC_CHROMINANCE))
JPEG_TRAILER = b"\xff\xd9"      # EOI


def huffman_codes(table):
    """{symbol: (code, length)} of a (BITS, HUFFVAL) table: codes of one length are consecutive in HUFFVAL order, the first
    code of a length is twice the one after the last of the length before (T.81 Annex C)."""
    bits, vals = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def quant_tables(quality=90):
    """uint16 [2][64], natural order: the luminance and chrominance tables of `quality` (1 .. 100) by the libjpeg rule:
    scale = 5000 // q below 50, else 200 - 2 q; every entry clamp((base * scale + 50) // 100, 1, 255)."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError("jpeg: quality is an integer 1 .. 100, got %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([LUMINANCE_BASE, CHROMINANCE_BASE], np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


def restart_interval(width, channels=1):
    """MCUs of a restart interval: one MCU row, capped at 64.  A function of (width, channels) only (and, as it stands, not
    of channels: an MCU is one 8 x 8 block of every component)."""
    if channels not in (1, 3):
        raise ValueError("jpeg: channels is 1 (grey) or 3 (RGB), got %r" % (channels,))
    return min((int(width) + 7) // 8, MAX_INTERVAL)


def intervals(height, width, channels=1):
    """Restart intervals of one frame's scan."""
    mcus = ((int(height) + 7) // 8) * ((int(width) + 7) // 8)
    ri = restart_interval(width, channels)
    return (mcus + ri - 1) // ri


# ----------------------------------------------------------------------------- container
def _segment(marker, data):
    return b"\xff" + bytes([marker]) + struct.pack(">H", len(data) + 2) + data


def jpeg_header(width, height, channels, quality=90, restart_interval=None):
    """Everything before the entropy-coded data: SOI, APP0 (JFIF 1.01, no density unit, 1:1), DQT (one segment: table 0,
    and table 1 for colour, in zigzag order), SOF0 (the TRUE size), DHT (one segment: DC and AC table 0, and DC and AC
    table 1 for colour), DRI, SOS.  restart_interval None: this module's rule."""
    width, height = int(width), int(height)
    if channels not in (1, 3):
        raise ValueError("jpeg: channels is 1 (grey) or 3 (RGB), got %r" % (channels,))
    if not (1 <= width <= MAX_DIM and 1 <= height <= MAX_DIM):
        raise ValueError("jpeg: a frame is 1 .. 65535 pixels wide and high, got %d x %d" % (width, height))
    ri = globals()["restart_interval"](width, channels) if restart_interval is None else int(restart_interval)
    if not 1 <= ri <= 65535:
        raise ValueError("jpeg: a restart interval is 1 .. 65535 MCUs, got %d" % ri)
    qt = quant_tables(quality)
    ntab = 1 if channels == 1 else 2
    out = [b"\xff\xd8", _segment(0xE0, b"JFIF\x00\x01\x01\x00" + struct.pack(">HHBB", 1, 1, 0, 0))]
    out.append(_segment(0xDB, b"".join(bytes([t]) + bytes(int(qt[t][ZIGZAG[k]]) for k in range(64)) for t in range(ntab))))
    comps = b"".join(bytes([c + 1, 0x11, 0 if c == 0 else 1]) for c in range(channels))
    out.append(_segment(0xC0, struct.pack(">BHHB", 8, height, width, channels) + comps))
    out.append(_segment(0xC4, b"".join(bytes([cls << 4 | dest]) + bytes(tab[0]) + bytes(tab[1])
                                       for cls, dest, tab in HUFFMAN_TABLES if dest < ntab)))
    out.append(_segment(0xDD, struct.pack(">H", ri)))
    scan = b"".join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in range(channels))
    out.append(_segment(0xDA, bytes([channels]) + scan + b"\x00\x3f\x00"))
    return b"".join(out)


def jpeg_pieces(scan, width, height, channels, quality=90):
    """The file as three byte strings: header, the scan (entropy-coded intervals and RST markers), trailer."""
    return jpeg_header(width, height, channels, quality), scan, JPEG_TRAILER


# ----------------------------------------------------------------------------- device
def _frames_shape(frames):
    import torch
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.uint8):
        raise ValueError("jpeg: frames must be a uint8 tensor in device memory (there is no CPU encoder here)")
    if frames.dim() == 3:
        channels = 1
    elif frames.dim() == 4 and int(frames.shape[3]) in (1, 3):
        channels = int(frames.shape[3])
    else:
        raise ValueError("jpeg: frames are [N,H,W] (grey) or [N,H,W,C] with C = 1 or 3 (RGB), got %s" % (tuple(frames.shape),))
    N, H, W = (int(v) for v in frames.shape[:3])
    if N and not (1 <= H <= MAX_DIM and 1 <= W <= MAX_DIM):
        raise ValueError("jpeg: a frame is 1 .. 65535 pixels wide and high, got %d x %d" % (W, H))
    return N, H, W, channels


def _need_gpu(what):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("jpeg: %s encodes on the GPU (there is no CPU encoder here)" % what)


def _device_tables(quality, device):
    import torch
    return torch.from_numpy(quant_tables(quality).view(np.int16).copy()).to(device)


def interval_sizes(frames, quality=90):
    """(sizes [N][intervals] as a host uint32 array: the bytes of every restart interval's entropy-coded data, stuffing and
    final padding included, markers excluded; the same array as a DEVICE int32 tensor, which spnet_jpeg_pack reads): one
    launch, one D2H copy."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    ni = intervals(H, W, channels)
    sizes = torch.empty((N, ni), dtype=torch.int32, device=frames.device)
    qt = _device_tables(quality, frames.device)
    with torch.cuda.device(frames.device):
        L.spnet_jpeg_scan(frames.data_ptr(), N, H, W, channels, qt.data_ptr(), sizes.data_ptr(), L.current_stream())
    return sizes.cpu().numpy().view(np.uint32), sizes


def scan_offsets(sizes):
    """int64 [N + 1]: frame n's scan is bytes offsets[n] .. offsets[n+1] - 1: its intervals and the 2-byte RST marker between
    any two of them."""
    sizes = np.asarray(sizes).astype(np.int64)
    offsets = np.zeros(sizes.shape[0] + 1, np.int64)
    np.cumsum(sizes.sum(axis=1) + 2 * (sizes.shape[1] - 1), out=offsets[1:])
    return offsets


def pack_frames(frames, sizes_dev, offsets, quality=90, out=None):
    """Runs spnet_jpeg_pack: the scans of `frames` into `out` (a uint8 device tensor; None: allocated exactly) at the byte
    offsets [N + 1].  Returns out."""
    import torch
    from . import _lib as L
    N, H, W, channels = _frames_shape(frames)
    frames = frames.contiguous()
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if out is None:
        out = torch.empty((int(offsets[-1]),), dtype=torch.uint8, device=frames.device)
    off = torch.from_numpy(offsets).to(frames.device)
    qt = _device_tables(quality, frames.device)
    with torch.cuda.device(frames.device):
        L.spnet_jpeg_pack(frames.data_ptr(), N, H, W, channels, qt.data_ptr(), sizes_dev.data_ptr(), off.data_ptr(),
                          out.data_ptr(), int(out.numel()), L.current_stream())
    return out


def scans_device(frames, quality=90):
    """The scan of every frame, as views of one host array."""
    N = _frames_shape(frames)[0]
    if N == 0:
        return []
    sizes, sizes_dev = interval_sizes(frames, quality)
    off = scan_offsets(sizes)
    out = pack_frames(frames, sizes_dev, off, quality).cpu().numpy()
    return [out[int(off[n]):int(off[n + 1])] for n in range(N)]


def _pool_size(threads, jobs):
    return max(1, min(MAX_THREADS, int(threads), jobs))


def encode_jpeg_device(frames, quality=90):
    """JPEG files of uint8 device frames [N,H,W] (grey) or [N,H,W,C] (C = 3: RGB), as a list of bytes."""
    _need_gpu("encode_jpeg_device")
    N, H, W, channels = _frames_shape(frames)
    scans = scans_device(frames, quality)
    if not scans:
        return []
    header = jpeg_header(W, H, channels, quality)
    return [header + s.tobytes() + JPEG_TRAILER for s in scans]


def write_jpeg_device(frames, paths, quality=90, threads=MAX_THREADS, pool=None):
    """encode_jpeg_device, written to `paths` by a thread pool of this process (at most 16 threads; nothing is forked).
    pool: a caller's ThreadPoolExecutor to use instead.  Returns the size of every file."""
    _need_gpu("write_jpeg_device")
    N, H, W, channels = _frames_shape(frames)
    paths = list(paths)
    if len(paths) != N:
        raise ValueError("jpeg: %d frames, %d paths" % (N, len(paths)))
    scans = scans_device(frames, quality)
    if not scans:
        return []
    header = jpeg_header(W, H, channels, quality)

    def job(k):
        with open(paths[k], "wb") as f:
            f.write(header)
            f.write(scans[k])
            f.write(JPEG_TRAILER)
        return len(header) + len(scans[k]) + len(JPEG_TRAILER)

    if pool is not None:
        return list(pool.map(job, range(N)))
    with ThreadPoolExecutor(max_workers=_pool_size(threads, N)) as own:
        return list(own.map(job, range(N)))


# ----------------------------------------------------------------------------- Motion-JPEG in a RIFF AVI
RIFF_LIMIT = (1 << 31) - 1      # the file never passes this many bytes (32-bit sizes, signed in many readers; no OpenDML)
_AVIF_HASINDEX = 0x10
_AVIIF_KEYFRAME = 0x10
_HDRL_BYTES = 4 + (8 + 56) + (8 + 4 + (8 + 56) + (8 + 40))      # 'hdrl', avih, LIST strl (strh, strf)
_MOVI_LIST_AT = 12 + 8 + _HDRL_BYTES                            # file position of the movi LIST's header


class MjpegWriter:
    """A Motion-JPEG movie: every frame one complete JPEG file in a 00dc chunk of a plain RIFF AVI.

      RIFF 'AVI '  LIST 'hdrl' ( avih  LIST 'strl' ( strh: vids / MJPG, dwRate / dwScale = fps as a rational
                                                     strf: BITMAPINFOHEADER, biCompression MJPG ) )
                   LIST 'movi' ( 00dc ... )            chunks padded to even length
                   idx1                                one entry per frame, offsets counted from the 'movi' tag

    add(frames) encodes uint8 device frames [n,H,W] / [n,H,W,C] on the GPU and appends them in order; nothing but one
    call's frames and 16 index bytes per frame written so far is held.  Sizes and frame counts are patched by close().
    RIFF sizes are 32-bit: add raises ValueError before the file would pass 2 GiB - 1 (OpenDML is not written).
    encoder (for tests and other producers): a callable frames -> list of JPEG files (bytes) used instead of
    encode_jpeg_device."""

    def __init__(self, path, width, height, fps=5.0, channels=3, quality=90, encoder=None):
        self.width, self.height, self.channels, self.quality = int(width), int(height), int(channels), int(quality)
        if self.channels not in (1, 3):
            raise ValueError("mjpeg: channels is 1 (grey) or 3 (RGB), got %r" % (channels,))
        if not (1 <= self.width <= MAX_DIM and 1 <= self.height <= MAX_DIM):
            raise ValueError("mjpeg: a frame is 1 .. 65535 pixels wide and high, got %d x %d" % (self.width, self.height))
        rate = Fraction(fps).limit_denominator(100000)
        if rate <= 0:
            raise ValueError("mjpeg: fps must be positive, got %r" % (fps,))
        self.rate, self.scale = rate.numerator, rate.denominator
        self.path = path
        self._encoder = encoder
        self._index = []                  # (offset from the 'movi' tag, length) of every chunk
        self._max_chunk = 0
        self._size = _MOVI_LIST_AT + 12   # bytes written so far: headers, LIST movi's header and tag
        self._f = open(path, "wb")
        self._f.write(self._headers())
        self.closed = False

    frames = property(lambda self: len(self._index))

    def _headers(self):
        n = len(self._index)
        movi_bytes = self._size - _MOVI_LIST_AT - 8
        riff_bytes = self._size + 8 + 16 * n - 8
        usec = (1000000 * self.scale + self.rate // 2) // self.rate
        per_sec = min(0xFFFFFFFF, -(-self._max_chunk * self.rate // self.scale))
        avih = struct.pack("<14I", usec, per_sec, 0, _AVIF_HASINDEX, n, 0, 1, self._max_chunk, self.width, self.height,
                           0, 0, 0, 0)
        strh = b"vidsMJPG" + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, self.scale, self.rate, 0, n, self._max_chunk,
                                         0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3,
                           0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        assert len(hdrl) == _HDRL_BYTES
        return (b"RIFF" + struct.pack("<I", riff_bytes) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", movi_bytes) + b"movi")

    def add(self, frames):
        """Appends the frames of one call, in order.  ValueError for frames of another size or channel count, and before
        the file would pass 2 GiB - 1 (nothing of that call is written then)."""
        if self.closed:
            raise ValueError("mjpeg: %s is closed" % (self.path,))
        shape = tuple(int(v) for v in frames.shape)
        if len(shape) == 3:
            shape = shape + (1,)
        if len(shape) != 4 or shape[1:] != (self.height, self.width, self.channels):
            raise ValueError("mjpeg: frames of %s do not fit a movie of %d x %d with %d channel(s)"
                             % ("x".join(str(v) for v in frames.shape), self.width, self.height, self.channels))
        if shape[0] == 0:
            return
        files = self._encoder(frames) if self._encoder is not None else encode_jpeg_device(frames, self.quality)
        if len(files) != shape[0]:
            raise ValueError("mjpeg: %d frames were encoded into %d files" % (shape[0], len(files)))
        grown = sum(8 + len(f) + (len(f) & 1) for f in files)
        final = self._size + grown + 8 + 16 * (len(self._index) + len(files))
        if final > RIFF_LIMIT:
            raise ValueError("mjpeg: %s would pass the 2 GiB - 1 limit of a RIFF AVI with these %d frames (%d bytes); "
                             "close it and start another file (OpenDML is not written)" % (self.path, len(files), final))
        for data in files:
            self._index.append((self._size - _MOVI_LIST_AT - 8, len(data)))
            self._f.write(b"00dc" + struct.pack("<I", len(data)))
            self._f.write(data)
            if len(data) & 1:
                self._f.write(b"\x00")
            self._size += 8 + len(data) + (len(data) & 1)
            self._max_chunk = max(self._max_chunk, len(data))

    def close(self):
        if self.closed:
            return
        self.closed = True
        try:
            self._f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            for at, length in self._index:
                self._f.write(b"00dc" + struct.pack("<III", _AVIIF_KEYFRAME, at, length))
            self._f.seek(0)
            self._f.write(self._headers())
        finally:
            self._f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
