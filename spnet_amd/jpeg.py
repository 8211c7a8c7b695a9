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

Reading (csrc/jpeg_decode.hip, csrc/jpeg_decode_core.h; additive and opt-in: --device_decode, --movie_in): parse_jpeg walks
the markers and finds the restart intervals, plan_decode builds what the kernels read, decode_jpeg_device /
read_jpeg_device have the contract of their PNG namesakes (codec_host.decode_batch: one size per call, host fallback through
codec_host.host_frame, one pinned upload, one status download), read_frames_device routes a list of PNG and JPEG files by
signature, MjpegReader walks a RIFF AVI.  Baseline JPEG, grey or YCbCr 4:4:4 / 4:2:2 / 4:2:0; the pixels are Pillow's, sample for sample (DESIGN.md
section 5f).  Two entropy kernels share one workspace: a lane per restart interval (spnet_jpeg_entropy) and, for the long
intervals of files without restart markers, a workgroup per interval that decodes segments speculatively and chains them
until the result is the serial one (spnet_jpeg_entropy_sync, csrc/jpeg_sync_core.h); entropy= picks, see ENTROPY_MODES.
"""
import struct
from fractions import Fraction

import numpy as np

from .codec_host import MAX_THREADS, decode_batch, map_pool, read_file, stage, write_files

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

    def encode():
        scans = scans_device(frames, quality)
        header = jpeg_header(W, H, channels, quality)
        return lambda k: (header, scans[k], JPEG_TRAILER)

    return write_files(paths, N, encode, threads, pool, "jpeg")


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


# ----------------------------------------------------------------------------- reading: container
# What the device decoder (csrc/jpeg_decode.hip) takes: baseline sequential DCT (SOF0), 8 bit, ONE scan over all components,
# one component (grey) or three that Pillow reads as YCbCr (JFIF, or no Adobe segment saying otherwise), luma sampled 1x1,
# 2x1 or 2x2 and chroma 1x1, quantisation tables of 8-bit entries, at most two Huffman tables per class.  Everything else
# (progressive, extended, arithmetic, 12 bit, CMYK / Adobe transforms, several scans, fill bytes, restart markers out of
# sequence) is left to Pillow.  A frame without a DHT segment (common in Motion-JPEG) uses the Annex K tables, as
# libjpeg-turbo does.
STATUS_NAMES = ("ok", "bit pattern that is no code", "coefficient index past 63", "magnitude category too large",
                "bits missing before the interval's MCUs are done", "bytes left over after the interval's MCUs",
                "table entry outside the launch's arrays")
TABLE_WORDS = 4 * 226           # one Huffman table set in device form: DC 0, AC 0, DC 1, AC 1 (jpeg_decode_core.h)
MAX_BLOB = (1 << 31) - 1024     # spnet_jpeg_entropy: 32-bit byte positions
MAX_PIXELS = 1 << 28            # H * W of one frame
# entropy=: "interval": every restart interval is one lane of spnet_jpeg_entropy; "sync": every interval is a workgroup of
# spnet_jpeg_entropy_sync; "auto": intervals of at least SYNC_MIN_BYTES bytes go to the sync kernel, the rest to the lane
# kernel, in one call on one workspace.  The coefficients are the same whichever kernel wrote them.
ENTROPY_MODES = ("auto", "interval", "sync")
DEFAULT_ENTROPY = "auto"
SYNC_MIN_BYTES = 8192           # the measured crossover (tools/jpeg_decode_time.py)
SYNC_SEG_BYTES = 128            # bytes of a lane's segment: a multiple of 4 in 4 .. 4096 (measured, as above)
_SOF_OTHER = frozenset(range(0xC1, 0xD0)) - {0xC4, 0xC8, 0xCC}
_EMPTY_TABLE = ((0,) * 16, ())


class JpegInfo:
    """What parse_jpeg found.  width, height, components (1 | 3), hs, vs (luma sampling factors), quant {id: uint16 [64] in
    natural order}, comp_quant / comp_dc / comp_ac (per component: table ids), huffman {(class, id): (BITS, HUFFVAL)},
    restart (MCUs per interval, 0: none), bounds (int64 [n + 1][2]: the byte range of every restart interval's entropy-coded
    data in `data`), data (the file), host_reason: None for a file the device decodes, else why the host has to (str)."""
    __slots__ = ("width", "height", "components", "hs", "vs", "quant", "comp_quant", "comp_dc", "comp_ac", "huffman",
                 "restart", "bounds", "data", "host_reason")

    def __init__(self):
        self.width = self.height = self.components = self.hs = self.vs = None
        self.quant, self.huffman = {}, {}
        self.comp_quant = self.comp_dc = self.comp_ac = ()
        self.restart = 0
        self.bounds = None
        self.data = b""
        self.host_reason = None

    @property
    def device(self):
        return self.host_reason is None

    @property
    def mcu_grid(self):
        """(MCU columns, MCU rows)."""
        return (self.width + 8 * self.hs - 1) // (8 * self.hs), (self.height + 8 * self.vs - 1) // (8 * self.vs)

    @property
    def blocks(self):
        """8 x 8 blocks of all components: the file's share of the coefficient workspace."""
        mw, mh = self.mcu_grid
        return mw * mh * (self.hs * self.vs + (2 if self.components == 3 else 0))


def parse_jpeg(data):
    """The marker walk: SOI, APPn / COM (skipped, but for what JFIF and Adobe say about colour), DQT, SOF0, DHT, DRI, SOS,
    the restart markers (one vectorised scan), EOI.  Raises nothing: a file the device cannot take, a damaged container
    included, comes back with host_reason set and is left to the host decoder, which decides what it is."""
    info = JpegInfo()
    info.data = data
    buf = np.frombuffer(data, np.uint8)
    n = int(buf.size)

    def no(reason):
        info.host_reason = reason
        return info

    if n < 4 or buf[0] != 0xFF or buf[1] != 0xD8:
        return no("no JPEG signature")
    pos = 2
    jfif = False
    adobe = None
    frame = None                 # [(id, h, v, tq)]
    have_dht = False
    while True:
        if pos + 4 > n:
            return no("the file ends in its headers")
        if buf[pos] != 0xFF:
            return no("no marker where one is due")
        m = int(buf[pos + 1])
        if m == 0xFF:            # fill byte
            pos += 1
            continue
        if m == 0xD8 or m == 0xD9 or 0xD0 <= m <= 0xD7 or m == 0x01:
            return no("marker FF %02X in the headers" % m)
        length = int(buf[pos + 2]) << 8 | int(buf[pos + 3])
        if length < 2 or pos + 2 + length > n:
            return no("segment FF %02X runs past the end of the file" % m)
        body = buf[pos + 4:pos + 2 + length]
        pos += 2 + length
        if m == 0xE0:
            jfif = jfif or (body.size >= 5 and bytes(body[:5]) == b"JFIF\x00")
        elif m == 0xEE:
            if body.size >= 12 and bytes(body[:5]) == b"Adobe":
                adobe = int(body[11])
        elif m == 0xDB:
            k = 0
            while k < body.size:
                pq, tq = int(body[k]) >> 4, int(body[k]) & 15
                if pq != 0:
                    return no("quantisation table of 16-bit entries")
                if tq > 3 or k + 65 > body.size:
                    return no("damaged DQT")
                table = np.zeros(64, np.uint16)
                table[np.array(ZIGZAG)] = body[k + 1:k + 65]
                info.quant[tq] = table
                k += 65
        elif m == 0xC0:
            if frame is not None:
                return no("a second frame header")
            if body.size < 6:
                return no("damaged SOF0")
            precision, info.height, info.width, nc = (int(body[0]), int(body[1]) << 8 | int(body[2]),
                                                       int(body[3]) << 8 | int(body[4]), int(body[5]))
            if precision != 8:
                return no("%d-bit samples" % precision)
            if body.size != 6 + 3 * nc:
                return no("damaged SOF0")
            if nc not in (1, 3):
                return no("%d components" % nc)
            if info.width < 1 or info.height < 1:
                return no("empty image (or a DNL-defined height)")
            frame = [(int(body[6 + 3 * c]), int(body[7 + 3 * c]) >> 4, int(body[7 + 3 * c]) & 15, int(body[8 + 3 * c]))
                     for c in range(nc)]
            info.components = nc
        elif m in _SOF_OTHER:
            return no("not baseline (SOF%d)" % (m - 0xC0))
        elif m == 0xC4:
            have_dht = True
            k = 0
            while k < body.size:
                if k + 17 > body.size:
                    return no("damaged DHT")
                tc, th = int(body[k]) >> 4, int(body[k]) & 15
                bits = tuple(int(v) for v in body[k + 1:k + 17])
                count = sum(bits)
                if tc > 1 or th > 1 or count > 256 or k + 17 + count > body.size:
                    return no("damaged DHT, or a table id above 1")
                if _oversubscribed(bits):
                    return no("over-subscribed Huffman code")
                info.huffman[(tc, th)] = (bits, tuple(int(v) for v in body[k + 17:k + 17 + count]))
                k += 17 + count
        elif m == 0xDD:
            if body.size != 2:
                return no("damaged DRI")
            info.restart = int(body[0]) << 8 | int(body[1])
        elif m == 0xCC:
            return no("arithmetic coding")
        elif m == 0xDA:
            break
        # every other segment (APPn, COM, ...) is skipped
    if frame is None:
        return no("SOS before SOF0")
    nc = info.components
    if body.size != 4 + 2 * nc or int(body[0]) != nc:
        return no("a scan that does not hold every component (several scans)")
    if (int(body[1 + 2 * nc]), int(body[2 + 2 * nc]), int(body[3 + 2 * nc])) != (0, 63, 0):
        return no("spectral selection / successive approximation")
    dc, ac = [], []
    for c in range(nc):
        if int(body[1 + 2 * c]) != frame[c][0]:
            return no("scan components out of frame order")
        td, ta = int(body[2 + 2 * c]) >> 4, int(body[2 + 2 * c]) & 15
        if td > 1 or ta > 1:
            return no("Huffman table id above 1")
        dc.append(td)
        ac.append(ta)
    info.comp_dc, info.comp_ac = tuple(dc), tuple(ac)
    info.comp_quant = tuple(f[3] for f in frame)
    if any(t not in info.quant for t in info.comp_quant):
        return no("a quantisation table that was never defined")
    if not have_dht:
        info.huffman = {(cls, dest): tab for cls, dest, tab in HUFFMAN_TABLES}
    if any((0, t) not in info.huffman for t in dc) or any((1, t) not in info.huffman for t in ac):
        return no("a Huffman table that was never defined")
    if nc == 1:
        info.hs = info.vs = 1            # a single component is not interleaved: its sampling factors do not matter
    else:
        ids = tuple(f[0] for f in frame)
        # as libjpeg decides: JFIF says YCbCr; else Adobe's transform flag; else the ids (R G B means RGB)
        if jfif:
            ycc = True
        elif adobe is not None:
            ycc = adobe == 1
        else:
            ycc = ids != (82, 71, 66)
        if adobe is not None and adobe != 1:
            ycc = False
        if not ycc:
            return no("three components that are not YCbCr")
        info.hs, info.vs = frame[0][1], frame[0][2]
        if (info.hs, info.vs) not in ((1, 1), (2, 1), (2, 2)) or any(f[1:3] != (1, 1) for f in frame[1:]):
            return no("sampling factors %s" % ",".join("%dx%d" % f[1:3] for f in frame))
    if info.width * info.height > MAX_PIXELS:
        return no("larger than the device decoder's budget")
    # ---- the scan: every FF that is not followed by 00 is a marker
    scan = buf[pos:]
    at = np.flatnonzero((scan[:-1] == 0xFF) & (scan[1:] != 0)) + pos if scan.size > 1 else np.zeros(0, np.int64)
    kinds = buf[at + 1] if at.size else np.zeros(0, np.uint8)
    other = np.flatnonzero((kinds < 0xD0) | (kinds > 0xD7))
    if other.size == 0:
        return no("no EOI")
    last = int(other[0])
    if int(kinds[last]) != 0xD9:
        return no("marker FF %02X in the scan (fill bytes, several scans, DNL)" % int(kinds[last]))
    rst_at, rst_kind = at[:last], kinds[:last]
    mw, mh = info.mcu_grid
    mcus = mw * mh
    want = (mcus + info.restart - 1) // info.restart - 1 if info.restart else 0
    if rst_at.size != want or not np.array_equal(rst_kind, 0xD0 + (np.arange(want) & 7)):
        return no("restart markers out of sequence")
    if want and np.any(np.diff(rst_at) < 2):
        return no("restart markers out of sequence")
    bounds = np.empty((want + 1, 2), np.int64)
    bounds[:, 0] = np.concatenate(([pos], rst_at + 2))
    bounds[:, 1] = np.concatenate((rst_at, [int(at[last])]))
    info.bounds = bounds
    return info


def _oversubscribed(bits):
    """More codes of some length than that length has left (T.81 Annex C builds codes by counting up)."""
    code = 0
    for length in range(16):
        code += bits[length]
        if code > 1 << (length + 1):
            return True
        code <<= 1
    return False


def device_table(table):
    """One Huffman table (BITS, HUFFVAL) in the device's form, 226 uint32 words (jpeg_decode_core.h): look[256] as uint16
    (length << 8 | symbol for every code of up to 8 bits, indexed by the next 8 bits; 0: longer, or no code), maxcode[17]
    (int32, the largest code of each length 1 .. 16, -1: none; [0] unused), valoff[17] (int32: index of the length's first
    symbol minus its first code), vals[256] (uint8)."""
    bits, vals = table
    look = np.zeros(256, np.uint16)
    maxcode = np.full(17, -1, np.int32)
    valoff = np.zeros(17, np.int32)
    symbols = np.zeros(256, np.uint8)
    symbols[:len(vals)] = vals
    code, k = 0, 0
    for length in range(1, 17):
        count = bits[length - 1]
        if count:
            valoff[length] = k - code
            if length <= 8:
                for j in range(count):
                    lo = (code + j) << (8 - length)
                    look[lo:lo + (1 << (8 - length))] = length << 8 | int(symbols[k + j])
            code += count
            k += count
            maxcode[length] = code - 1
        code <<= 1
    return np.concatenate([look.view(np.uint32), maxcode.view(np.uint32), valoff.view(np.uint32), symbols.view(np.uint32)])


def plan_decode(infos, sync_min_bytes=None):
    """The arrays one launch pair reads, for files that are all info.device (host numpy arrays):
      blob       uint8: the files' entropy-coded bytes, interval after interval (markers left out)
      intervals  int32 [n][8]: first byte, end byte (positions in blob), file, first MCU, MCUs, 0, 0, 0 -- grouped by table
                 set, every group padded with empty intervals to a multiple of 64 (a workgroup holds ONE set in LDS)
      files      int32 [N][16]: components, hs, vs, MCU columns, MCU rows, table set, first block (in the workspace), 0,
                 (DC table | AC table << 4) x 3, quantisation table x 3, 0, 0
      tables     uint32 [sets][TABLE_WORDS], deduplicated
      quant      uint16 [q][64], natural order, deduplicated
      blocks     8 x 8 blocks of the workspace
    sync_min_bytes (None: as above, nothing else): the intervals are split -- one of at least that many bytes goes to
      sync_intervals  int32 [m][8], the same record, in file order, neither grouped nor padded (spnet_jpeg_entropy_sync
                 loads the table set per interval)
    and only the others stay in `intervals`; every interval is in exactly one of the two."""
    sets, quants = {}, {}
    files = np.zeros((len(infos), 16), np.int32)
    per_set = {}
    sync_rows = []
    pieces = []
    at = 0
    block = 0
    for f, info in enumerate(infos):
        key = tuple(info.huffman.get(k, _EMPTY_TABLE) for k in ((0, 0), (1, 0), (0, 1), (1, 1)))
        s = sets.setdefault(key, len(sets))
        mw, mh = info.mcu_grid
        files[f, :7] = (info.components, info.hs, info.vs, mw, mh, s, block)
        block += info.blocks
        for c in range(info.components):
            q = quants.setdefault(info.quant[info.comp_quant[c]].tobytes(), len(quants))
            files[f, 8 + c] = info.comp_dc[c] | info.comp_ac[c] << 4
            files[f, 11 + c] = q
        ri = info.restart or mw * mh
        raw = np.frombuffer(info.data, np.uint8)
        rows = per_set.setdefault(s, [])
        for i, (lo, hi) in enumerate(info.bounds):
            lo, hi = int(lo), int(hi)
            pieces.append(raw[lo:hi])
            long = sync_min_bytes is not None and hi - lo >= sync_min_bytes
            (sync_rows if long else rows).append((at, at + hi - lo, f, i * ri, min(ri, mw * mh - i * ri), 0, 0, 0))
            at += hi - lo
    intervals = []
    for s in sorted(per_set):
        rows = per_set[s]
        if not rows:
            continue
        f0 = rows[0][2]
        rows += [(0, 0, f0, 0, 0, 0, 0, 0)] * (-len(rows) % 64)
        intervals += rows
    tables = np.stack([np.concatenate([device_table(t) for t in key]) for key in sets]) if sets else \
        np.zeros((0, TABLE_WORDS), np.uint32)
    quant = np.stack([np.frombuffer(q, np.uint16) for q in quants]) if quants else np.zeros((0, 64), np.uint16)
    blob = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
    plan = dict(blob=blob, intervals=np.array(intervals, np.int32).reshape(-1, 8), files=files, tables=tables,
                quant=quant, blocks=block)
    if sync_min_bytes is not None:
        plan["sync_intervals"] = np.array(sync_rows, np.int32).reshape(-1, 8)
    return plan


class DecodeInfo(list):
    """The third value of return_info: the sorted indices of the files the host decoded (a list, as it always was), and as
    attributes how many restart intervals each entropy kernel decoded in the call."""

    def __init__(self, fallback=(), lane_intervals=0, sync_intervals=0):
        super().__init__(fallback)
        self.lane_intervals, self.sync_intervals = int(lane_intervals), int(sync_intervals)


def _entropy_split(entropy, seg_bytes):
    """(sync_min_bytes for plan_decode, seg_bytes) of an entropy= / seg_bytes= pair; ValueError before anything else."""
    if entropy is None:
        entropy = DEFAULT_ENTROPY
    if entropy not in ENTROPY_MODES:
        raise ValueError('jpeg: entropy is "auto", "interval" or "sync", got %r' % (entropy,))
    seg = SYNC_SEG_BYTES if seg_bytes is None else seg_bytes
    if not isinstance(seg, (int, np.integer)) or isinstance(seg, bool) or seg < 4 or seg > 4096 or seg % 4:
        raise ValueError("jpeg: seg_bytes is a multiple of 4 in 4 .. 4096, got %r" % (seg_bytes,))
    return {"interval": None, "sync": 0, "auto": SYNC_MIN_BYTES}[entropy], int(seg)


# ----------------------------------------------------------------------------- reading: device
def _decode_parsed(infos, sources, device, channels, return_info, split):
    """split: _entropy_split's pair, which the entry points work out before they read a file."""
    sync_min, seg_bytes = split

    def launch(idx, shape, out, device):
        import torch
        from . import _lib as L
        if not idx:
            return [], (0, 0)
        H, W = shape[:2]
        plan = plan_decode([infos[k] for k in idx], sync_min)
        if plan["blob"].size > MAX_BLOB or plan["blocks"] * 64 > (1 << 31) - 1:
            raise ValueError("jpeg: %d files of %d x %d are more than one call decodes; pass fewer" % (len(idx), W, H))
        n = len(idx)
        C = shape[2] if channels == "all" else 1
        sync_iv = plan.get("sync_intervals", np.zeros((0, 8), np.int32))
        # one pinned upload, every piece padded to 16 bytes
        dev, starts, staging = stage([plan["intervals"], plan["files"], plan["tables"], plan["quant"], plan["blob"], sync_iv],
                                     device, pinned=True, align=16)
        p_iv, p_files, p_tables, p_quant, p_blob, p_sync = (dev.data_ptr() + s for s in starts)
        got = out if n == len(out) else torch.empty((n,) + shape, dtype=torch.uint8, device=device)
        coef = torch.zeros((max(plan["blocks"], 1), 64), dtype=torch.int16, device=device)
        st = torch.empty((n,), dtype=torch.int32, device=device)
        with torch.cuda.device(device):
            L.spnet_jpeg_entropy(p_blob, int(plan["blob"].size), p_iv, int(plan["intervals"].shape[0]), p_files, n, p_tables,
                                 int(plan["tables"].shape[0]), coef.data_ptr(), int(plan["blocks"]), st.data_ptr(),
                                 L.current_stream())
            if sync_iv.shape[0]:                 # behind the lane kernel, which has cleared the status
                L.spnet_jpeg_entropy_sync(p_blob, int(plan["blob"].size), p_sync, int(sync_iv.shape[0]), p_files, n, p_tables,
                                          int(plan["tables"].shape[0]), seg_bytes, coef.data_ptr(), int(plan["blocks"]),
                                          st.data_ptr(), L.current_stream())
            L.spnet_jpeg_pixels(coef.data_ptr(), int(plan["blocks"]), p_files, n, p_quant, int(plan["quant"].shape[0]), H, W,
                                C, got.data_ptr() if channels == "first" else 0, got.data_ptr() if channels == "all" else 0,
                                st.data_ptr(), L.current_stream())
        return [(idx, st, got, (staging, coef))], (int((plan["intervals"][:, 4] > 0).sum()), int(sync_iv.shape[0]))

    return decode_batch(infos, sources, device, channels, return_info, "jpeg", lambda info: info.components, launch,
                        DecodeInfo)


def decode_jpeg_device(datas, device=None, channels="first", return_info=False, threads=MAX_THREADS, entropy=None,
                       seg_bytes=None):
    """JPEG files (a list of bytes) -> a uint8 DEVICE tensor [N,H,W] holding channel 0 of every pixel (what
    utils._load_one(..., as_uint8=True) keeps: the grey level, or R), or [N,H,W,C] with channels="all".  The entropy-coded
    bytes are uploaded as they are and decoded on the GPU (Huffman, dequantisation, IDCT, upsampling, colour).  Files the
    device does not take (see parse_jpeg) and files it rejects (status != 0) are decoded by the default path's Pillow call
    and uploaded into their place, so the pixels are the default path's in every case and a corrupt file raises what it
    raises there.  All files of a call have one size (ValueError otherwise).  return_info: also the status array
    (jpeg_decode_core.h's codes, STATUS_NAMES) and the sorted indices of the files the host decoded, as a DecodeInfo,
    whose lane_intervals / sync_intervals say how many restart intervals each entropy kernel decoded.  entropy: one of
    ENTROPY_MODES (None: DEFAULT_ENTROPY); seg_bytes: the sync kernel's segment (None: SYNC_SEG_BYTES).  Neither changes
    a pixel."""
    datas = list(datas)
    split = _entropy_split(entropy, seg_bytes)
    return _decode_parsed(map_pool(parse_jpeg, datas, threads), datas, device, channels, return_info, split)


def read_jpeg_device(paths, threads=MAX_THREADS, device=None, channels="first", return_info=False, entropy=None,
                     seg_bytes=None):
    """decode_jpeg_device of files on disk, read and parsed by a thread pool of this process (at most 16 threads; nothing
    is forked)."""
    paths = list(paths)
    split = _entropy_split(entropy, seg_bytes)
    infos = map_pool(lambda p: parse_jpeg(read_file(p)), paths, threads)
    return _decode_parsed(infos, paths, device, channels, return_info, split)


def _is_jpeg(path):
    with open(path, "rb") as f:
        return f.read(2) == b"\xff\xd8"


def read_frames_device(paths, threads=MAX_THREADS, device=None, channels="first", return_info=False, entropy=None,
                       seg_bytes=None):
    """Frames of PNG and JPEG files, routed by signature: files that begin FF D8 go to read_jpeg_device, every other file
    to png.read_png_device, unchanged; the results land in one tensor in input order.  A list without JPEG files is ONE
    call of read_png_device with the same arguments.  With return_info the status of a JPEG file is offset by 100 (PNG and
    JPEG codes share one array).  entropy / seg_bytes: read_jpeg_device's, handed on only where given."""
    from . import png
    paths = list(paths)
    _entropy_split(entropy, seg_bytes)
    how = {k: v for k, v in (("entropy", entropy), ("seg_bytes", seg_bytes)) if v is not None}
    jpg = [k for k, p in enumerate(paths) if _is_jpeg(p)]
    if not jpg:
        return png.read_png_device(paths, threads=threads, device=device, channels=channels, return_info=return_info)
    if len(jpg) == len(paths):
        got = read_jpeg_device(paths, threads=threads, device=device, channels=channels, return_info=return_info, **how)
        if return_info:
            return got[0], np.where(got[1] != 0, got[1] + 100, 0).astype(np.int32), got[2]
        return got
    import torch
    other = [k for k in range(len(paths)) if k not in set(jpg)]
    a, sa, fa = read_jpeg_device([paths[k] for k in jpg], threads=threads, device=device, channels=channels,
                                 return_info=True, **how)
    b, sb, fb = png.read_png_device([paths[k] for k in other], threads=threads, device=device, channels=channels,
                                    return_info=True)
    if a.shape[1:] != b.shape[1:]:
        raise ValueError("jpeg: the JPEG files are %s, the other files %s (one call decodes files of one size)"
                         % ("x".join(str(int(v)) for v in a.shape[1:]), "x".join(str(int(v)) for v in b.shape[1:])))
    out = torch.empty((len(paths),) + tuple(a.shape[1:]), dtype=torch.uint8, device=a.device)
    out[torch.as_tensor(jpg, device=a.device)] = a
    out[torch.as_tensor(other, device=a.device)] = b
    if not return_info:
        return out
    status = np.zeros(len(paths), np.int32)
    status[jpg] = np.where(sa != 0, sa + 100, 0)
    status[other] = sb
    return out, status, DecodeInfo(sorted([jpg[k] for k in fa] + [other[k] for k in fb]),
                                   getattr(fa, "lane_intervals", 0), getattr(fa, "sync_intervals", 0))


# ----------------------------------------------------------------------------- Motion-JPEG in a RIFF AVI: reading
class MjpegReader:
    """The frames of a Motion-JPEG RIFF AVI (every file MjpegWriter writes; no OpenDML, the first video stream only): avih
    and strh give size, frame count and rate; the frames are the 00dc / 00db chunks of LIST movi in file order (found by
    walking movi, so idx1 is not needed; chunks are padded to even length; LIST rec groups are entered).  ValueError for a
    file that is not a RIFF AVI or whose video stream's handler / compression is not MJPG."""

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            data = f.read()
        self._data = data
        n = len(data)
        if n < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
            raise ValueError("mjpeg: %s is not a RIFF AVI" % (path,))
        self.width = self.height = None
        self.rate, self.scale = 0, 1
        self._usec = 0
        self._chunks = []                 # (position of the payload, length)
        handler = None
        seen_strh = False

        def walk(lo, hi, depth):
            nonlocal handler, seen_strh
            pos = lo
            while pos + 8 <= hi:
                tag = data[pos:pos + 4]
                size, = struct.unpack("<I", data[pos + 4:pos + 8])
                end = pos + 8 + size
                if end > hi:
                    if tag == b"LIST" and data[pos + 8:pos + 12] == b"movi":
                        end = hi                        # a movie cut short: take the chunks that are whole
                    else:
                        break
                if tag == b"LIST":
                    if depth < 4 and end >= pos + 12:
                        walk(pos + 12, end, depth + 1)
                elif tag == b"avih" and size >= 40:
                    v = struct.unpack("<10I", data[pos + 8:pos + 48])
                    self._usec, self.width, self.height = v[0], v[8], v[9]
                elif tag == b"strh" and size >= 36 and not seen_strh and data[pos + 8:pos + 12] == b"vids":
                    seen_strh = True
                    handler = data[pos + 12:pos + 16]
                    self.scale, self.rate = struct.unpack("<II", data[pos + 28:pos + 36])
                elif tag == b"strf" and seen_strh and size >= 20 and handler is not None and len(handler) == 4:
                    handler = handler + data[pos + 24:pos + 28]          # biCompression
                elif tag in (b"00dc", b"00db"):
                    self._chunks.append((pos + 8, size))
                pos = end + (size & 1 if end != hi else 0)

        walk(12, n, 0)
        if handler is None:
            raise ValueError("mjpeg: %s has no video stream" % (path,))
        if handler[:4].upper() != b"MJPG" and handler[4:8].upper() != b"MJPG":
            raise ValueError("mjpeg: the video stream of %s is %r, not MJPG (Motion-JPEG is the only codec read here)"
                             % (path, handler[:4].decode("latin-1")))
        self._chunks = [c for c in self._chunks if c[1] > 0]             # (an empty chunk is a dropped frame)

    def __len__(self):
        return len(self._chunks)

    @property
    def size(self):
        """(width, height) as avih states them."""
        return self.width, self.height

    @property
    def fps(self):
        if self.rate and self.scale:
            return self.rate / self.scale
        return 1e6 / self._usec if self._usec else 0.0

    def frame_bytes(self, i):
        """Frame i as the JPEG file it is."""
        at, length = self._chunks[range(len(self._chunks))[i]]
        return self._data[at:at + length]

    def read_device(self, indices=None, channels="first", device=None, return_info=False, entropy=None, seg_bytes=None):
        """decode_jpeg_device of the frames `indices` (a slice, an iterable of indices, None: all), in that order."""
        if indices is None:
            indices = slice(None)
        picks = range(len(self))[indices] if isinstance(indices, slice) else [range(len(self))[int(i)] for i in indices]
        return decode_jpeg_device([self.frame_bytes(i) for i in picks], device=device, channels=channels,
                                  return_info=return_info, entropy=entropy, seg_bytes=seg_bytes)
