"""Cases the tests of the self-synchronising JPEG entropy decoder share (tests/test_jpeg_sync_cpu.py,
tests/test_jpeg_sync_gpu.py): damaged Pillow-written files without restart markers."""
from spnet_amd import jpeg as J
from tests.helpers import jpeg_decode_corpus as C


def scan_bounds(data):
    info = J.parse_jpeg(data)
    assert info.device and info.bounds.shape[0] == 1, info.host_reason             # one interval: no restart markers
    return int(info.bounds[0][0]), int(info.bounds[0][1])


def pillow_damaged(shape=(40, 64)):
    """name -> file, and the sound file: a Pillow file without restart markers with a byte flipped mid-scan, with its scan
    cut short, and with garbage (no FF) between the scan and EOI.  Each still parses as a file the device takes."""
    sound = C.pillow_jpeg(C.content("noise", shape, 5), quality=90)
    lo, hi = scan_bounds(sound)
    flipped = bytearray(sound)
    at = next(p for p in range((lo + hi) // 2, hi) if sound[p] not in (0xFF, 0xFF ^ 0x5A) and sound[p - 1] != 0xFF)
    flipped[at] ^= 0x5A
    cut = sound[:lo + (hi - lo) // 2] + b"\xff\xd9"
    garbage = sound[:hi] + bytes([0x12, 0x34, 0x56, 0x78] * 3) + sound[hi:]
    bad = dict(flipped=bytes(flipped), cut=cut, garbage=garbage)
    for name, data in bad.items():
        assert J.parse_jpeg(data).device and J.parse_jpeg(data).bounds.shape[0] == 1, name
    return bad, sound
