"""The host side of the PNG decoder (spnet_amd/png.py: parse_png and the argument checks of the opt-in flags) and the
decode core (spnet_amd/csrc/inflate_core.h) as the stand-alone program tools/inflate_host_check.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer and run over the whole corpus of tests/helpers/png_decode_corpus.py:
the bounds rules are proven here, on plain arrays, before the same state machine meets a malformed stream on a GPU."""
import io
import os
import shutil
import subprocess
import sys
import zlib

import numpy as np
import pytest
from PIL import Image

from spnet_amd import png as P
from tests.helpers import png_decode_corpus as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_length(case):
    H, W, ch = case.shape
    return H * (1 + W * ch)


# ----------------------------------------------------------------------------- parse_png
def test_parse_png_reads_what_pillow_and_png_container_write():
    img = C.textured((17, 31, 3), 3)
    buf = io.BytesIO()
    Image.fromarray(img, "RGB").save(buf, "PNG")
    info = P.parse_png(buf.getvalue())
    assert (info.width, info.height, info.bit_depth, info.colour_type, info.interlace) == (31, 17, 8, 2, 0)
    assert info.device and info.channels == 3 and not info.trns
    raw = np.frombuffer(zlib.decompress(info.zstream), np.uint8).reshape(17, 1 + 31 * 3)
    assert raw[:, 0].max() <= 4
    z = C.deflate(C.filter_stream(img, [0] * 17))
    info = P.parse_png(P.png_container(z, 31, 17, 3))
    assert info.device and bytes(info.zstream) == z and (info.width, info.height, info.channels) == (31, 17, 3)
    for channels, ct in P.COLOUR_TYPE.items():
        info = P.parse_png(P.png_container(z, 31, 17, channels))
        assert info.colour_type == ct and info.channels == channels


def test_parse_png_joins_idat_chunks_and_skips_ancillary_ones():
    cases = {c.name: c for c in C.container_files()}
    streams = {name: bytes(P.parse_png(c.data).zstream) for name, c in cases.items()}
    assert len(set(streams.values())) == 1 and all(P.parse_png(c.data).device for c in cases.values())
    assert cases["idat_every_byte"].data.count(b"IDAT") == len(streams["idat_every_byte"])
    assert b"tEXt" in cases["ancillary_chunks"].data and b"gAMA" in cases["ancillary_chunks"].data


def test_parse_png_reports_a_damaged_container_and_raises_nothing():
    good = C.container_files()[2].data                     # tEXt, gAMA, IDAT
    assert P.parse_png(good).device
    at = good.index(b"IDAT") + 6
    flipped = good[:at] + bytes([good[at] ^ 1]) + good[at + 1:]
    assert "CRC" in P.parse_png(flipped).host_reason
    at = good.index(b"tEXt") + 6                           # the default decoder raises on this: the host decides
    damaged = good[:at] + bytes([good[at] ^ 1]) + good[at + 1:]
    assert "CRC" in P.parse_png(damaged).host_reason
    with pytest.raises(Exception):
        C.load_one_pixels(damaged)
    for bad in (b"", b"not a png", good[:20], good[:-12], good[:-5], b"\x00" + good[1:]):
        info = P.parse_png(bad)
        assert not info.device and isinstance(info.host_reason, str)


def test_classification_of_every_corpus_file():
    for c in C.good_files() + C.malformed_files() + C.bit_flip_files(8):
        info = P.parse_png(c.data)
        assert info.device, (c.name, info.host_reason)
        assert (info.height, info.width, info.channels) == c.shape, c.name
    reasons = {c.name: P.parse_png(c.data).host_reason for c in C.host_only_files()}
    assert all(r is not None for r in reasons.values()), reasons
    assert "colour type 3" in reasons["palette"] and "16" in reasons["sixteen_bit"] and "1" in reasons["one_bit"]
    assert reasons["interlaced"] == "interlaced" and reasons["grey_trns"] == "tRNS"
    huge = P.png_container(b"", 40000, 2, 1)                # a row longer than the unfilter kernel holds
    assert "budget" in P.parse_png(huge).host_reason


def test_the_corpus_filter_routine_agrees_with_pillow():
    """The numpy filter is the corpus' own code: Pillow must decode its files to the pixels they were made from."""
    for c in C.filter_files() + C.container_files():
        H, W, ch = c.shape
        assert C.pillow_pixels(c.data).shape == (H, W, ch), c.name
    img = C.textured((17, 31, 4), 9)
    for ft in range(5):
        assert np.array_equal(C.pillow_pixels(C.png_of(img, [ft] * 17)), img), ft


def test_decode_needs_a_gpu():
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            P.decode_png_device([C.pillow_files()[0].data])
        with pytest.raises(RuntimeError, match="GPU"):
            P.read_png_device([])
    with pytest.raises(ValueError, match="channels"):
        P.decode_png_device([C.pillow_files()[0].data], channels="some")


# ----------------------------------------------------------------------------- the decode core under sanitizers
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/inflate_host_check.cpp with -fsanitize=address,undefined, as a program of its own (no preloading)."""
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "inflate_host_check")
    cmd = [clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "spnet_amd", "csrc"), os.path.join(ROOT, "tools", "inflate_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_host_check(exe, cases, directory):
    """{name: (status, bytes or None)} of the program over the zlib streams of `cases`."""
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "manifest.txt"), "w") as m:
        for c in cases:
            with open(os.path.join(directory, c.name), "wb") as f:
                f.write(P.parse_png(c.data).zstream)
            m.write("%s %d\n" % (c.name, stream_length(c)))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, directory], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        name, status = line.split()
        data = None
        if int(status) == 0:
            with open(os.path.join(directory, name + ".out"), "rb") as f:
                data = f.read()
        out[name] = (int(status), data)
    assert set(out) == {c.name for c in cases}
    return out


def test_core_inflates_every_good_stream_as_zlib_does(host_check, tmp_path):
    cases = C.good_files()
    got = run_host_check(host_check, cases, str(tmp_path / "good"))
    for c in cases:
        status, data = got[c.name]
        assert status == 0, (c.name, P.STATUS_NAMES[status])
        assert data == zlib.decompress(P.parse_png(c.data).zstream), c.name


def test_core_rejects_every_malformed_stream_with_its_status(host_check, tmp_path):
    cases = C.malformed_files()
    got = run_host_check(host_check, cases, str(tmp_path / "bad"))
    for c in cases:
        status, _ = got[c.name]
        assert status in c.expect, (c.name, P.STATUS_NAMES[status])
    assert len({got[c.name][0] for c in cases}) >= 9          # distinct codes, not one catch-all


def test_core_and_zlib_agree_on_200_bit_flips(host_check, tmp_path):
    cases = C.bit_flip_files()
    assert len(cases) == 200
    got = run_host_check(host_check, cases, str(tmp_path / "flips"))
    survived = 0
    for c in cases:
        status, data = got[c.name]
        try:
            ref = zlib.decompress(P.parse_png(c.data).zstream)
        except zlib.error:
            ref = None
        if ref is not None and len(ref) == stream_length(c):
            assert status == 0 and data == ref, c.name
            survived += 1
        else:
            assert status != 0, c.name
    print("bit flips that still inflate: %d of %d" % (survived, len(cases)))


# ----------------------------------------------------------------------------- argument checks of the opt-in surface
def test_build_x_refuses_device_decode_without_uint8_grey_frames():
    from spnet_amd import utils as U
    with pytest.raises(ValueError, match="device_decode"):
        U.build_X(1, ["x.png"], grayscale=True, as_uint8=False, device_decode=True)
    with pytest.raises(ValueError):
        U.build_X(1, ["x.png"], grayscale=False, as_uint8=True, device_decode=True)


@pytest.mark.parametrize("script", ["predict_spnet.py", "evaluate_spnet.py", "train_spnet.py", "augment_preproc.py"])
def test_cli_offers_device_decode(script):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True,
                       env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--device_decode" in r.stdout
