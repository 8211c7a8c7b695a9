"""The host side of the JPEG decoder (spnet_amd/jpeg.py: parse_jpeg, plan_decode, MjpegReader, read_frames_device's
routing), the numpy restatement of the decoder (tests/helpers/jpeg_decode_ref.py) against Pillow, and the decode core
(spnet_amd/csrc/jpeg_decode_core.h) as the stand-alone program tools/jpeg_decode_host_check.cpp, built with AddressSanitizer
and UndefinedBehaviorSanitizer and run over the whole corpus and the damaged files: the bounds rules are proven here, on
plain arrays of exact size, before the same code meets a malformed stream on a GPU."""
import io
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
from PIL import Image

from spnet_amd import jpeg as J
from tests.helpers import jpeg_decode_corpus as C
from tests.helpers import jpeg_decode_ref as R
from tests.helpers import jpeg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def expected():
    return C.expected(C.corpus())


# ----------------------------------------------------------------------------- the restatement against Pillow
def test_the_corpus_is_what_it_says():
    names = [c.name for c in C.corpus()]
    assert len(set(names)) == len(names) == 4 * 3 * 4 + 2 * 3 * 4 * 4 + 2 * 3 * 4 * 12
    # the ramp makes this project's encoder emit ZRL, the flat frame nothing but DC codes and EOB
    ramp = jpeg_ref.encode_scan(C.content("ramp", (19, 37)), 10)[2]
    flat = jpeg_ref.encode_scan(C.content("flat", (19, 37)), 90)[2]
    assert ramp["zrl"] > 0
    assert flat["eob"] == 3 * 5 and flat["ac_category"] == 0
    by_name = {c.name: c for c in C.corpus()}
    assert J.parse_jpeg(by_name["24x40x3-noise-q90-pillow-plain-s2"].data).hs == 2
    assert (J.parse_jpeg(by_name["24x40x3-noise-q90-pillow-plain-s1"].data).hs,
            J.parse_jpeg(by_name["24x40x3-noise-q90-pillow-plain-s1"].data).vs) == (2, 1)
    assert J.parse_jpeg(by_name["19x37-noise-q90-pillow-plain-sNone"].data).restart == 0
    assert J.parse_jpeg(by_name["19x37-noise-q90-pillow-rst_blocks-sNone"].data).restart == 2
    plain = J.parse_jpeg(by_name["19x37-noise-q90-pillow-plain-sNone"].data).huffman
    assert J.parse_jpeg(by_name["19x37-noise-q90-pillow-optimize-sNone"].data).huffman != plain      # custom tables


def test_restatement_equals_pillow_exactly(expected):
    wrong = []
    for c in C.corpus():
        status, got = R.decode(c.data, J.HUFFMAN_TABLES)
        want = expected[c.name]
        if status != 0 or not np.array_equal(got.reshape(want.shape), want):
            wrong.append((c.name, status, None if got is None else int((got.reshape(want.shape) != want).sum())))
    assert not wrong, wrong[:10]


def test_a_frame_without_dht_uses_the_annex_k_tables():
    """Common in Motion-JPEG.  Pillow (libjpeg-turbo) decodes such a frame with the tables of T.81 Annex K; so does this."""
    frame = C.content("noise", (24, 40))
    whole = C.pillow_jpeg(frame, quality=90)
    bare = C.without_dht(whole)
    assert b"\xff\xc4" not in bare[:bare.index(b"\xff\xda")]
    want = np.asarray(Image.open(io.BytesIO(bare)))
    assert np.array_equal(want, np.asarray(Image.open(io.BytesIO(whole))))
    info = J.parse_jpeg(bare)
    assert info.device and info.huffman == {(cls, dest): tab for cls, dest, tab in J.HUFFMAN_TABLES}
    status, got = R.decode(bare, J.HUFFMAN_TABLES)
    assert status == 0 and np.array_equal(got, want)


# ----------------------------------------------------------------------------- parse_jpeg
def test_parse_agrees_with_the_restatements_marker_walk():
    for c in C.corpus():
        info = J.parse_jpeg(c.data)
        w = R.walk(c.data, J.HUFFMAN_TABLES)
        assert info.device, (c.name, info.host_reason)
        assert (info.height, info.width, info.components) == (w["height"], w["width"], len(w["comps"])), c.name
        assert [tuple(b) for b in info.bounds.tolist()] == w["intervals"], c.name
        assert info.restart == w["restart"]
        for k, comp in enumerate(w["comps"]):
            assert np.array_equal(info.quant[info.comp_quant[k]], w["quant"][comp[2]])
            assert (info.comp_dc[k], info.comp_ac[k]) == comp[3:5]


def test_files_the_device_leaves_to_the_host():
    frame = C.content("noise", (24, 40, 3))
    for data, word in ((C.progressive(frame), "SOF2"), (C.cmyk(), "4 components"), (C.adobe_rgb(frame), "not YCbCr"),
                       (b"\x89PNG\r\n\x1a\n", "signature"), (b"", "signature")):
        info = J.parse_jpeg(data)
        assert not info.device and word in info.host_reason, (word, info.host_reason)
    assert Image.open(io.BytesIO(C.adobe_rgb(frame))).mode == "RGB"
    # 16-bit quantisation entries: the 8-bit table rewritten with precision 1
    data = C.pillow_jpeg(C.content("noise", (8, 8)), quality=90)
    at = data.index(b"\xff\xdb")
    table = data[at + 5:at + 69]
    wide = b"\xff\xdb" + struct.pack(">H", 2 + 1 + 128) + b"\x10" + b"".join(b"\x00" + bytes([v]) for v in table)
    assert "16-bit" in J.parse_jpeg(data[:at] + wide + data[at + 69:]).host_reason
    # restart markers out of sequence
    ours = bytearray(jpeg_ref.encode_jpeg(C.content("noise", (40, 16)), 90))
    at = ours.index(b"\xff\xd1")
    ours[at + 1] = 0xD3
    assert "out of sequence" in J.parse_jpeg(bytes(ours)).host_reason


def test_truncated_files_come_back_clean():
    """Cut at every segment boundary (and around each), and at a few places inside the scan: device=False with a reason,
    never an exception."""
    for c in (C.corpus()[0], C.corpus()[-1]):
        cuts = C.segment_boundaries(c.data)
        cuts += [cuts[-1] + 1, cuts[-1] + 7, len(c.data) - 2, len(c.data) - 1]
        for cut in cuts:
            info = J.parse_jpeg(c.data[:cut])
            assert not info.device and isinstance(info.host_reason, str), (c.name, cut)
        assert J.parse_jpeg(c.data).device


def test_plan_groups_intervals_by_table_set():
    by_name = {c.name: c for c in C.corpus()}
    names = ["19x37-noise-q90-ours", "19x37-noise-q90-pillow-optimize-sNone", "19x37-ramp-q10-ours"]
    plan = J.plan_decode([J.parse_jpeg(by_name[n].data) for n in names])
    assert plan["tables"].shape == (2, J.TABLE_WORDS) and plan["intervals"].shape[0] == 128
    sets = plan["files"][plan["intervals"][:, 2], 5]
    assert set(sets[:64]) == {0} and set(sets[64:]) == {1}
    real = plan["intervals"][plan["intervals"][:, 4] > 0]
    assert real.shape[0] == 3 + 1 + 3 and plan["blocks"] == 3 * 15              # 19 x 37: 3 x 5 blocks, a row per interval
    assert int(real[:, 1].max()) == plan["blob"].size


# ----------------------------------------------------------------------------- the decode core under sanitizers
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/jpeg_decode_host_check.cpp with -fsanitize=address,undefined, as a program of its own (no preloading)."""
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("hostcheck") / "jpeg_decode_host_check")
    cmd = [clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "spnet_amd", "csrc"), os.path.join(ROOT, "tools", "jpeg_decode_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_host_check(exe, datas, directory):
    """[(status, pixels [H][W][C] or None)] of files of one size, decoded in ONE plan."""
    infos = [J.parse_jpeg(d) for d in datas]
    assert all(i.device for i in infos), [i.host_reason for i in infos]
    plan = J.plan_decode(infos)
    H, W = infos[0].height, infos[0].width
    plan_path, out_path = os.path.join(directory, "plan.bin"), os.path.join(directory, "out.bin")
    with open(plan_path, "wb") as f:
        f.write(np.array([plan["blob"].size, plan["intervals"].shape[0], len(infos), plan["tables"].shape[0],
                          plan["quant"].shape[0], plan["blocks"], H, W], np.int64).tobytes())
        for key in ("intervals", "files", "tables", "quant", "blob"):
            f.write(plan[key].tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, plan_path, out_path], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    raw = open(out_path, "rb").read()
    pos, out = 0, []
    for info in infos:
        status, = struct.unpack("<i", raw[pos:pos + 4])
        pos += 4
        pixels = None
        if status == 0:
            n = H * W * info.components
            pixels = np.frombuffer(raw[pos:pos + n], np.uint8).reshape(H, W, info.components)
            pos += n
        out.append((status, pixels))
    assert pos == len(raw)
    return out


def test_core_equals_pillow_on_the_corpus(host_check, expected, tmp_path):
    for shape in C.SHAPES:
        cases = [c for c in C.corpus() if c.shape == shape]           # every source, option and table set in one plan
        for c, (status, got) in zip(cases, run_host_check(host_check, [c.data for c in cases], str(tmp_path))):
            assert status == 0 and np.array_equal(got, expected[c.name]), (c.name, status)


def test_core_rejects_damaged_files_and_nothing_else(host_check, tmp_path):
    bad, sound = C.damaged()
    names = sorted(bad)
    datas = [sound] + [bad[n] for n in names] + [sound]
    out = run_host_check(host_check, datas, str(tmp_path))
    want = C.pillow_pixels(sound)
    assert out[0][0] == 0 and out[-1][0] == 0 and np.array_equal(out[0][1], want) and np.array_equal(out[-1][1], want)
    for n, (status, _) in zip(names, out[1:-1]):
        ref_status, _ = R.decode(bad[n], J.HUFFMAN_TABLES)
        assert status != 0 and ref_status != 0, (n, status, ref_status)
    assert out[1 + names.index("cut")][0] == R.INPUT_EXHAUSTED


def test_core_survives_a_flip_of_every_byte_of_a_scan(host_check, tmp_path):
    """Every byte of a small scan flipped in turn, all in one plan: whatever the status, nothing is read or written out of
    bounds (the sanitizers watch), and a file that is accepted holds what Pillow decodes from the same bytes."""
    sound = jpeg_ref.encode_jpeg(C.content("noise", (16, 16), 9), 50)
    info = J.parse_jpeg(sound)
    lo, hi = int(info.bounds[0][0]), int(info.bounds[-1][1])
    datas = []
    for p in range(lo, hi):
        d = bytearray(sound)
        d[p] ^= 0xFF
        if J.parse_jpeg(bytes(d)).device:
            datas.append(bytes(d))
    assert len(datas) > (hi - lo) // 2
    out = run_host_check(host_check, datas, str(tmp_path))
    assert sum(1 for s, _ in out if s != 0) > len(out) // 2
    for d, (status, got) in zip(datas, out):
        if status == 0:
            assert np.array_equal(got, C.pillow_pixels(d))


# ----------------------------------------------------------------------------- Motion-JPEG
def _movie(path, files, width, height):
    it = iter(files)
    with J.MjpegWriter(path, width, height, fps=12.5, channels=1, encoder=lambda frames: [next(it) for _ in frames]) as w:
        for k in range(len(files)):
            w.add(np.zeros((1, height, width), np.uint8))
    return path


def test_reader_returns_what_went_into_the_writer(tmp_path):
    files = [jpeg_ref.encode_jpeg(C.content("noise", (16, 24), s), 90) for s in range(4)]
    files[1] += b"\x00" if len(files[1]) % 2 == 0 else b""          # one odd-sized chunk at least
    files[2] = files[2] + (b"" if len(files[2]) % 2 else b"\x00")
    assert any(len(f) % 2 for f in files)
    path = _movie(str(tmp_path / "m.avi"), files, 24, 16)
    r = J.MjpegReader(path)
    assert len(r) == 4 and r.size == (24, 16) and r.fps == 12.5
    assert [r.frame_bytes(k) for k in range(4)] == files and r.frame_bytes(-1) == files[3]
    # the same file with idx1 cut off
    data = open(path, "rb").read()
    cut = str(tmp_path / "noidx.avi")
    with open(cut, "wb") as f:
        f.write(data[:data.rindex(b"idx1")])
    r2 = J.MjpegReader(cut)
    assert [r2.frame_bytes(k) for k in range(len(r2))] == files


def test_reader_on_a_hand_built_avi_and_a_foreign_codec(tmp_path):
    frames = [b"\xff\xd8odd", b"\xff\xd8even"]                       # 5 bytes (padded) and 6

    def chunk(tag, body):
        return tag + struct.pack("<I", len(body)) + body + (b"\x00" if len(body) & 1 else b"")

    def avi(handler, compression):
        avih = struct.pack("<14I", 40000, 0, 0, 0, 2, 0, 1, 0, 32, 16, 0, 0, 0, 0)
        strh = b"vids" + handler + struct.pack("<IHHIIIIIIII4H", 0, 0, 0, 0, 1, 25, 0, 2, 0, 0, 0, 0, 0, 32, 16)
        strf = struct.pack("<IiiHH4sIiiII", 40, 32, 16, 1, 24, compression, 0, 0, 0, 0, 0)
        strl = chunk(b"LIST", b"strl" + chunk(b"strh", strh) + chunk(b"strf", strf))
        hdrl = chunk(b"LIST", b"hdrl" + chunk(b"avih", avih) + strl)
        movi = chunk(b"LIST", b"movi" + chunk(b"00dc", frames[0]) + chunk(b"01wb", b"snd") + chunk(b"00db", frames[1]))
        body = b"AVI " + hdrl + chunk(b"JUNK", b"\x00" * 7) + movi
        return b"RIFF" + struct.pack("<I", len(body)) + body

    path = str(tmp_path / "hand.avi")
    with open(path, "wb") as f:
        f.write(avi(b"mjpg", b"MJPG"))
    r = J.MjpegReader(path)
    assert len(r) == 2 and r.size == (32, 16) and r.fps == 25.0
    assert [r.frame_bytes(0), r.frame_bytes(1)] == frames
    with open(path, "wb") as f:
        f.write(avi(b"H264", b"H264"))
    with pytest.raises(ValueError, match="not MJPG"):
        J.MjpegReader(path)
    with open(path, "wb") as f:
        f.write(b"RIFF\x04\x00\x00\x00WAVE")
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        J.MjpegReader(path)


# ----------------------------------------------------------------------------- routing
def test_read_frames_device_routes_by_signature(tmp_path, monkeypatch):
    import torch
    from spnet_amd import png as P
    paths = []
    for k, head in enumerate((b"\x89PNG", b"\xff\xd8\xff", b"BM", b"\xff\xd8\xff")):
        p = str(tmp_path / ("f%d" % k))
        with open(p, "wb") as f:
            f.write(head)
        paths.append(p)
    calls = []

    def stub(kind, value):
        def read(ps, threads=16, device=None, channels="first", return_info=False):
            ps = list(ps)
            calls.append((kind, ps, channels))
            out = torch.full((len(ps), 2, 3), value, dtype=torch.uint8)
            for j, p in enumerate(ps):
                out[j, 0, 0] = int(p[-1])
            status = np.zeros(len(ps), np.int32)
            status[-1] = 4
            return (out, status, [len(ps) - 1]) if return_info else out
        return read

    monkeypatch.setattr(J, "read_jpeg_device", stub("jpeg", 200))
    monkeypatch.setattr(P, "read_png_device", stub("png", 100))
    out, status, fallback = J.read_frames_device(paths, return_info=True)
    assert sorted(calls) == [("jpeg", [paths[1], paths[3]], "first"), ("png", [paths[0], paths[2]], "first")]
    assert out[:, 0, 0].tolist() == [0, 1, 2, 3] and out[:, 1, 1].tolist() == [100, 200, 100, 200]
    assert status.tolist() == [0, 0, 4, 104] and fallback == [2, 3]
    # without a JPEG file: ONE call of read_png_device with the same arguments, its result as it is
    calls.clear()
    got = J.read_frames_device([paths[0], paths[2]], channels="all")
    assert calls == [("png", [paths[0], paths[2]], "all")] and got.shape == (2, 2, 3)
    calls.clear()
    got = J.read_frames_device([paths[1]], channels="all")
    assert calls == [("jpeg", [paths[1]], "all")]


def test_argument_checks_come_before_the_gpu():
    with pytest.raises(ValueError):
        J.decode_jpeg_device([C.corpus()[0].data], channels="some")
