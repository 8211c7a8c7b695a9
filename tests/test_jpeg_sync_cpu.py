"""The self-synchronising entropy decoder (spnet_amd/csrc/jpeg_sync_core.h) as the stand-alone program
tools/jpeg_sync_host_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer: the workgroup of
csrc/jpeg_decode_sync.hip with its lanes in a loop, over plain arrays of exact size, beside the serial decode_interval of
jpeg_decode_core.h, which is the oracle -- same status, same workspace.  And the host side of entropy= (spnet_amd/jpeg.py):
the split plan and the argument checks."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from spnet_amd import jpeg as J
from tests.helpers import jpeg_decode_corpus as C
from tests.helpers import jpeg_ref
from tests.helpers.jpeg_sync_cases import pillow_damaged, scan_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEGS = (4, 8, 32, 256)
LANES = 8                # of the emulated workgroup: small, so that the corpus's short scans still run to several batches


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    """tools/jpeg_sync_host_check.cpp with -fsanitize=address,undefined, as a program of its own (no preloading)."""
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    exe = str(tmp_path_factory.mktemp("synccheck") / "jpeg_sync_host_check")
    cmd = [clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "spnet_amd", "csrc"), os.path.join(ROOT, "tools", "jpeg_sync_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_sync_check(exe, datas, directory, seg_bytes, lanes=LANES):
    """[(sync status, serial status, workspaces equal)] of files decoded in ONE plan, and the most rounds a batch took.
    The sanitizers must have stayed silent."""
    infos = [J.parse_jpeg(d) for d in datas]
    assert all(i.device for i in infos), [i.host_reason for i in infos]
    plan = J.plan_decode(infos)
    plan_path = os.path.join(directory, "plan.bin")
    with open(plan_path, "wb") as f:
        f.write(np.array([plan["blob"].size, plan["intervals"].shape[0], len(infos), plan["tables"].shape[0],
                          plan["quant"].shape[0], plan["blocks"], infos[0].height, infos[0].width], np.int64).tobytes())
        for key in ("intervals", "files", "tables", "quant", "blob"):
            f.write(plan[key].tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, plan_path, str(seg_bytes), str(lanes)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr and not r.stderr, \
        r.stderr[-3000:]
    lines = r.stdout.splitlines()
    out = [tuple(int(v) for v in line.split()[3::2]) for line in lines if line.startswith("file ")]
    assert len(out) == len(datas) and lines[-1].startswith("rounds ")
    return out, int(lines[-1].split()[1])


# ----------------------------------------------------------------------------- the corpus
@pytest.mark.parametrize("seg_bytes", SEGS)
def test_sync_equals_serial_on_the_corpus(host_check, tmp_path, seg_bytes):
    """Every device-eligible case (both encoders, every option, table set and sampling), every interval through the
    emulated workgroup: status 0 and decode_interval's workspace."""
    for shape in C.SHAPES:
        cases = [c for c in C.corpus() if c.shape == shape and J.parse_jpeg(c.data).device]
        assert len(cases) >= 48
        out, _ = run_sync_check(host_check, [c.data for c in cases], str(tmp_path), seg_bytes)
        wrong = [(c.name, o) for c, o in zip(cases, out) if o != (0, 0, 1)]
        assert not wrong, wrong[:10]


# ----------------------------------------------------------------------------- boundaries, stated from the bytes alone
def _boundary_frame(shape, kind, sub, seed):
    kw = dict(quality=100)
    if sub is not None:
        kw["subsampling"] = sub
    return C.pillow_jpeg(C.content(kind, shape, seed), **kw)


def _split_ff00(data, seg_bytes):
    """Segment boundaries that fall between an FF and the 00 stuffed behind it."""
    lo, hi = scan_bounds(data)
    return [p for p in range(lo, hi - 1) if data[p] == 0xFF and data[p + 1] == 0 and (p + 1 - lo) % seg_bytes == 0]


@pytest.mark.parametrize("shape,sub", [((40, 64), None), ((48, 64, 3), 2)], ids=["grey", "420"])
def test_segment_boundaries_in_ff00_and_blocks_across_segments(host_check, tmp_path, shape, sub):
    seg = 4
    # the seed is searched here, on the CPU: the first whose scan has a segment boundary inside an FF 00 pair
    data = next(d for d in (_boundary_frame(shape, "noise", sub, s) for s in range(40)) if _split_ff00(d, seg))
    lo, hi = scan_bounds(data)
    info = J.parse_jpeg(data)
    assert info.restart == 0 and (info.hs, info.vs) == ((2, 2) if sub == 2 else (1, 1))
    assert len(_split_ff00(data, seg)) >= 1
    # a block of more than 2 * 32 bits touches three segments of 32 bits at least; the scan's data bits (stuffed zeros
    # and at most 7 pad bits taken off) over its blocks is the mean block, and some block is no shorter than the mean
    stuffed = sum(1 for p in range(lo, hi - 1) if data[p] == 0xFF and data[p + 1] == 0)
    mean_bits = (8 * (hi - lo - stuffed) - 7) / info.blocks
    assert mean_bits > 2 * 8 * seg, mean_bits
    assert (hi - lo + seg - 1) // seg > LANES                                     # and several batches
    out, _ = run_sync_check(host_check, [data], str(tmp_path), seg)
    assert out == [(0, 0, 1)]
    # flat: DC-only blocks of a few bits -- more blocks than twice the segments, so several finish inside one segment
    flat = _boundary_frame(shape, "flat", sub, 0)
    flo, fhi = scan_bounds(flat)
    assert J.parse_jpeg(flat).blocks > 2 * ((fhi - flo + seg - 1) // seg)
    out, _ = run_sync_check(host_check, [flat], str(tmp_path), seg)
    assert out == [(0, 0, 1)]


# ----------------------------------------------------------------------------- damaged input
@pytest.mark.parametrize("seg_bytes", (4, 32))
def test_damaged_files_get_the_serial_decoders_status(host_check, tmp_path, seg_bytes):
    bad, sound = C.damaged()
    names = sorted(bad)
    out, _ = run_sync_check(host_check, [sound] + [bad[n] for n in names] + [sound], str(tmp_path), seg_bytes)
    assert out[0] == (0, 0, 1) and out[-1] == (0, 0, 1)
    for n, (status, serial, _) in zip(names, out[1:-1]):
        assert serial != 0 and status == serial, (n, status, serial)              # the same code on the corpus kinds
    bad, sound = pillow_damaged()
    names = sorted(bad)
    out, _ = run_sync_check(host_check, [sound] + [bad[n] for n in names] + [sound], str(tmp_path), seg_bytes)
    assert out[0] == (0, 0, 1) and out[-1] == (0, 0, 1)
    for n, (status, serial, _) in zip(names, out[1:-1]):
        assert (status != 0) == (serial != 0), (n, status, serial)
    by_name = dict(zip(names, out[1:-1]))
    assert by_name["cut"][1] == 4 and by_name["garbage"][1] == 5 and by_name["cut"][0] != 0 and by_name["garbage"][0] != 0


def test_sync_survives_a_flip_of_every_byte_of_a_scan(host_check, tmp_path):
    """Every byte of a small scan without restart markers flipped in turn, all in one plan: the sanitizers stay silent,
    a file is rejected exactly when the serial decoder rejects it, and where both accept the workspaces are equal."""
    sound = C.pillow_jpeg(C.content("noise", (16, 16), 9), quality=50)
    lo, hi = scan_bounds(sound)
    datas = []
    for p in range(lo, hi):
        d = bytearray(sound)
        d[p] ^= 0xFF
        if J.parse_jpeg(bytes(d)).device:
            datas.append(bytes(d))
    assert len(datas) > (hi - lo) // 2
    for seg_bytes in (4, 32):
        out, _ = run_sync_check(host_check, datas, str(tmp_path), seg_bytes)
        assert sum(1 for s, _, _ in out if s != 0) > len(out) // 2
        for k, (status, serial, equal) in enumerate(out):
            assert (status != 0) == (serial != 0), (k, status, serial)
            if status == 0:
                assert equal == 1, k


def test_the_chain_settles_early_on_ordinary_frames(host_check, tmp_path):
    """What the speed rests on (it is measured on the GPU): on a frame with ordinary statistics a lane that started from
    a guess falls in with the true decode, so a batch settles in far fewer rounds than it has lanes."""
    yy, xx = np.mgrid[0:96, 0:128]
    frame = (110 + 70 * np.cos(np.hypot(xx - 50, yy - 40) ** 2 / 300) + np.random.default_rng(1).normal(0, 12, (96, 128)))
    data = C.pillow_jpeg(np.clip(frame, 0, 255).astype(np.uint8), quality=90)
    lo, hi = scan_bounds(data)
    assert (hi - lo) // 64 >= 64
    out, rounds = run_sync_check(host_check, [data], str(tmp_path), 64, lanes=64)
    assert out == [(0, 0, 1)] and rounds <= 16, rounds


# ----------------------------------------------------------------------------- host logic
def _infos():
    by_name = {c.name: c for c in C.corpus()}
    names = ["19x37-noise-q90-ours", "19x37-noise-q90-pillow-optimize-sNone", "19x37-ramp-q10-ours",
             "19x37-noise-q100-pillow-plain-sNone"]
    return [J.parse_jpeg(by_name[n].data) for n in names]


def test_default_plan_is_unchanged_and_the_split_plan_loses_nothing():
    infos = _infos()
    plan = J.plan_decode(infos)
    assert sorted(plan) == ["blob", "blocks", "files", "intervals", "quant", "tables"]
    assert plan["intervals"].shape[0] % 64 == 0 and plan["intervals"].shape[0] == 64 * plan["tables"].shape[0]
    real = plan["intervals"][plan["intervals"][:, 4] > 0]
    assert real.shape[0] == 3 + 1 + 3 + 1
    sizes = real[:, 1] - real[:, 0]
    for cut in (0, int(np.sort(sizes)[4]), int(sizes.max()) + 1):
        split = J.plan_decode(infos, cut)
        for key in ("blob", "files", "tables", "quant"):
            assert np.array_equal(split[key], plan[key]), key
        assert split["blocks"] == plan["blocks"]
        lane = split["intervals"][split["intervals"][:, 4] > 0]
        sync = split["sync_intervals"]
        assert sync.dtype == np.int32 and sync.shape[1] == 8 and (sync[:, 4] > 0).all()          # no padding
        assert ((sync[:, 1] - sync[:, 0]) >= cut).all() and ((lane[:, 1] - lane[:, 0]) < cut).all()
        both = sorted(map(tuple, np.concatenate([lane, sync]).tolist()))
        assert both == sorted(map(tuple, real.tolist()))                          # every interval in exactly one list
        assert split["intervals"].shape[0] % 64 == 0
    assert J.plan_decode(infos, 0)["intervals"].shape[0] == 0


def test_our_own_files_keep_the_lane_kernel():
    """SYNC_MIN_BYTES is above the longest interval this project's encoder writes for a 384 x 512 frame: an MCU row of
    512 pixels of noise at quality 100."""
    row = jpeg_ref.encode_jpeg(C.content("noise", (8, 512), 3), 100)
    bounds = J.parse_jpeg(row).bounds
    assert bounds.shape[0] == 1
    assert J.SYNC_MIN_BYTES > int(bounds[0][1] - bounds[0][0])
    assert J.DEFAULT_ENTROPY in J.ENTROPY_MODES and J.SYNC_SEG_BYTES % 4 == 0 and 4 <= J.SYNC_SEG_BYTES <= 4096


def test_entropy_argument_checks_come_before_the_gpu(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("the GPU was asked for"))
    data = C.corpus()[0].data
    path = str(tmp_path / "a.jpg")
    with open(path, "wb") as f:
        f.write(data)
    it = iter([data])
    with J.MjpegWriter(str(tmp_path / "m.avi"), 37, 19, channels=1, encoder=lambda frames: [next(it) for _ in frames]) as w:
        w.add(np.zeros((1, 19, 37), np.uint8))
    reader = J.MjpegReader(str(tmp_path / "m.avi"))
    for bad in (dict(entropy="fast"), dict(entropy=1), dict(seg_bytes=6), dict(seg_bytes=0), dict(seg_bytes=8192),
                dict(entropy="sync", seg_bytes=2.5)):
        for call in (lambda kw: J.decode_jpeg_device([data], **kw), lambda kw: J.read_jpeg_device([path], **kw),
                     lambda kw: J.read_frames_device([path], **kw), lambda kw: reader.read_device(**kw)):
            with pytest.raises(ValueError, match="entropy|seg_bytes"):
                call(bad)
