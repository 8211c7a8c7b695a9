"""The device JPEG encoder (csrc/jpeg.hip through spnet_amd/jpeg.py) against its numpy restatement (tests/helpers/jpeg_ref.py,
itself held to Pillow in tests/test_jpeg_cpu.py): the interval sizes and the scan byte for byte through the raw entry points,
with sentinels before, between and behind the slots, and the whole file through encode_jpeg_device; then batch
independence, slot discipline, the argument checks, the movie writer on device frames and one command-line run.

Shapes are the smallest at which the kernel can still go wrong: one block; a batch of three; both sizes off the 8-grid in
colour; 65 blocks in a row (past a wave and the interval cap: intervals run across the row end); 9 MCU rows (markers up to
RST7) and 11 (RST7 is followed by RST0 again);
uniform noise at quality 100 (stuffed FF 00 pairs); the 0/255 checkerboard at 100 (largest magnitudes); a constant frame
(EOB-only blocks); a ramp at quality 10 that emits ZRL -- 5x + 15y in uint8, which wraps at 256: a ramp that never wraps
emits no ZRL at any slope (slopes 0 .. 36 in both directions were searched), the wrap lines leave the lone high coefficient
a ZRL needs."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests.helpers import jpeg_ref as R

pytestmark = pytest.mark.gpu

BASE = 3            # the first slot starts here: not word aligned
GAP = 5             # unwritten bytes at the end of every slot: the guard between two scans
PAD = 64            # sentinel bytes behind the last slot
SENTINEL = 0xA5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _cases():
    rng = np.random.default_rng(21)
    yy, xx = np.mgrid[0:16, 0:24]
    board = ((np.indices((16, 24)).sum(0) & 1) * 255).astype(np.uint8)
    return {
        "one_block": (rng.integers(0, 256, (1, 8, 8), dtype=np.uint8), 90),
        "batch_of_three": (rng.integers(0, 256, (3, 16, 24), dtype=np.uint8), 90),
        "colour_off_grid": (rng.integers(0, 256, (2, 13, 21, 3), dtype=np.uint8), 90),
        "wide_65_blocks": (rng.integers(0, 256, (1, 8, 520), dtype=np.uint8), 90),
        "tall_9_rows": (rng.integers(0, 256, (1, 72, 8), dtype=np.uint8), 90),
        "tall_11_rows": (rng.integers(0, 256, (1, 88, 8), dtype=np.uint8), 90),
        "noise_q100_colour": (rng.integers(0, 256, (1, 16, 16, 3), dtype=np.uint8), 100),
        "checkerboard_q100": (np.stack([board, 255 - board]), 100),
        "constant": (np.full((1, 16, 24), 77, np.uint8), 90),
        "ramp_q10": (((5 * xx + 15 * yy) & 255).astype(np.uint8)[None], 10),
    }


CASES = _cases()


@pytest.fixture(scope="module")
def reference():
    """name -> per frame (scan bytes, interval sizes, stats) of the helper; computed once, never changed."""
    _need_gpu()
    return {name: [R.encode_scan(f, q) for f in batch] for name, (batch, q) in CASES.items()}


def _encode(batch, quality, shrink=None):
    """Both kernels on a [N, ...] host batch through the raw entry points: slots GAP bytes larger than the scans (shrink: the
    frame whose slot is one byte too SMALL instead), sentinels everywhere.  The whole buffer comes back."""
    from spnet_amd import jpeg as J
    dev = torch.from_numpy(batch).cuda()
    sizes, sizes_dev = J.interval_sizes(dev, quality)
    exact = np.diff(J.scan_offsets(sizes))
    slots = exact + GAP
    if shrink is not None:
        slots[shrink] = exact[shrink] - 1
    offsets = np.concatenate([[BASE], BASE + np.cumsum(slots)]).astype(np.int64)
    buf = torch.full((int(offsets[-1]) + PAD,), SENTINEL, dtype=torch.uint8, device="cuda")
    J.pack_frames(dev, sizes_dev, offsets, quality, out=buf)
    return dict(sizes=sizes, exact=exact, offsets=offsets, out=buf.cpu().numpy())


def _check_guards(res, skip=None):
    out, off = res["out"], res["offsets"]
    assert (out[:BASE] == SENTINEL).all() and (out[int(off[-1]):] == SENTINEL).all() and out.size - int(off[-1]) == PAD
    for n in range(len(res["exact"])):
        if n != skip:
            assert (out[int(off[n]) + int(res["exact"][n]):int(off[n + 1])] == SENTINEL).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_scan_and_pack_equal_the_reference(name, reference):
    from spnet_amd import jpeg as J
    batch, quality = CASES[name]
    res = _encode(batch, quality)
    for n, (scan, sizes, stats) in enumerate(reference[name]):
        assert np.array_equal(res["sizes"][n], sizes)                               # every interval's exact size
        assert int(res["exact"][n]) == len(scan)
        lo = int(res["offsets"][n])
        assert res["out"][lo:lo + len(scan)].tobytes() == scan                      # byte for byte
    _check_guards(res)
    stats = reference[name][0][2]
    if name == "noise_q100_colour":
        assert stats["stuffed"] > 0 and b"\xff\x00" in reference[name][0][0]        # stuffing is exercised
    if name == "ramp_q10":
        assert stats["zrl"] > 0
    if name == "checkerboard_q100":
        assert stats["ac_category"] >= 9 and stats["dc_category"] >= 1
    if name == "constant":
        assert stats["ac_category"] == 0 and stats["eob"] == 6
    if name == "tall_9_rows":
        assert len(reference[name][0][1]) == 9 and reference[name][0][0].count(b"\xff\xd7") >= 1          # up to RST7
    if name == "tall_11_rows":                                                      # 10 markers: RST7 is followed by RST0, RST1
        scan, sizes = reference[name][0][:2]
        at = int(sizes[:9].sum()) + 2 * 8
        assert scan[at:at + 2] == b"\xff\xd0" and scan[at - int(sizes[8]) - 2:at - int(sizes[8])] == b"\xff\xd7"
    if name == "wide_65_blocks":
        assert len(reference[name][0][1]) == 2
    # the public encoder: the whole file, and Pillow reads it
    files = J.encode_jpeg_device(torch.from_numpy(batch).cuda(), quality)
    assert files == [R.encode_jpeg(f, quality) for f in batch]
    im = Image.open(io.BytesIO(files[0]))
    im.load()
    assert im.size == (batch.shape[2], batch.shape[1]) and im.mode == ("L" if batch.ndim == 3 else "RGB")
    again = _encode(batch, quality)
    assert np.array_equal(again["out"], res["out"]) and np.array_equal(again["sizes"], res["sizes"])       # two runs


def test_a_frames_bytes_do_not_depend_on_the_batch():
    _need_gpu()
    from spnet_amd import jpeg as J
    rng = np.random.default_rng(3)
    for shape in ((16, 24), (13, 21, 3)):
        frame = rng.integers(0, 256, shape, dtype=np.uint8)
        others = rng.integers(0, 256, (2,) + shape, dtype=np.uint8)
        alone = J.encode_jpeg_device(torch.from_numpy(frame[None]).cuda())
        third = J.encode_jpeg_device(torch.from_numpy(np.concatenate([others, frame[None]])).cuda())
        assert alone[0] == third[2] == R.encode_jpeg(frame, 90) and third[0] != third[2]


def test_a_slot_one_byte_too_small_loses_bytes_only_inside_itself(reference):
    batch, quality = CASES["batch_of_three"]
    res = _encode(batch, quality, shrink=1)
    off = res["offsets"]
    for n, (scan, _, _) in enumerate(reference["batch_of_three"]):
        lo = int(off[n])
        if n == 1:
            assert int(off[2]) - lo == len(scan) - 1
            assert res["out"][lo:int(off[2])].tobytes() == scan[:-1]                # the last byte is dropped, nothing else
        else:
            assert res["out"][lo:lo + len(scan)].tobytes() == scan
    _check_guards(res, skip=1)


def test_entry_points_refuse_bad_arguments():
    _need_gpu()
    from spnet_amd import _lib as L
    src = torch.zeros(64 * 3, dtype=torch.uint8, device="cuda")
    qt = torch.ones(128, dtype=torch.int16, device="cuda")
    sizes = torch.full((16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, 32], dtype=torch.int64, device="cuda")
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    s = L.current_stream()
    p, q, z, o, b = src.data_ptr(), qt.data_ptr(), sizes.data_ptr(), offs.data_ptr(), out.data_ptr()
    for bad in ((1, 8, 8, 2), (1, 8, 8, 4), (1, 8, 8, 0), (1, 0, 8, 1), (1, 8, 0, 1), (-1, 8, 8, 1), (1, 65536, 8, 1),
                (1, 8, 65536, 3)):
        with pytest.raises(L.HipError):
            L.spnet_jpeg_scan(p, *bad, q, z, s)
        with pytest.raises(L.HipError):
            L.spnet_jpeg_pack(p, *bad, q, z, o, b, 64, s)
    for args in ((0, 1, 8, 8, 1, q, z), (p, 1, 8, 8, 1, 0, z), (p, 1, 8, 8, 1, q, 0), (p, 1, 8, 8, 1, q + 1, z),
                 (p, 1, 8, 8, 1, q, z + 2)):
        with pytest.raises(L.HipError):
            L.spnet_jpeg_scan(*args, s)                                             # NULL or misaligned
    good = [p, 1, 8, 8, 1, q, z, o, b, 64]
    for k, v in ((0, 0), (5, 0), (6, 0), (7, 0), (8, 0), (5, q + 1), (6, z + 1), (7, o + 4), (9, -1)):
        args = list(good)
        args[k] = v
        with pytest.raises(L.HipError):
            L.spnet_jpeg_pack(*args, s)
    L.spnet_jpeg_scan(p, 0, 8, 8, 1, q, z, s)                                       # empty batch: nothing to do
    L.spnet_jpeg_pack(p, 0, 8, 8, 3, q, z, o, b, 64, s)
    torch.cuda.synchronize()
    assert (sizes.cpu().numpy() == 0x5A5A5A5A).all() and (out.cpu().numpy() == SENTINEL).all()          # nothing was launched
    from spnet_amd import jpeg as J
    assert J.encode_jpeg_device(torch.empty((0, 8, 8), dtype=torch.uint8, device="cuda")) == []
    assert J.write_jpeg_device(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda"), []) == []
    for bad in (torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device="cuda"), torch.zeros((1, 8, 8), dtype=torch.uint8),
                torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda")):
        with pytest.raises(ValueError):
            J.encode_jpeg_device(bad)


def test_writer_and_movie_on_device_frames(tmp_path):
    _need_gpu()
    from spnet_amd import jpeg as J
    rng = np.random.default_rng(8)
    frames = rng.integers(0, 256, (3, 16, 24, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    files = J.encode_jpeg_device(dev, 85)
    paths = [str(tmp_path / ("f%d.jpg" % k)) for k in range(3)]
    assert J.write_jpeg_device(dev, paths, quality=85, threads=2) == [len(f) for f in files]
    assert [open(p, "rb").read() for p in paths] == files
    movie = str(tmp_path / "m.avi")
    with J.MjpegWriter(movie, 24, 16, fps=5.0, quality=85) as w:
        w.add(dev[:1])
        w.add(dev[1:])
        with pytest.raises(ValueError):
            w.add(dev[:, :8])
    data = open(movie, "rb").read()
    avi = R.parse_avi(data)
    assert avi["total_frames"] == avi["length"] == 3 and (avi["width"], avi["height"]) == (24, 16)
    assert (avi["rate"], avi["scale"]) == (5, 1) and len(avi["index"]) == 3
    for k, chunk in enumerate(avi["frames"]):
        assert avi["movi_tag"] + avi["index"][k][2] == avi["chunk_at"][k] and avi["index"][k][3] == len(chunk)
        got = Image.open(io.BytesIO(chunk))
        assert got.mode == "RGB" and got.size == (24, 16)
        assert np.array_equal(np.asarray(got), np.asarray(Image.open(io.BytesIO(files[k]))))


def _run_cli(cmd, cwd):
    """A child process, as tests/test_cli_gpu.py starts its entry points."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, cmd[0])] + cmd[1:], cwd=cwd, env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    return r.stdout


def test_predict_command_line_writes_jpeg_files_and_a_movie(tmp_path):
    """predict_spnet.py --device_overlay --device_jpeg --movie against --device_overlay --device_png on 16 fake-ESPI frames:
    the .jpg files and no .png beside them, a movie of as many frames, the same CSV."""
    _need_gpu()
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    data = tmp_path / "frames"
    F.write_dataset(str(data) + "/", 16, seed=6)
    model = M.Model((331, 331, 1), Y0size=576, seed=8)
    model.save_weights(str(tmp_path / "w.hdf5"))
    del model
    common = ["predict_spnet.py", "-w", "w.hdf5", "-d", str(data), "-b", "8", "--device_overlay"]
    _run_cli(common + ["-l", "logs/png/", "--device_png"], str(tmp_path))
    _run_cli(common + ["-l", "logs/jpg/", "--device_jpeg", "--jpeg_quality", "80", "--movie", "strike.avi", "--movie_fps", "8"],
             str(tmp_path))
    png_dir, jpg_dir = tmp_path / "logs" / "png", tmp_path / "logs" / "jpg"
    names = sorted(os.listdir(jpg_dir))
    assert names == ["hawley_spnet.csv"] + ["steelpan_pred_%05d.jpg" % k for k in range(16)]             # and no .png
    assert sorted(os.listdir(png_dir)) == ["hawley_spnet.csv"] + ["steelpan_pred_%05d.png" % k for k in range(16)]
    assert (jpg_dir / "hawley_spnet.csv").read_bytes() == (png_dir / "hawley_spnet.csv").read_bytes()
    avi = R.parse_avi((tmp_path / "strike.avi").read_bytes())
    assert avi["total_frames"] == len(avi["frames"]) == 16 and (avi["rate"], avi["scale"]) == (8, 1)
    first = Image.open(io.BytesIO(avi["frames"][0]))
    assert first.size == (512, 384) and first.mode == "RGB"
    assert avi["frames"][0] == (jpg_dir / "steelpan_pred_00000.jpg").read_bytes()
    lossless = np.asarray(Image.open(png_dir / "steelpan_pred_00000.png")).astype(np.float64)
    err = np.asarray(first).astype(np.float64) - lossless
    assert 10 * np.log10(255.0 ** 2 / np.mean(err * err)) > 25                     # the same picture
    with pytest.raises(subprocess.CalledProcessError):
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        subprocess.run([sys.executable, os.path.join(root, "predict_spnet.py"), "--device_jpeg", "--device_png"], check=True,
                       capture_output=True, env=dict(os.environ, PYTHONPATH=root), timeout=300)          # argparse refuses
