"""The mask-fitting rule on the host (spnet_amd/masks.py: label_components_host, component_sums_host, rows_from_sums,
ellipses_from_masks_host, read_masks) against the flood-fill oracle of tests/helpers/mask_fit_ref.py -- exact equality of
labels and sums on every case of its table --, the stand-alone program tools/mask_fit_host_check.cpp (the kernels' union-find
and tile / border geometry of csrc/mask_fit_core.h with the lanes in a loop, under AddressSanitizer and UBSan), the
round-trip tolerances, and evaluate_spnet.py --pred_masks as far as it goes without a model and without a GPU.

ROUND-TRIP TOLERANCES.  The device fit equals the host fit bit for bit, so these judge the METHOD (moments of a pixel mask
against the painted ellipse), not a kernel, and are measured on the CPU: ellipses_from_masks_host(ring_masks_host(rows))
against rows on the full-size case's own 48 seeded rows (mask_fit_ref.fullsize_rows, a in [6, 56], b in [4, a]).  Measured
worst errors: centre 0.2823 px, axes 0.1702 px, angle 1.532 deg (angles compared where a - b >= 4: 83 % of the rows).  The
constants below are those times 1.25; the margin covers nothing but a future change of the seed."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from spnet_amd import masks as MK
from tests.helpers import mask_fit_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_CENTRE, MEASURED_AXES, MEASURED_ANGLE = 0.2822708815956297, 0.17017170587205754, 1.5319859182254447
TOL_CENTRE, TOL_AXES, TOL_ANGLE = 1.25 * MEASURED_CENTRE, 1.25 * MEASURED_AXES, 1.25 * MEASURED_ANGLE
CASES = list(range(len(R.cases())))
TOL0_CASES = [i for i in CASES if R.cases()[i].join_tol == 0]     # scipy labels one value at a time: join_tol 0 only


# ----------------------------------------------------------------------------- labels and sums
@pytest.mark.parametrize("index", CASES, ids=R.case_ids())
def test_c1_host_equals_the_oracle(index):
    c = R.cases()[index]
    R.check_construction(index)
    labels, comps = R.expected(index)
    got = MK.label_components_host(c.masks, c.join_tol)
    assert got.dtype == np.int32 and np.array_equal(got, labels)
    want_n, want_sums = R.packed(comps, c.C)
    n, sums = MK.component_sums_host(c.masks, c.join_tol, c.C)
    assert n.dtype == np.int32 and sums.dtype == np.int64 and sums.shape == (c.masks.shape[0], c.C, 8)
    assert np.array_equal(n, want_n) and np.array_equal(sums, want_sums)
    n2, sums2 = MK.component_sums_host(c.masks, c.join_tol, c.C, labels=labels)
    assert np.array_equal(n2, want_n) and np.array_equal(sums2, want_sums)


@pytest.mark.parametrize("index", TOL0_CASES, ids=[R.case_ids()[i] for i in TOL0_CASES])
def test_c2_partition_equals_scipy_at_join_tol_0(index):
    ndimage = pytest.importorskip("scipy.ndimage")
    c = R.cases()[index]
    got = MK.label_components_host(c.masks, 0)
    for b, frame in enumerate(c.masks):
        for v in np.unique(frame[frame > 0]):
            want, n = ndimage.label(frame == v, np.ones((3, 3)))
            sel = frame == v
            pairs = np.unique(np.stack([want[sel], got[b][sel]], 1), axis=0)      # a bijection between the two labellings
            assert len(pairs) == n == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1])), (c.name, b, int(v))


def test_c3_wide_sums_do_not_wrap():
    index = R.case_ids().index("wide")
    _, comps = R.expected(index)
    sxx = comps[0][0][3]
    assert sxx == sum(x * x for x in range(16384)) and sxx > 2 ** 32
    _, sums = MK.component_sums_host(R.cases()[index].masks)
    assert int(sums[0, 0, 3]) == sxx


# ----------------------------------------------------------------------------- rows_from_sums
def test_c4_rows_of_a_rectangle_in_closed_form():
    m = np.zeros((1, 9, 11), np.uint8)
    m[0, 2:5, 3:8] = 70                          # 3 rows x 5 columns, x 3 .. 7, y 2 .. 4
    rows, count = MK.ellipses_from_masks_host(m)
    assert rows.dtype == np.float64 and rows.shape == (1, 128, 6) and count.dtype == np.int32 and count.tolist() == [1]
    cx, cy, a, b, ang, rings = rows[0, 0]
    # a w x h rectangle of unit squares has variances w^2 / 12 and h^2 / 12: a = 2 sqrt(25 / 12), b = 2 sqrt(9 / 12)
    assert cx == 5.5 and cy == 3.5 and rings == 7.0 and ang == 0.0
    assert abs(a - 5.0 / np.sqrt(3.0)) < 1e-12 and abs(b - np.sqrt(3.0)) < 1e-12 and a > b
    assert not rows[0, 1:].any()
    # the same rectangle upright: the long axis is vertical, +-90 degrees
    rows, _ = MK.ellipses_from_masks_host(np.ascontiguousarray(m.transpose(0, 2, 1)))
    assert abs(abs(rows[0, 0, 4]) - 90.0) < 1e-12 and abs(rows[0, 0, 2] - 5.0 / np.sqrt(3.0)) < 1e-12
    # a single pixel: its centre, and the unit square's own variance
    one = np.zeros((1, 4, 4), np.uint8)
    one[0, 2, 1] = 25
    rows, _ = MK.ellipses_from_masks_host(one)
    assert rows[0, 0].tolist() == [1.5, 2.5, 2.0 * np.sqrt(1.0 / 12.0), 2.0 * np.sqrt(1.0 / 12.0), 0.0, 2.5]
    # a diagonal of pixels going down to the right: image y points down, so the angle is negative (the painter's sign)
    d = np.zeros((1, 8, 8), np.uint8)
    d[0, np.arange(8), np.arange(8)] = 10
    rows, _ = MK.ellipses_from_masks_host(d, join_tol=0)
    assert abs(rows[0, 0, 4] + 45.0) < 1e-12


def test_c5_rows_from_sums_min_pixels_packing_and_order():
    m = np.zeros((2, 8, 40), np.uint8)
    m[0, 1, 1] = 10                              # 1 pixel
    m[0, 1:3, 5:8] = 20                          # 6 pixels
    m[0, 4, 10:12] = 30                          # 2 pixels
    m[0, 5:8, 20:30] = 40                        # 30 pixels
    m[1, 0:2, 0:2] = 50                          # 4 pixels
    n, sums = MK.component_sums_host(m)
    assert n.tolist() == [4, 1] and sums[0, :4, 0].tolist() == [1, 6, 2, 30]
    rows, count = MK.rows_from_sums(sums, n)
    assert count.tolist() == [4, 1] and rows[0, :4, 5].tolist() == [1.0, 2.0, 3.0, 4.0]
    rows3, count3 = MK.rows_from_sums(sums, n, min_pixels=3)
    assert count3.tolist() == [2, 1] and rows3[0, :2, 5].tolist() == [2.0, 4.0] and not rows3[0, 2:].any()
    assert np.array_equal(rows3[0, 0], rows[0, 1]) and np.array_equal(rows3[0, 1], rows[0, 3])
    rows7, count7 = MK.rows_from_sums(sums, n, min_pixels=7)
    assert count7.tolist() == [1, 0] and not rows7[1].any()
    # only the first min(n, C) slots count, whatever the others hold
    junk = sums.copy()
    junk[1, 1:] = 99
    assert np.array_equal(MK.rows_from_sums(junk, n)[0], rows)
    with pytest.raises(ValueError):
        MK.rows_from_sums(sums.astype(np.int32), n)
    with pytest.raises(ValueError):
        MK.rows_from_sums(sums, n, min_pixels=0)


def test_c6_overflow_names_the_frame_or_truncates():
    index = R.case_ids().index("cap")
    c = R.cases()[index]
    masks = np.concatenate([np.zeros_like(c.masks), c.masks])
    with pytest.raises(ValueError, match="frame 1 holds 130 components"):
        MK.ellipses_from_masks_host(masks)
    rows, count = MK.ellipses_from_masks_host(masks, overflow="truncate")
    assert count.tolist() == [0, 128]
    assert rows[1, :, 0].tolist() == [2.0 * (i % 65) + 0.5 for i in range(128)]          # the first 128 in raster order
    rows, count = MK.ellipses_from_masks_host(masks, max_components=16, overflow="truncate")
    assert rows.shape == (2, 16, 6) and count.tolist() == [0, 16]
    for bad in (dict(join_tol=256), dict(join_tol=-1), dict(max_components=0), dict(max_components=129), dict(min_pixels=0),
                dict(overflow="drop")):
        with pytest.raises(ValueError):
            MK.ellipses_from_masks_host(masks, **bad)
    with pytest.raises(TypeError):
        MK.label_components_host(masks.astype(np.int32))


# ----------------------------------------------------------------------------- the round trip
def test_c7_round_trip_within_the_measured_tolerances():
    rows, count = R.fullsize_rows()
    gap = np.abs(rows[..., 2] - rows[..., 3])
    assert (gap >= 4.0).mean() >= 0.5                       # a condition on the inputs: enough rows have an angle to compare
    painted = MK.ring_masks_host(rows, count, R.FULL_H, R.FULL_W)
    fit_rows, fit_count = MK.ellipses_from_masks_host(painted)
    assert fit_count.tolist() == [12] * R.FULL_B
    e_centre, e_axes, e_angle, share = R.roundtrip_errors(rows, count, fit_rows, fit_count)    # also: rings exactly
    print("round trip: centre %.4f px, axes %.4f px, angle %.4f deg (%.0f %% of the rows)"
          % (e_centre, e_axes, e_angle, 100 * share))
    assert share >= 0.5
    assert e_centre <= TOL_CENTRE and e_axes <= TOL_AXES and e_angle <= TOL_ANGLE
    # rows -> mask -> rows -> mask: what the fit loses at the rim, as the pixel metric sees it
    again = MK.ring_masks_host(fit_rows[:, :12], fit_count, R.FULL_H, R.FULL_W)
    res = MK.compare_masks_host(again, painted, tol=0)
    assert res["ring_acc"] == 1.0 and res["object_iou"] > 0.9


# ----------------------------------------------------------------------------- files and the command line
def test_c8_read_masks_and_missing_file(tmp_path):
    m = np.zeros((2, 6, 9), np.uint8)
    m[0, 1:3, 2:5] = 30
    m[1, 4, 4] = 110
    paths = [str(tmp_path / ("m%d.png" % i)) for i in range(2)]
    MK.write_masks(m, paths)
    assert np.array_equal(MK.read_masks(paths), m)
    gone = str(tmp_path / "steelpan_0000007.png")
    with pytest.raises(FileNotFoundError, match="steelpan_0000007.png"):
        MK.read_masks(paths + [gone])
    assert MK.read_masks([]).shape[0] == 0


def _run_evaluate(args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_spnet.py")] + args, cwd=ROOT, capture_output=True,
                          text=True, timeout=300)


def test_c10_pred_masks_arguments(tmp_path):
    r = _run_evaluate(["--help"])
    assert r.returncode == 0 and "--pred_masks" in r.stdout and "--mask_join_tol" in r.stdout and "--mask_min_pixels" in r.stdout
    r = _run_evaluate(["-d", str(tmp_path), "--pred_masks", str(tmp_path), "--mask_join_tol", "256"])
    assert r.returncode == 2 and "--mask_join_tol is 0 .. 255" in r.stderr
    r = _run_evaluate(["-d", str(tmp_path), "--pred_masks", str(tmp_path), "--mask_min_pixels", "0"])
    assert r.returncode == 2 and "--mask_min_pixels is at least 1" in r.stderr
    r = _run_evaluate(["-d", str(tmp_path), "--pred_masks", str(tmp_path / "nowhere")])
    assert r.returncode == 2 and "nowhere" in r.stderr


def test_c11_pred_masks_missing_file_is_named(tmp_path):
    import evaluate_spnet as E
    data, pred = tmp_path / "Val", tmp_path / "pred"
    data.mkdir()
    pred.mkdir()
    files = [str(data / ("steelpan_%07d.png" % i)) for i in range(3)]
    assert E.pred_mask_paths(files, str(pred)) == [str(pred / ("steelpan_%07d.png" % i)) for i in range(3)]
    MK.write_masks(np.zeros((2, 4, 4), np.uint8), E.pred_mask_paths(files[:2], str(pred)))
    with pytest.raises(FileNotFoundError, match="steelpan_0000002.png"):
        E.read_pred_masks(files, str(pred))
    assert E.read_pred_masks(files[:2], str(pred)).shape == (2, 4, 4)


# ----------------------------------------------------------------------------- the kernels' core under sanitizers
def test_c12_core_under_sanitizers_equals_a_flood_fill(tmp_path):
    """tools/mask_fit_host_check.cpp with -fsanitize=address,undefined, as a program of its own (no preloading)."""
    clang = next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(p)), None)
    clang = clang or shutil.which("clang++")
    if clang is None:
        pytest.skip("no clang++")
    exe = str(tmp_path / "mask_fit_host_check")
    cmd = [clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(ROOT, "spnet_amd", "csrc"), os.path.join(ROOT, "tools", "mask_fit_host_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and not r.stderr, (r.stdout[-1000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert lines[-1] == "all equal" and len(lines) > 70 and all(l.endswith("equal 1") for l in lines[:-1])
