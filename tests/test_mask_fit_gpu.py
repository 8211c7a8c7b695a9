"""csrc/mask_fit.hip through spnet_amd/masks.py against the flood-fill oracle (tests/helpers/mask_fit_ref.py): labels and sums
exactly equal, and ellipses_from_masks_device bit for bit equal to ellipses_from_masks_host.

The kernels' tile is 64 x 16, so the border cases of the table sit at x = 63 | 64 and y = 15 | 16.  Shapes are the smallest
at which the kernels can still go wrong: 1 x 1, 1 x 200, 200 x 1, 16 x 64 (exactly one tile), 33 x 130 (three tiles each way,
partial tiles, W % 16 != 0, frames that are not 16-byte aligned in a batch), 48 x 192 for the chains that cross every tile,
1 x 16,384 for sums beyond 32 bits; one full-size case.  The oracle's answers are computed once (mask_fit_ref.expected)."""
import numpy as np
import pytest
import torch

from spnet_amd import masks as MK
from tests.helpers import mask_fit_ref as R

pytestmark = pytest.mark.gpu
INVALID = "hipError_t 1$"           # hipErrorInvalidValue
CASES = list(range(len(R.cases())))
FILL = 0xA5


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _raw(case, label_offset=0, sums_offset=0):
    """Both entry points on output arrays pre-filled with 0xA5, `*_offset` ELEMENTS past the start of their buffers; returns
    (labels, n, sums, the elements around the three arrays)."""
    from spnet_amd import _lib as L
    B, H, W = case.masks.shape
    C = case.C
    masks = torch.from_numpy(case.masks).cuda()
    lab = torch.full((4 * (B * H * W + 8),), FILL, dtype=torch.uint8, device="cuda").view(torch.int32)
    n = torch.full((4 * (B + 8),), FILL, dtype=torch.uint8, device="cuda").view(torch.int32)
    sums = torch.full((8 * (B * C * 8 + 8),), FILL, dtype=torch.uint8, device="cuda").view(torch.int64)
    st = L.current_stream()
    L.spnet_mask_label(masks.data_ptr(), B, H, W, case.join_tol, lab.data_ptr() + 4 * label_offset, st)
    L.spnet_mask_moments(masks.data_ptr(), lab.data_ptr() + 4 * label_offset, B, H, W, C, n.data_ptr() + 4,
                         sums.data_ptr() + 8 * sums_offset, st)
    lab_h, n_h, sums_h = lab.cpu().numpy(), n.cpu().numpy(), sums.cpu().numpy()
    lo, hi = label_offset, label_offset + B * H * W
    so, sh = sums_offset, sums_offset + B * C * 8
    around = [lab_h[:lo], lab_h[hi:], n_h[:1], n_h[1 + B:], sums_h[:so], sums_h[sh:]]
    return lab_h[lo:hi].reshape(B, H, W), n_h[1:1 + B], sums_h[so:sh].reshape(B, C, 8), around


def _untouched(around):
    return all((a.view(np.uint8) == FILL).all() for a in around)


@pytest.mark.parametrize("index", CASES, ids=R.case_ids())
def test_g1_labels_and_sums_equal_the_oracle(index):
    _need_gpu()
    c = R.cases()[index]
    R.check_construction(index)
    want_labels, comps = R.expected(index)
    want_n, want_sums = R.packed(comps, c.C)
    labels, n, sums, around = _raw(c, label_offset=1, sums_offset=1)     # 4 / 8 bytes past an aligned address: all that is asked
    assert np.array_equal(labels, want_labels)
    assert np.array_equal(n, want_n)
    assert np.array_equal(sums, want_sums)                               # slots beyond min(n, C) are ZERO, not 0xA5
    assert _untouched(around)
    # through the module, on aligned tensors
    masks = torch.from_numpy(c.masks).cuda()
    lab_d = MK.label_components_device(masks, c.join_tol)
    assert lab_d.dtype == torch.int32 and np.array_equal(lab_d.cpu().numpy(), want_labels)
    n_d, sums_d = MK.component_sums_device(masks, c.join_tol, c.C, labels=lab_d)
    assert n_d.dtype == torch.int32 and sums_d.dtype == torch.int64
    assert np.array_equal(n_d.cpu().numpy(), want_n) and np.array_equal(sums_d.cpu().numpy(), want_sums)
    n_d, sums_d = MK.component_sums_device(c.masks, c.join_tol, c.C)       # a host array is uploaded; labels made inside
    assert np.array_equal(n_d.cpu().numpy(), want_n) and np.array_equal(sums_d.cpu().numpy(), want_sums)


@pytest.mark.parametrize("index", CASES, ids=R.case_ids())
def test_g2_device_rows_equal_host_rows_bit_for_bit(index):
    _need_gpu()
    c = R.cases()[index]
    for min_pixels in (1, 3):
        want_rows, want_count = MK.ellipses_from_masks_host(c.masks, c.join_tol, min_pixels, c.C, overflow="truncate")
        rows, count = MK.ellipses_from_masks_device(torch.from_numpy(c.masks).cuda(), c.join_tol, min_pixels, c.C,
                                                    overflow="truncate")
        assert rows.is_cuda and rows.dtype == torch.float64 and count.dtype == torch.int32
        assert np.array_equal(count.cpu().numpy(), want_count)
        assert np.array_equal(rows.cpu().numpy().view(np.uint64), want_rows.view(np.uint64))


def test_g3_cap_raises_naming_the_frame_or_truncates():
    _need_gpu()
    c = R.cases()[R.case_ids().index("cap")]
    masks = torch.from_numpy(np.concatenate([np.zeros_like(c.masks), c.masks])).cuda()
    with pytest.raises(ValueError, match="frame 1 holds 130 components"):
        MK.ellipses_from_masks_device(masks)
    rows, count = MK.ellipses_from_masks_device(masks, overflow="truncate")
    assert count.tolist() == [0, 128]
    assert rows[1, :, 0].tolist() == [2.0 * (i % 65) + 0.5 for i in range(128)]
    assert rows[1, :, 1].tolist() == [2.0 * (i // 65) + 0.5 for i in range(128)]


def test_g4_empty_batch_and_argument_errors():
    _need_gpu()
    from spnet_amd import _lib as L
    st = L.current_stream()
    H, W, C = 16, 64, 4
    masks = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    labels = torch.full((H * W + 4,), 7, dtype=torch.int32, device="cuda")
    n = torch.full((4,), 7, dtype=torch.int32, device="cuda")
    sums = torch.full((C * 8 + 4,), 7, dtype=torch.int64, device="cuda")
    m, l, nn, s = masks.data_ptr(), labels.data_ptr(), n.data_ptr(), sums.data_ptr()
    # B == 0 succeeds and launches nothing
    L.spnet_mask_label(m, 0, H, W, 0, l, st)
    L.spnet_mask_moments(m, l, 0, H, W, C, nn, s, st)
    assert tuple(MK.label_components_device(masks[:0]).shape) == (0, H, W)
    rows, count = MK.ellipses_from_masks_device(masks[:0])
    assert tuple(rows.shape) == (0, 128, 6) and tuple(count.shape) == (0,)
    for args in ((None, 1, H, W, 0, l), (m, 1, H, W, 0, None), (m, 1, 0, W, 0, l), (m, 1, H, 0, 0, l), (m, 1, 16385, W, 0, l),
                 (m, 1, H, 16385, 0, l), (m, 1, H, W, 256, l), (m, 1, H, W, -1, l), (m, -1, H, W, 0, l), (m, 1, H, W, 0, l + 2)):
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_mask_label(*args, st)
    for args in ((None, l, 1, H, W, C, nn, s), (m, None, 1, H, W, C, nn, s), (m, l, 1, H, W, C, None, s),
                 (m, l, 1, H, W, C, nn, None), (m, l, 1, H, W, 0, nn, s), (m, l, 1, H, W, 129, nn, s), (m, l, 1, 0, W, C, nn, s),
                 (m, l, 1, H, 16385, C, nn, s), (m, l, -1, H, W, C, nn, s), (m, l + 2, 1, H, W, C, nn, s),
                 (m, l, 1, H, W, C, nn + 2, s), (m, l, 1, H, W, C, nn, s + 4)):
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_mask_moments(*args, st)
    torch.cuda.synchronize()
    assert (labels == 7).all() and (n == 7).all() and (sums == 7).all()          # nothing was launched
    for bad in (dict(join_tol=256), dict(max_components=0), dict(max_components=129), dict(min_pixels=0), dict(overflow="x")):
        with pytest.raises(ValueError):
            MK.ellipses_from_masks_device(masks, **bad)
    with pytest.raises(TypeError):
        MK.label_components_device(masks.int())


def test_g5_full_size_painted_by_the_device_and_fitted_there():
    _need_gpu()
    rows, count = R.fullsize_rows()
    rows_d, count_d = torch.from_numpy(rows).cuda(), torch.from_numpy(count).cuda()
    painted = MK.ring_masks_device(rows_d, count_d, H=R.FULL_H, W=R.FULL_W)
    fit_rows, fit_count = MK.ellipses_from_masks_device(painted)
    assert fit_count.tolist() == [12] * R.FULL_B
    painted_h = painted.cpu().numpy()
    want_rows, want_count = MK.ellipses_from_masks_host(painted_h)
    assert np.array_equal(fit_count.cpu().numpy(), want_count)
    assert np.array_equal(fit_rows.cpu().numpy().view(np.uint64), want_rows.view(np.uint64))
    assert np.array_equal(MK.label_components_device(painted).cpu().numpy(), MK.label_components_host(painted_h))
    # rings exactly, every row within the round-trip tolerances of tests/test_mask_fit_cpu.py
    from tests.test_mask_fit_cpu import TOL_ANGLE, TOL_AXES, TOL_CENTRE
    e_centre, e_axes, e_angle, share = R.roundtrip_errors(rows, count, fit_rows.cpu().numpy(), want_count)
    assert share >= 0.5 and e_centre <= TOL_CENTRE and e_axes <= TOL_AXES and e_angle <= TOL_ANGLE
    # and the loop closes: the fitted rows go into the grid codec as they are
    from spnet_amd.augmentation import encode_targets_device
    Y, flags = encode_targets_device(fit_rows[:, :16].contiguous(), fit_count)
    assert tuple(Y.shape) == (R.FULL_B, 576) and not flags.any()
