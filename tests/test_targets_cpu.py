"""Host halves of the device target codec (csrc/targets.hip): the two tables the host hands the kernel must hold exactly
what the host codec computes itself, or the device could not have its bits."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trig_table_is_the_codecs_own_cos_and_sin():
    from spnet_amd import augmentation as A
    t = A.trig_2deg_table()
    assert t.shape == (360, 2) and t.dtype == np.float32
    # one ellipse per whole degree through the host codec: its cos 2t / sin 2t entries, denormalised (range 2, mean 0)
    rows = np.zeros((360, 1, 6))
    rows[:, 0] = [100.0, 100.0, 30.0, 20.0, 0.0, 3.0]
    rows[:, 0, 4] = np.arange(360)
    Y, overflow = A._encode_targets(rows, np.ones(360, np.int32))
    assert not overflow.any()
    cell = Y.reshape(360, 6, 6, 2, 8)[:, 0, 1, 0]           # (100 - 40) / 71 = 0, (100 - 40) / 51 = 1
    np.testing.assert_array_equal(cell[:, 4] * np.float32(2), t[:, 0])
    np.testing.assert_array_equal(cell[:, 5] * np.float32(2), t[:, 1])


def test_warp_fwd_holds_warp_metadatas_matrices():
    from spnet_amd import augmentation as A
    p = A.new_warp_params([0, 1, 2], 384, 512)
    A.set_warp(p, 0, -1, 12.5, 3, -4)
    A.set_warp(p, 2, 1, -20.0, 0, 0)
    f = A.warp_fwd(p)
    assert f.shape == (3, 8) and f.dtype == np.float64
    for j, a in enumerate((12.5, 0.0, -20.0)):
        want = A.rotation_matrix_2d((256.0, 192.0), a, 1.0).reshape(6) if a else np.array([1.0, 0, 0, 0, 1.0, 0])
        assert f[j, :6].tobytes() == want.tobytes() and f[j, 6] == a and f[j, 7] == 0


def test_header_declares_the_entry_point():
    from spnet_amd import _abi
    with open(os.path.join(ROOT, "include", "spnet_hip.h")) as fh:
        sigs = _abi.parse_header(fh.read())
    assert len(sigs["spnet_encode_targets"][1]) == 15
