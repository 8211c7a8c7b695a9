"""The helpers the device codecs share on the host (spnet_amd/codec_host.py): the pool rule, the staged upload's layout, the
file writer and the ordered map.  Plain CPU: stage runs with device "cpu", where the one copy is a copy in host memory."""
import os
from concurrent import futures
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from spnet_amd import codec_host as CH
from spnet_amd import jpeg as J
from spnet_amd import png as P


def test_pool_size_is_within_1_and_16_and_the_job_count():
    assert CH.MAX_THREADS == P.MAX_THREADS == J.MAX_THREADS == 16
    assert CH.pool_size(16, 512) == 16 and CH.pool_size(64, 512) == 16 and CH.pool_size(4, 512) == 4
    assert CH.pool_size(16, 3) == 3 and CH.pool_size(16, 1) == 1
    assert CH.pool_size(0, 512) == 1 and CH.pool_size(-2, 512) == 1 and CH.pool_size(16, 0) == 1


def test_stage_pads_every_part_and_the_bytes_round_trip():
    rng = np.random.default_rng(0)
    parts = [rng.integers(-2 ** 62, 2 ** 62, 5, dtype=np.int64), rng.integers(-2 ** 31, 2 ** 31, (3, 7), dtype=np.int32),
             rng.integers(0, 2 ** 16, 9, dtype=np.uint16), rng.integers(0, 256, 13, dtype=np.uint8), np.zeros(0, np.int32),
             rng.integers(0, 256, 1, dtype=np.uint8)]
    dev, starts, host = CH.stage(parts, "cpu", pinned=False, align=16)
    assert dev.dtype == host.dtype and dev.dtype.itemsize == 1 and dev.device.type == "cpu"
    assert starts == [0, 48, 144, 176, 192, 192] and all(s % 16 == 0 for s in starts)
    assert dev.numel() == 208
    got = dev.numpy()
    for s, p in zip(starts, parts):
        assert got[s:s + p.nbytes].tobytes() == p.tobytes()
        assert np.array_equal(got[s:s + p.nbytes].view(p.dtype).reshape(p.shape), p)
    # align 1: back to back, as the PNG decoder lays the streams behind their offsets
    dev, starts, _ = CH.stage(parts, "cpu", pinned=False, align=1)
    assert starts == [0, 40, 124, 142, 155, 155] and dev.numpy().tobytes() == b"".join(p.tobytes() for p in parts)


def test_stage_takes_lists_of_only_empty_parts():
    dev, starts, host = CH.stage([np.zeros(0, np.uint8), np.zeros((0, 8), np.int32)], "cpu", pinned=False, align=16)
    assert starts == [0, 0] and dev.dtype.itemsize == 1
    assert CH.stage([], "cpu", pinned=False, align=16)[1] == []


def test_write_files_returns_the_sizes_and_leaves_a_callers_pool_open(tmp_path):
    files = [(b"head", np.arange(k, dtype=np.uint8), b"", b"tail" * k) for k in range(5)]
    paths = [str(tmp_path / ("f%d.bin" % k)) for k in range(5)]
    calls = []

    def encode():
        calls.append(1)
        return lambda k: files[k]

    sizes = CH.write_files(paths, 5, encode, threads=3, pool=None, name="png")
    assert calls == [1] and sizes == [os.path.getsize(p) for p in paths] == [4 + 5 * k for k in range(5)]
    for k, p in enumerate(paths):
        with open(p, "rb") as f:
            assert f.read() == b"head" + bytes(range(k)) + b"tail" * k

    class Counting(ThreadPoolExecutor):
        maps = 0

        def map(self, *a, **kw):
            Counting.maps += 1
            return super().map(*a, **kw)

    more = [str(tmp_path / ("g%d.bin" % k)) for k in range(5)]
    with Counting(max_workers=2) as pool:
        assert CH.write_files(iter(more), 5, encode, threads=16, pool=pool, name="png") == sizes
        assert Counting.maps == 1
        assert pool.submit(lambda: 7).result() == 7            # still open
    assert CH.write_files([], 0, lambda: pytest.fail("nothing to encode"), 16, None, "png") == []


def test_write_files_refuses_a_wrong_number_of_paths_before_anything_is_encoded_or_written(tmp_path):
    paths = [str(tmp_path / "a.bin"), str(tmp_path / "b.bin")]
    for name in ("png", "jpeg"):
        with pytest.raises(ValueError) as e:
            CH.write_files(paths, 3, lambda: pytest.fail("encoded"), 16, None, name)
        assert str(e.value) == "%s: 3 frames, 2 paths" % name
    assert os.listdir(str(tmp_path)) == []


def test_map_pool_keeps_the_order_and_needs_no_pool_for_no_items(monkeypatch):
    assert CH.map_pool(lambda v: v * v, range(40), threads=5) == [v * v for v in range(40)]
    assert CH.map_pool(lambda v: v + 1, iter([3, 1, 2])) == [4, 2, 3]
    monkeypatch.setattr(CH, "ThreadPoolExecutor", lambda **kw: pytest.fail("a pool was created"))
    monkeypatch.setattr(futures, "ThreadPoolExecutor", lambda **kw: pytest.fail("a pool was created"))
    assert CH.map_pool(lambda v: pytest.fail("called"), []) == []
