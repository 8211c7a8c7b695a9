"""The host side of the device PNG encoder (spnet_amd/png.py) and its specification (tests/helpers/png_ref.py), without a
GPU: the length-limited prefix code, the block header, the helper's whole streams against zlib and Pillow, the container's
CRCs, and the product's host functions against the helper."""
import heapq
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from tests.helpers import png_ref as R


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def _hist(levels):
    """{grey level: count} -> [256]."""
    h = np.zeros(256, np.int64)
    for v, c in levels.items():
        h[v] = c
    return h


def _histograms():
    r = np.random.RandomState(2)
    noise = np.clip(r.normal(40, 40, 384 * 512), 0, 255).astype(np.uint8)
    return {
        "single_literal": _hist({0: 272}),
        "two_literals": _hist({0: 16, 9: 200}),
        "three_literals": _hist({0: 1, 77: 1}),                # a 1x1 frame: filter byte, pixel (+ end of block)
        "all_256_flat": np.full(256, 12, np.int64),
        "all_256_random": r.randint(1, 4000, 256).astype(np.int64),
        "fibonacci_20": R.histogram(R.filtered_stream(R.fibonacci_frame())).astype(np.int64),     # the GPU tests' frame
        "fibonacci_30": _hist({0: 384, **{10 + k: c for k, c in enumerate(_fib(30))}}),
        "espi_noise": np.bincount(noise, minlength=256).astype(np.int64) + _hist({0: 384}),
        "skewed_full": np.concatenate([[10 ** 7], np.arange(1, 256)]).astype(np.int64),
    }


def _huffman_cost_and_depth(freq):
    """An independent Huffman (heapq over (weight, depth)): the optimal cost, and the depth of the tree this run built."""
    heap = [(int(f), 0) for f in freq if f > 0]
    if len(heap) == 1:
        return heap[0][0], 1
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return cost, heap[0][1]


@pytest.mark.parametrize("name", sorted(_histograms()))
def test_code_lengths_are_a_complete_limited_prefix_code(name):
    from spnet_amd import png as P
    hist = _histograms()[name]
    lengths = P.huffman_code_lengths(hist)
    freq = [int(c) for c in hist] + [1]
    assert lengths.shape == (257,)
    used = [s for s in range(257) if freq[s] > 0]
    assert all(lengths[s] == 0 for s in range(257) if freq[s] == 0)
    assert all(1 <= lengths[s] <= 15 for s in used)
    assert len(used) >= 2 and sum(2 ** (15 - int(lengths[s])) for s in used) == 2 ** 15       # Kraft sum 1, in integers
    cost, depth = _huffman_cost_and_depth(freq)
    mine = sum(freq[s] * int(lengths[s]) for s in used)
    if depth <= 15:
        assert mine == cost
    else:
        assert mine >= cost
    assert list(lengths) == R.literal_lengths(hist)                        # the helper restates the same construction
    if name == "single_literal":
        assert lengths[0] == 1 and lengths[256] == 1
    if name.startswith("fibonacci"):
        assert depth > 15 and max(lengths) == 15                           # the limiter is what is being tested


def test_limiter_meets_other_limits_too():
    from spnet_amd import png as P
    freq = _fib(19)                                                        # the code-length alphabet's size, natural depth 18
    for limit in (5, 7, 9):
        ln = P._limited_lengths(freq, limit)
        assert max(ln) <= limit and sum(2 ** (limit - v) for v in ln) == 2 ** limit
        assert ln == R.code_lengths(freq, limit)
    with pytest.raises(ValueError):
        P._limited_lengths([1] * 40, 5)


def test_canonical_codes_follow_the_rfc_example():
    from spnet_amd import png as P
    lengths = [3, 3, 3, 3, 3, 2, 4, 4]                                     # RFC 1951 section 3.2.2, symbols A .. H
    want = [0b010, 0b011, 0b100, 0b101, 0b110, 0b00, 0b1110, 0b1111]
    assert list(P.canonical_codes(lengths)) == want
    assert R.canonical(lengths) == want


@pytest.fixture(scope="module")
def frames():
    r = np.random.RandomState(7)
    out = dict(R.small_frames())
    out["grey_noise_96x128"] = np.clip(r.normal(40, 40, (96, 128)), 0, 255).astype(np.uint8)
    out["rgb_40x33"] = r.randint(0, 256, (40, 33, 3)).astype(np.uint8)
    return out


@pytest.fixture(scope="module")
def encoded(frames):
    return {k: R.zlib_stream(v) for k, v in frames.items()}


def test_helper_streams_inflate_to_the_filtered_stream(frames, encoded):
    for name, (z, info) in encoded.items():
        assert zlib.decompress(z) == info["stream"].tobytes(), name        # inflate also verifies the Adler-32 trailer
        assert info["adler"] == zlib.adler32(info["stream"].tobytes()), name
        assert len(z) == 2 + (info["nbits"] + 7) // 8 + 4, name
        assert len(z) <= -(-9 * info["stream"].size // 8) + 1024, name     # the size bound the GPU tests rely on
        assert int(info["hist"].sum()) == info["stream"].size and info["hist"][0] >= frames[name].shape[0]


def test_helper_png_opens_to_the_same_pixels_and_its_crcs_hold(frames, encoded):
    for name, frame in frames.items():
        png = R.png_bytes(frame, encoded[name][0])
        im = Image.open(io.BytesIO(png))
        im.load()
        assert im.mode == ("L" if frame.ndim == 2 else "RGB") and im.size == (frame.shape[1], frame.shape[0])
        assert np.array_equal(np.asarray(im), frame), name
        chunks = R.read_chunks(png)
        assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        for tag, data, crc in chunks:
            assert crc == zlib.crc32(data, zlib.crc32(tag)), (name, tag)
        assert struct.unpack(">IIBBBBB", chunks[0][1]) == (frame.shape[1], frame.shape[0], 8, 0 if frame.ndim == 2 else 2, 0, 0, 0)


def test_product_host_functions_match_the_helper(frames, encoded):
    from spnet_amd import png as P
    names = sorted(frames)
    plan = P.plan_frames(np.stack([encoded[k][1]["hist"] for k in names]))
    assert plan["offsets"][0] == 0
    for i, name in enumerate(names):
        z, info = encoded[name]
        assert list(plan["lengths"][i]) == info["lengths"], name
        assert list(plan["codes"][i] & 0xffff) == info["codes"] and list(plan["codes"][i] >> 16) == info["lengths"], name
        nbits = int(plan["header_bits"][i])
        words = plan["header"][i]
        bits = [(int(words[k // 32]) >> (k % 32)) & 1 for k in range(nbits)]
        assert bits == info["header_bits"], name
        assert nbits <= 32 * P.HEADER_WORDS and not any(int(w) >> 0 for w in words[(nbits + 31) // 32:])
        assert int(plan["offsets"][i + 1] - plan["offsets"][i]) == len(z), name      # the exact size, known before packing
        frame = frames[name]
        assert P.png_container(z, frame.shape[1], frame.shape[0], 1 if frame.ndim == 2 else 3) == R.png_bytes(frame, z), name


def test_device_entry_points_refuse_host_arrays():
    from spnet_amd import png as P
    with pytest.raises(ValueError):
        P.encode_png_device(np.zeros((1, 4, 4), np.uint8))
