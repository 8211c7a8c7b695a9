"""The LZ77 stage of the PNG encoder without a GPU: the restated token rule and bit writer (tests/helpers/png_lz_ref.py)
against zlib and Pillow, and production's host plan (spnet_amd.png.plan_frames_lz: codes, header, exact sizes, the
per-frame choice) against streams assembled from the helper's tokens.

Bound for the all-equal frame (derived, not measured).  A segment holds 1024 stream bytes and the parse restarts at its
start; in a stream of equal bytes every position but the very first has the distance-1 candidate, whose length is cut only
by 258 and by the segment's end, so a segment is at most 1 literal + ceil(1023 / 258) = 4 matches = 5 tokens.  A token is at
most 15 + 5 + 15 + 13 = 48 bits, the header at most 3 + 14 + 19 * 3 + 316 * 7 = 2286 bits, the end of block 15:
    bytes <= 2 + ceil((2286 + 48 * 5 * ceil(L / 1024) + 15) / 8) + 4
The all-zero 64 x 64 frame (L = 4160, filter bytes included, 5 segments) must stay under 2 + ceil(3501 / 8) + 4 = 444."""
import io
import zlib

import numpy as np
import pytest
from PIL import Image

from tests.helpers import png_lz_ref as Z
from tests.helpers import png_ref as R

NAMES = sorted(Z.lz_frames()) + ["noise_rgb_48x64x3"]


@pytest.fixture(scope="module")
def frames():
    out = dict(Z.lz_frames())
    r = np.random.RandomState(2)
    grey = (np.clip(np.rint(128 + r.normal(40, 40, (48, 64))), 0, 255) * r.randint(0, 2, (48, 64))).astype(np.uint8)
    out["noise_rgb_48x64x3"] = np.stack([grey] * 3, axis=2)
    return out


@pytest.fixture(scope="module")
def reference(frames):
    return {k: Z.lz_stream(v) for k, v in frames.items()}


def _production_plan(info):
    from spnet_amd import png as P
    S = info["stream"]
    return P.plan_frames_lz(R.histogram(S)[None], info["lhist"][None], info["dhist"][None])


@pytest.mark.parametrize("name", NAMES)
def test_helper_stream_is_a_valid_png(name, frames, reference):
    frame = frames[name]
    lz, info = reference[name]
    assert zlib.decompress(lz) == info["stream"].tobytes()
    im = Image.open(io.BytesIO(R.png_bytes(frame, lz)))
    im.load()
    assert np.array_equal(np.asarray(im), frame)
    for p, n, d in info["tokens"]:                                           # the rule's limits
        if n:
            assert 3 <= n <= 258 and 1 <= d <= min(p, 32768) and p // 1024 == (p + n - 1) // 1024
    assert sum(n or 1 for _, n, _ in info["tokens"]) == info["stream"].size


@pytest.mark.parametrize("name", NAMES)
def test_production_plan_on_the_helper_tokens(name, frames, reference):
    """Production's codes, header and sizes, the helper's tokens and bit writer: the stream decompresses and is exactly as
    long as planned; the plan's choice is the smaller stream and never longer than the literal-only one."""
    from spnet_amd import png as P
    frame = frames[name]
    lz, info = reference[name]
    plan = _production_plan(info)
    ll, dl = [int(v) for v in plan["llengths"][0]], [int(v) for v in plan["dlengths"][0]]
    assert ll == list(info["ll"]) and dl == list(info["dl"])                # two constructions, one code
    lc, dc = [int(v) for v in P.canonical_codes(ll)], [int(v) for v in P.canonical_codes(dl)]
    assert [int(v) & 0xffff for v in plan["lcodes"][0]] == lc and [int(v) >> 16 for v in plan["lcodes"][0]] == ll
    assert [int(v) & 0xffff for v in plan["dcodes"][0]] == dc and [int(v) >> 16 for v in plan["dcodes"][0]] == dl
    acc, nbits = P.lz_block_header(ll, dl)
    head = [(acc >> k) & 1 for k in range(nbits)]
    assert head == info["header_bits"] and nbits <= 2286
    built, _ = Z.assemble(info["stream"], info["tokens"], ll, lc, dl, dc, head)
    assert built == lz and zlib.decompress(built) == info["stream"].tobytes()
    assert len(built) == int(plan["lz_sizes"][0])
    literal = R.zlib_stream(frame)[0]
    assert int(plan["literal_sizes"][0]) == len(literal)
    chosen, took_lz, _ = Z.chosen_stream(frame)
    assert bool(plan["use_lz"][0]) == took_lz == (len(lz) < len(literal))
    assert int(plan["offsets"][1]) == len(chosen) <= len(literal)
    assert int(plan["lz_header_bits"][0]) == (nbits if took_lz else -1)


def test_the_frames_exercise_what_they_are_for(reference):
    tok = {k: v[1]["tokens"] for k, v in reference.items()}
    assert all(n == 0 for _, n, _ in tok["grey_1x1"] + tok["rgb_3x5"])       # no match: the HDIST edge case
    assert not reference["rgb_3x5"][1]["dhist"].any()
    zeros = reference["zeros_64x64"][1]
    assert zeros["lhist"][285] > 0 and zeros["dhist"][0] > 0 and zeros["dhist"][1:].sum() == 0     # one distance symbol
    assert (0, 0, 0) == tok["zeros_64x64"][0] and (1, 258, 1) == tok["zeros_64x64"][1]
    assert 2 in {d for _, n, d in tok["period2_7x13"] if n} and 3 in {d for _, n, d in tok["period3_7x13"] if n}
    assert any(n and d % 3 == 0 for _, n, d in tok["replicated_16x24x3"])
    assert [(n, d) for _, n, d in tok["far_32768"] if d > 1024] == [(199, 32768)]
    assert all(d <= 1024 for _, n, d in tok["far_32769"])                   # one byte too far: it stays literals
    assert [d for _, n, d in tok["tile_repeat_17000"] if n >= 83] == [16384] * 3
    # the Fibonacci frame: with matches its two codes come out 13 and 9 deep, so nothing is limited on the LZ side; its LZ
    # stream is the longer one and the frame takes the fallback, whose literal code IS limited (16 deep before)
    fib = reference["fibonacci"][1]
    assert max(fib["ll"]) <= 15 and max(fib["dl"]) <= 15 and fib["dhist"].sum() > 1000
    assert max(R.code_lengths(list(R.histogram(fib["stream"])) + [1], 64)) == 16


def test_all_equal_frame_stays_under_the_derived_bound(reference):
    lz, info = reference["zeros_64x64"]
    L = info["stream"].size
    assert L == 4160
    assert len(info["tokens"]) <= 5 * -(-L // 1024)
    assert len(lz) <= 2 + -(-(2286 + 48 * 5 * -(-L // 1024) + 15) // 8) + 4 == 444


def test_plan_of_a_batch_mixes_both_paths(frames):
    from spnet_amd import png as P
    batch = R.batch_of(frames["zeros_64x64"], 5)
    infos = [Z.lz_stream(f)[1] for f in batch]
    plan = P.plan_frames_lz(np.stack([R.histogram(i["stream"]) for i in infos]), np.stack([i["lhist"] for i in infos]),
                            np.stack([i["dhist"] for i in infos]))
    assert plan["use_lz"].any() and not plan["use_lz"].all()
    want = [len(Z.chosen_stream(f)[0]) for f in batch]
    assert np.diff(plan["offsets"]).tolist() == want
    with pytest.raises(ValueError):
        P.plan_frames_lz(np.zeros((2, 256)), np.zeros((1, 286)), np.zeros((2, 30)))
    with pytest.raises(ValueError):
        P.lz_block_header([0] * 257, [0] * 30)
