"""csrc/audio.hip through the raw entry point and through spnet_amd/audio.py against the numpy twin (note_envelopes_host,
which tests/test_audio_cpu.py holds to the Python-integer oracle): exact equality of re and im, element for element.  No
tolerance appears anywhere.

Shapes are the smallest at which the kernel can still go wrong: S = 3 with len (0, 50, L); T 1, 5 and 37 (one frame, less
than a group of 8, four groups and a partial one); Wn 64, 192 (neither a power of two nor a multiple of the workgroup),
2048 (the default) and 8192 (the whole table; one frame a group at hop 441/10 and beyond); K 1, 5, 7 and 64 (fewer units
than waves, and sixteen rounds); hops 1/1, 441/10 and 300/1 (overlapping windows, a fraction, gaps at Wn 64); offsets
before the recording, at its start and ten samples before its end."""
import numpy as np
import pytest
import torch

from spnet_amd import audio as AU

pytestmark = pytest.mark.gpu
INVALID = "hipError_t 1$"           # hipErrorInvalidValue
L_REC = 9000
GUARD, SENTINEL, CANARY = 8, 0x5A5A5A5A5A5A5A5A, 0x7E7E7E7E7E7E7E7E


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def recording():
    """(pcm int16 [3, L], len (0, 50, L)) with full-scale samples among the random ones; never modified."""
    pcm = np.random.RandomState(7).randint(-32768, 32768, (3, L_REC)).astype(np.int16)
    pcm[:, ::97], pcm[:, 5::89] = -32768, 32767
    pcm.setflags(write=False)
    return pcm, np.array([0, 50, L_REC], np.int32)


def _steps(K):
    f = np.concatenate([[261.63, 1000.5, 3000.0, 0.0, 23999.0, 440.0, 523.25], np.linspace(100.0, 20000.0, 57)])
    return AU.note_steps(f[:K], 48000)


class Guarded:
    """An int64 device array of n elements with GUARD canary words before and after it, pre-filled with a sentinel."""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int64, device="cuda")
        self.buf[GUARD:GUARD + n] = SENTINEL
        self.ptr = self.buf.data_ptr() + 8 * GUARD

    def host(self, shape, written=True):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + self.n:] == CANARY).all(), "a canary was overwritten"
        body = h[GUARD:GUARD + self.n].reshape(shape).copy()
        assert not written or not (body == SENTINEL).any(), "an element was not written"
        return body


def _raw(pcm, lens, T, hop, offset, steps, win, ctab=None):
    """The entry point itself into guarded, pre-filled arrays: (re, im) int64 [S, T, K] on the host."""
    from spnet_amd import _lib as L
    ctab = AU.cos_table() if ctab is None else ctab
    S, K = pcm.shape[0], len(steps)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in
           (pcm, np.asarray(lens, np.int32), win, np.asarray(steps, np.uint32).view(np.int32), ctab)]
    re, im = Guarded(S * T * K), Guarded(S * T * K)
    L.spnet_note_envelopes(dev[0].data_ptr(), dev[1].data_ptr(), S, pcm.shape[1], T, offset, hop[0], hop[1], dev[2].data_ptr(),
                           len(win), dev[3].data_ptr(), K, dev[4].data_ptr(), re.ptr, im.ptr, L.current_stream())
    torch.cuda.synchronize()
    return re.host((S, T, K)), im.host((S, T, K))


CASES = [(1, 64, 1, (1, 1), 0), (5, 192, 5, (441, 10), -100), (37, 64, 5, (300, 1), 0), (37, 192, 64, (441, 10), L_REC - 10),
         (5, 8192, 5, (441, 10), 0), (37, 8192, 1, (1, 1), -100), (5, 64, 64, (300, 1), L_REC - 10), (37, 2048, 7, (240, 1), 0),
         (1, 8192, 64, (1, 1), 0), (37, 192, 1, (300, 1), -100), (1, 192, 5, (1, 1), L_REC - 10), (5, 64, 1, (441, 10), 0)]


@pytest.mark.parametrize("T,Wn,K,hop,offset", CASES, ids=["T%d-Wn%d-K%d-hop%d_%d-off%d" % (c[0], c[1], c[2], c[3][0], c[3][1], c[4])
                                                          for c in CASES])
def test_g1_device_equals_host_exactly(recording, T, Wn, K, hop, offset):
    _need_gpu()
    pcm, lens = recording
    win = AU.window_table(Wn)
    want = AU.note_envelopes_host(pcm, lens, T, hop, offset, _steps(K), win)
    got = _raw(pcm, lens, T, hop, offset, _steps(K), win)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert not got[0][0].any() and not got[1][0].any()                     # len 0
    assert want[0][2].any()                                                # the case is not empty


def test_g2_the_magnitude_bound(recording):
    """All samples -32768 with step 0 at Wn 8192: the Hann table, and a window of 32767 throughout (the largest sum the
    limits allow): the exact integers."""
    _need_gpu()
    pcm = np.full((1, 8192), -32768, np.int16)
    hann, flat = AU.window_table(8192), np.full(8192, 32767, np.int16)
    re, im = _raw(pcm, [8192], 1, (1, 1), 0, [0], hann)
    assert int(re[0, 0, 0]) == -32768 * 16384 * int(hann.astype(np.int64).sum()) and int(im[0, 0, 0]) == 0
    re, im = _raw(pcm, [8192], 1, (1, 1), 0, [0, 0], flat)
    assert re[0, 0].tolist() == [-32768 * 32767 * 16384 * 8192] * 2 and im[0, 0].tolist() == [0, 0]
    # any int16 content of the tables: the same sums as the twin
    rng = np.random.RandomState(3)
    ctab, win = (rng.randint(-32768, 32768, n).astype(np.int16) for n in (4096, 192))
    want = AU.note_envelopes_host(recording[0], recording[1], 5, (441, 10), 0, _steps(5), win, ctab)
    got = _raw(recording[0], recording[1], 5, (441, 10), 0, _steps(5), win, ctab)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_g3_independent_of_the_split(recording):
    """S = 3 in one call equals three calls of S = 1; T = 37 equals T = 20 followed by T = 17 with the offset advanced to
    frame 20's start.  Through note_envelopes_device, which also takes the recording as a device tensor."""
    _need_gpu()
    pcm, lens = recording
    win, steps, hop, off = AU.window_table(192), _steps(5), (441, 10), -100
    whole = [a.cpu().numpy() for a in AU.note_envelopes_device(pcm, lens, 37, hop, off, steps, win)]
    want = AU.note_envelopes_host(pcm, lens, 37, hop, off, steps, win)
    assert whole[0].dtype == np.int64 and np.array_equal(whole[0], want[0]) and np.array_equal(whole[1], want[1])
    pcm_d = torch.from_numpy(np.array(pcm)).cuda()
    for s in range(3):
        one = AU.note_envelopes_device(pcm_d[s:s + 1], torch.from_numpy(lens[s:s + 1]).cuda(), 37, hop, off, steps, win)
        assert np.array_equal(one[0].cpu().numpy()[0], whole[0][s]) and np.array_equal(one[1].cpu().numpy()[0], whole[1][s])
    head = AU.note_envelopes_device(pcm_d, lens, 20, hop, off, steps, win)
    tail = AU.note_envelopes_device(pcm_d, lens, 17, hop, off + (20 * hop[0]) // hop[1], steps, win)
    for c in range(2):
        assert np.array_equal(np.concatenate([head[c].cpu().numpy(), tail[c].cpu().numpy()], 1), whole[c])
    empty = AU.note_envelopes_device(pcm[:0], None, 4, hop, off, steps, win)
    assert tuple(empty[0].shape) == (0, 4, 5) and empty[0].dtype == torch.int64


def test_g4_every_limit_is_refused_and_nothing_is_written(recording):
    _need_gpu()
    from spnet_amd import _lib as L
    pcm, lens = recording
    win, steps = AU.window_table(8192), _steps(64)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (pcm, lens, win, steps.view(np.int32), AU.cos_table())]
    p = [d.data_ptr() for d in dev]
    re, im = Guarded(3 * 5 * 64), Guarded(3 * 5 * 64)
    st = L.current_stream()
    #        pcm   len   S  L      T  offset hop    win   Wn  step  K  ctab  re      im
    good = [p[0], p[1], 3, L_REC, 5, 0, 441, 10, p[2], 192, p[3], 5, p[4], re.ptr, im.ptr]
    I31, T20, O40 = 1 << 31, 1 << 20, 1 << 40
    bad = [(0, None), (1, None), (8, None), (10, None), (12, None), (13, None), (14, None),       # NULL pointers
           (2, -1), (4, 0), (4, -3), (4, T20 + 1), (9, 63), (9, 8193), (9, 0), (11, 0), (11, 65), (11, -1), (3, 0), (3, -5),
           (3, I31), (6, 0), (6, -1), (6, I31), (7, 0), (7, -2), (7, I31), (5, O40 + 1), (5, -O40 - 1),
           (13, re.ptr + 4), (14, im.ptr + 2), (1, p[1] + 2), (10, p[3] + 1)]                       # not aligned to the element
    for index, value in bad:
        args = list(good)
        args[index] = value
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_note_envelopes(*args, st)
    for S, T, K in ((33, T20, 64), (2049, T20, 1), (I31 - 1, 2, 1)):                               # S T K > 2^31 - 1
        args = list(good)
        args[2], args[4], args[11] = S, T, K
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_note_envelopes(*args, st)
    torch.cuda.synchronize()
    assert (re.host((3, 5, 64), written=False) == SENTINEL).all() and (im.host((3, 5, 64), written=False) == SENTINEL).all()
    # the limits themselves are inside: S == 0 does nothing, the largest offset and a hop of 2^31 - 1 are taken
    for index, value in ((2, 0), (5, O40), (5, -O40), (6, I31 - 1), (7, I31 - 1)):
        args = list(good)
        args[index] = value
        L.spnet_note_envelopes(*args, st)
    torch.cuda.synchronize()
    body = re.host((3, 5, 64), written=False).reshape(-1)
    assert not (body[:3 * 5 * 5] == SENTINEL).any() and (body[3 * 5 * 5:] == SENTINEL).all()
    # the host side refuses the same sizes before anything is uploaded
    with pytest.raises(ValueError):
        AU.note_envelopes_device(pcm, lens, 0, (441, 10), 0, _steps(5), AU.window_table(192))
    with pytest.raises(ValueError):
        AU.note_envelopes_device(pcm, lens, 5, (441, 10), 0, _steps(5), np.zeros(63, np.int16))
    with pytest.raises(TypeError):
        AU.note_envelopes_device(pcm.astype(np.int32), lens, 5, (441, 10), 0, _steps(5), AU.window_table(192))


def test_g5_the_float_step_is_shared(recording):
    """envelope() of the device sums and of the host sums: the same bits, and the amplitude of a full-scale sine."""
    _need_gpu()
    n = np.arange(6000)
    pcm = np.stack([np.rint(30000 * np.sin(2 * np.pi * 440.0 * n / 48000)), np.rint(900 * np.cos(2 * np.pi * 523.25 * n / 48000))])
    pcm = pcm.astype(np.int16)
    win, steps = AU.window_table(2048), AU.note_steps([440.0, 523.25], 48000)
    dev = AU.envelope(*AU.note_envelopes_device(pcm, None, 9, (240, 1), 0, steps, win), win)
    host = AU.envelope(*AU.note_envelopes_host(pcm, None, 9, (240, 1), 0, steps, win), win)
    assert dev.dtype == np.float64 and dev.shape == (2, 9, 2) and np.array_equal(dev.view(np.uint64), host.view(np.uint64))
    assert np.all(np.abs(dev[0, :, 0] - 15000) < 30) and np.all(np.abs(dev[1, :, 1] - 450) < 2)
    one = AU.note_curves(pcm[0], 48000, [("A4", 440.0, 0.0, 0.0), ("C5", 523.25, 0.0, 0.0)], 9, 200)
    assert np.array_equal(one, host[0]) and np.array_equal(AU.note_curves(pcm[0], 48000, [("A4", 440.0, 0, 0)], 9, 200, host=True),
                                                           host[0][:, :1])
