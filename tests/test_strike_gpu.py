"""csrc/espi_strike.hip against the numpy host rule (fake_espi.strike_params_host) and the Python-integer oracle
(tests/helpers/track_score_ref.py strike): every array bit for bit.  The kernel has one thread per slot and no tiling; the
sizes cover one block and several (7 S T above and below 256), T of 1, 2 and 4096, J of 0 and 8."""
import numpy as np
import pytest
import torch

from spnet_amd import fake_espi as F
from tests.helpers import track_score_ref as R
from tests.test_strike_cpu import hostile_base

pytestmark = pytest.mark.gpu
INVALID = "hipError_t 1$"
GUARD, CANARY = 8, 0x7E7E7E7E


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Guarded:
    """A device array of n 4-byte elements with canary words around it, pre-filled with the canary's neighbour pattern."""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device="cuda")
        self.buf[GUARD:GUARD + n] = 0x5A5A5A5A
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def host(self, shape):
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == CANARY).all() and (h[GUARD + self.n:] == CANARY).all(), "a canary was overwritten"
        return h[GUARD:GUARD + self.n].view(self.dtype).reshape(shape).copy()

    def untouched(self):
        return (self.host((-1,)).view(np.int32) == 0x5A5A5A5A).all()


def _raw(base, T, seed, J, first=0):
    from spnet_amd import _lib as L
    w0, n0, c0 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in base)
    S = len(base[2])
    out = Guarded(S * T * 5, np.float32), Guarded(S * T * 56, np.float32), Guarded(S * T, np.int32), Guarded(S * T * 7, np.int32)
    L.spnet_fake_espi_strike(w0.data_ptr(), n0.data_ptr(), c0.data_ptr(), first, S, T, seed, J, *(g.ptr for g in out),
                             L.current_stream())
    return tuple(g.host(s) for g, s in zip(out, ((S * T, 5), (S * T, 7, 8), (S * T,), (S * T, 7))))


def _same(got, want):
    for g, w in zip(got, want):
        w = np.asarray(w)
        assert g.shape == w.shape and np.array_equal(g.view(np.int32), w.astype(g.dtype).view(np.int32))   # bits: -0.0, NaN


@pytest.mark.parametrize("T,J,seed,first", [(1, 0, 0, 0), (2, 8, 1, 0), (9, 3, 0xFFFFFFFF, 5), (16, 8, 7, 306783370)])
def test_g1_entry_point_equals_the_host_rule_and_the_oracle(T, J, seed, first):
    _need_gpu()
    for base in (R.base_params(5, 11), hostile_base()):
        got = _raw(base, T, seed, J, first)
        _same(got, F.strike_params_host(*base, T, seed, J, first))
        want = R.strike(*base, T, seed, J, first)
        _same(got, (np.asarray(want[0], np.float32), np.asarray(want[1], np.float32).reshape(-1, 7, 8),
                    np.asarray(want[2], np.int32), np.asarray(want[3], np.int32)))


def test_g2_T_4096_on_one_sequence():
    _need_gpu()
    base = R.base_params(1, 4)
    _same(_raw(base, 4096, 3, 8), F.strike_params_host(*base, 4096, 3, 8))


def test_g3_strike_params_device_on_drawn_bases_any_split():
    _need_gpu()
    S, T = 9, 6
    whole = F.strike_params_device(S, T, seed=21, jitter=4)
    base = tuple(a.cpu().numpy() for a in F.draw_params_device(S, 21))
    _same([a.cpu().numpy() for a in whole], F.strike_params_host(*base, T, 21, 4))
    for lo, hi in ((0, 1), (1, 5), (5, 9)):
        part = F.strike_params_device(hi - lo, T, seed=21, jitter=4, first_sequence=lo)
        assert all(torch.equal(w[lo * T:hi * T], p) for w, p in zip(whole, part))
    ident = whole[3].cpu().numpy().reshape(S, T, 7)
    assert (ident[:, 0].max(1) > 0).all()                              # every struck note is there at frame 0
    rows_d = F.strike_rows(*whole[1:])
    rows_h = F.strike_rows(*(a.cpu().numpy() for a in whole[1:]))
    assert all(np.array_equal(d.cpu().numpy(), h) and d.cpu().numpy().dtype == h.dtype for d, h in zip(rows_d, rows_h))


def test_g4_no_sequences_and_invalid_arguments_write_nothing():
    _need_gpu()
    from spnet_amd import _lib as L
    base = R.base_params(2, 3)
    w0, n0, c0 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in base)
    out = Guarded(64, np.float32), Guarded(512, np.float32), Guarded(16, np.int32), Guarded(64, np.int32)
    w, n, c, i = (g.ptr for g in out)
    st = L.current_stream()
    good = [w0.data_ptr(), n0.data_ptr(), c0.data_ptr(), 0, 2, 4, 5, 0, w, n, c, i]
    L.spnet_fake_espi_strike(*(good[:4] + [0] + good[5:]), st)          # S == 0 succeeds
    bad = [good[:p] + [None] + good[p + 1:] for p in (0, 1, 2, 8, 9, 10, 11)]
    for pos, values in ((3, (-1, 306783377)), (4, (-1,)), (5, (0, -1, 4097)), (7, (-1, 9))):
        bad += [good[:pos] + [v] + good[pos + 1:] for v in values]
    bad.append(good[:4] + [1 << 20, 4096] + good[6:])                   # S * T beyond int32
    for args in bad:
        with pytest.raises(L.HipError, match=INVALID):
            L.spnet_fake_espi_strike(*args, st)
    torch.cuda.synchronize()
    assert all(g.untouched() for g in out)
    assert [tuple(a.shape) for a in F.strike_params_device(0, 4)] == [(0, 5), (0, 7, 8), (0,), (0, 7)]
    with pytest.raises(ValueError):
        F.strike_params_device(2, 4097)


def test_g5_generate_strike_device_rasterises_its_own_parameters():
    _need_gpu()
    S, T = 2, 4
    X, (rows, count), ident, U = F.generate_strike_device(S, T, seed=3, jitter=1, noise=False, want_u8=True)
    waves, nodes, nnode, ident_p = F.strike_params_device(S, T, seed=3, jitter=1)
    _, _, U2 = F.generate_device(S * T, 3, noise=False, want_u8=True, params=(waves, nodes, nnode))
    assert torch.equal(U, U2) and tuple(X.shape) == (S * T, F.IM_H, F.IM_W, 1)
    r, c, i = F.strike_rows(nodes, nnode, ident_p)
    assert torch.equal(rows, r) and torch.equal(count, c) and torch.equal(ident, i)
    # an absent antinode is not drawn: a frame in which an identity is missing differs from the frame before or after
    U = U.cpu().numpy()
    ident = ident.cpu().numpy()
    changed = [n for n in range(1, T) if set(ident[n]) != set(ident[n - 1])]
    assert all((U[n] != U[n - 1]).any() for n in changed)
    one_by_one = F.generate_strike_device(S, T, seed=3, jitter=1, noise=False, want_u8=True, chunk=3)[3]
    assert np.array_equal(one_by_one.cpu().numpy(), U)
