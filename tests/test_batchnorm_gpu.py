"""The BatchNorm family of csrc/bn.hip, kernel by kernel through the C ABI: every partial-sum kernel (c3, small, vec), both
apply kernels, the finalize kernels (direct, sliced, folded into the apply pass), the split entry points, ReLU6, the
activation boundaries, ill-conditioned channels and the refusals.

Every output buffer is pre-filled with NaN and followed by a 4 KiB guard band that must stay NaN; so are the columns
between the blocks of the `_ld` forms.  Every comparison takes one of the three forms of tests/test_small_kernels_gpu.py,
named in the comment next to it:
  (1) bit equality, where the code claims it or the result is a select;
  (2) exact-sum inputs: integer-valued x in [-8, 8] (dy in [-4, 4]), gamma / invstd powers of two, beta / mean integers:
      every partial sum is an integer (a multiple of 1/2 in the backward) below 2^24 in any order, so the statistics
      must equal tests/helpers/bn_ref.py's finalize_bits, and dgamma / dbeta the float64 sums, bit for bit -- one dropped,
      doubled or mis-strided row changes a sum by an integer;
  (3) a forward-error bound against the float64 reference on the same fp32 inputs, (n + 2) * 2^-24 * sum|terms| with n
      counted from the kernel's chain of roundings, or a bound propagated through such chains (section 4).
Constants quoted from bn.hip: BN_MAX_PARTS 256, BN_FIN_CH 16, BN_SLICE_MIN_P 1024, BN_SLICES 64, BN_FUSE_CH 32,
BN_FUSE_MAX_P 128 (512 while M*C <= 4 Mi), slabs of >= 64 rows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import bn_ref as B


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


NAN = float("nan")
U = 2.0 ** -24            # unit roundoff of fp32
GUARD = 1024              # floats behind every output: 4 KiB that must stay NaN
EPS, MOM = 1e-3, 0.99
MM0, MV0 = 0.3, 0.7       # moving statistics before the update: momentum * these is inexact, so a product fused into the
                          # sum would show in the bits


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()


def st():
    return torch.cuda.current_stream().cuda_stream


class Bufs:
    """NaN-prefilled (or initialised) device buffers, each followed by GUARD floats that must stay NaN"""

    def __init__(self):
        self.bufs = []

    def new(self, shape, init=None):
        n = int(np.prod(shape))
        buf = torch.full((n + GUARD,), NAN, device="cuda")
        view = buf[:n].view(shape)
        if init is not None:
            view.copy_(torch.as_tensor(init))
        self.bufs.append(buf)
        return view

    def guards_untouched(self):
        return all(bool(torch.isnan(b[b.numel() - GUARD:]).all()) for b in self.bufs)

    def all_nan(self):
        return all(bool(torch.isnan(b).all()) for b in self.bufs)


def bits_equal(got, want):
    """form (1): the same fp32 bits (want: numpy fp32 or a tensor)"""
    g = got.detach().cpu().numpy()
    w = want.detach().cpu().numpy() if torch.is_tensor(want) else np.asarray(want)
    assert g.dtype == np.float32 and w.dtype == np.float32
    return np.array_equal(g.view(np.uint32), w.reshape(g.shape).view(np.uint32))


def bounded(got, want, bound, what):
    """form (3) with the bound given elementwise: |got - want| <= bound (a NaN in `got` fails); prints the margin"""
    got = got.detach().double()
    want = torch.as_tensor(want, dtype=torch.float64, device=got.device).reshape(got.shape)
    bound = torch.as_tensor(bound, dtype=torch.float64, device=got.device).expand(got.shape)
    err = (got - want).abs().nan_to_num(nan=float("inf"))
    used = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print("%s: largest error %.3e, largest share of the bound %.3f" % (what, float(err.max()) if err.numel() else 0.0, used))
    assert bool((err <= bound).all()), what
    return used


def within(got, want, sum_abs, n, what):
    """form (3): |got - want| <= (n + 2) * 2^-24 * sum|terms| elementwise"""
    sum_abs = torch.as_tensor(sum_abs, dtype=torch.float64, device=got.device)
    return bounded(got, want, (n + 2) * U * sum_abs, "%s (n = %d)" % (what, n))


def ints(shape, lo, hi, seed):
    """integer-valued fp32 in [lo, hi], drawn on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, device="cuda", generator=g).float()


# ---- the host-side dispatch of bn.hip, restated to name the branch a shape reaches (checked against spnet_bn_ws)
def chan_lanes(c4n):
    cl = 8
    while cl < c4n and cl < 64:
        cl <<= 1
    return cl


def bn_parts(M, C):
    if C == 3 and M % 4 == 0:                       # bn_partial_c3_kernel: 256 threads x 4 groups of 4 pixels each
        return max(1, min(1024, -(-(M // 4) // 1024)))
    if C % 4:                                       # bn_partial_small_kernel: (64*C)*8 elements per workgroup
        return max(1, min(256, -(-(M * C) // (64 * C * 8))))
    cl = chan_lanes(C // 4)
    by, gx = 256 // cl, -(-(C // 4) // cl)
    return max(1, min(-(-M // (by * 8)), max(1, min(256, 2048 // gx))))


def vec_chain(M, C):
    """longest fp32 chain of bn_partial_vec_kernel: the rows one thread adds up, then the fold of blockDim.y sums"""
    by = 256 // chan_lanes(C // 4)
    return -(-M // (bn_parts(M, C) * by)) + (by - 1)


def fuse_ok(P, M, C):
    return P <= 128 or (P <= 512 and M * C <= (4 << 20))


def act64(t, act):
    return B.act_fwd(t, act)


# ============================================================================================ exact-sum inputs
_CACHE = {}


def exact_case(M, C):
    """x, residual, dy (integer-valued) and the per-channel parameters of form (2), cached per shape and never modified"""
    if (M, C) not in _CACHE:
        if M * C > 1 << 20:
            _CACHE.clear()                          # one large case on the device at a time
        c = np.arange(C)
        d = dict(x=ints((M, C), -8, 8, 1000 + M + C), res=ints((M, C), -3, 3, 2000 + M + C), dy=ints((M, C), -4, 4, 3000 + M + C),
                 gamma=dev(2.0 ** (c % 3 - 1)), beta=dev((c % 5 - 2).astype(np.float64)),
                 mean=dev(((c // 2) % 3 - 1).astype(np.float64)), invstd=dev(2.0 ** ((c // 3) % 3 - 1)))
        # backward: |xhat| <= (8 + 1) * 2, |g * xhat| <= 72 in halves: 144 * M < 2^24; forward: 64 * M < 2^24
        assert 144 * M < 2 ** 24
        _CACHE[(M, C)] = d
    return _CACHE[(M, C)]


def expected_stats(x, gamma, beta, M=None):
    C = x.shape[1]
    xd = x.double()
    s, q = xd.sum(0).cpu().numpy(), (xd * xd).sum(0).cpu().numpy()          # exact: integers below 2^24
    return B.finalize_bits(s, q, M or x.shape[0], gamma.cpu().numpy(), beta.cpu().numpy(), EPS, MOM, np.full(C, MM0, np.float32),
                           np.full(C, MV0, np.float32))


class FwdOut:
    def __init__(self, C, M, ldy=None, ws=0):
        self.b = Bufs()
        self.C, self.ldy = C, ldy or C
        self.mm, self.mv = self.b.new((C,), torch.full((C,), MM0)), self.b.new((C,), torch.full((C,), MV0))
        self.save, self.ss = self.b.new((2 * C,)), self.b.new((2 * C,))
        self.y = self.b.new((M, self.ldy))
        self.ws = self.b.new((max(ws, 1),))

    def check_stats(self, exp):
        """forms (1) / (2): mean, invstd, scale, shift and both moving statistics equal finalize_bits bit for bit"""
        C = self.C
        mean, invstd, sc, sh, mm, mv = exp
        assert self.b.guards_untouched()
        assert bits_equal(self.save[:C], mean) and bits_equal(self.save[C:], invstd), "save_mean / save_invstd"
        assert bits_equal(self.ss[:C], sc) and bits_equal(self.ss[C:], sh), "scale_shift"
        assert bits_equal(self.mm, mm) and bits_equal(self.mv, mv), "moving statistics"

    def check_y(self, x, exp, act, res=None, bcast=False, what="y"):
        """form (3), n = 2: one fma and the residual add on the fp32 coefficients just pinned (0.1f * v is a third rounding)"""
        C = self.C
        sc, sh = torch.from_numpy(exp[2]).cuda().double(), torch.from_numpy(exp[3]).cuda().double()
        xd = x.double()
        want, sa = act64(xd * sc + sh, act), (xd * sc).abs() + sh.abs()
        if res is not None:
            r = res.double().reshape(-1, 1) if bcast else res.double()
            want, sa = want + r, sa + r.abs()
        within(self.y[:, :C], want, sa, 2 + (act == 2), what)
        assert bool(torch.isnan(self.y[:, C:]).all()), "columns between the blocks"


def _variant(M, C):
    """activation and residual form of a shape: every act and every residual form occurs in each family"""
    k = (M + C) % 12
    return k % 4, ("none", "full", "bcast" if C % 4 else "full")[k % 3]


SMALL = [(C, M) for C in (1, 2, 3) for M in (1, 2, 63, 1001, 20001)]              # bn_partial_small_kernel; 20001: several workgroups
C3 = [(3, 4), (3, 4100), (3, 4 * 256 * 4 * 3 + 4)]                                 # bn_partial_c3_kernel; the last: a ragged fourth workgroup
# bn_partial_vec_kernel: bn_chan_lanes 8 / 16 / 64, so blockDim.y = 32 / 16 / 4 (36 and 260 leave channel lanes idle); the
# last two M of each C: bn_parts = 255, one below BN_MAX_PARTS, and 257 cut to 256 (a ninth row for the first threads)
VEC = [(C, M) for C, by in ((4, 32), (36, 16), (260, 4)) for M in (1, 7, 64, 65, 1000, by * 8 * 255, by * 8 * 256 + 1)]
# C = 64 on both sides of M*C = 4 Mi with 256 partial rows: the backward runs fused below (bn_bwd_fused_vec_kernel) and as
# two launches above (bn_bwd_finalize_kernel<0> + bn_bwd_apply_vec_kernel)
BIG = [(64, 65000), (64, 66000)]


@pytest.mark.parametrize("C,M", SMALL + C3 + VEC + BIG)
def test_training_forward_and_backward_exact_sums(L, C, M):
    """spnet_bn_fwd_train (partial kernel by shape, bn_fwd_finalize_kernel, bn_apply_scalar_kernel for C % 4 != 0 -- with an
    activation and with res_bcast -- or bn_apply_vec_kernel) and spnet_bn_bwd (the same partial kernels in MODE 1, then
    bn_bwd_finalize_kernel<0> + bn_bwd_apply_scalar_kernel, or for C % 4 == 0 the fused / two-launch forms), out of place
    and with dx == dy."""
    d = exact_case(M, C)
    act, rform = _variant(M, C)
    parts = bn_parts(M, C)
    assert L.spnet_bn_ws(M, C) == parts * 2 * C
    if (C, M) == C3[2]:
        assert parts == 4
    if C % 4 == 0 and M > 1000 and C != 64:
        assert parts == (256 if M % 2 else 255)
    res = {"none": None, "full": d["res"], "bcast": d["res"][:, 0].contiguous()}[rform]
    o = FwdOut(C, M, ws=parts * 2 * C)
    L.spnet_bn_fwd_train(d["x"].data_ptr(), M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(),
                         o.save.data_ptr(), o.save[C:].data_ptr(), o.ss.data_ptr(), act, None if res is None else res.data_ptr(),
                         int(rform == "bcast"), o.y.data_ptr(), EPS, MOM, o.ws.data_ptr(), st())
    exp = expected_stats(d["x"], d["gamma"], d["beta"])
    o.check_stats(exp)                                              # (2)
    o.check_y(d["x"], exp, act, res, rform == "bcast")              # (3)
    # LeakyReLU's g = dy * 0.1f is rounded, so its sums are not exact: the backward of those shapes runs ReLU6 instead
    # (act 2 in the backward: test_activation_edges_backward, and test_kernels_gpu.py on random data)
    _backward_exact(L, d, M, C, 3 if act == 2 else act, parts)


def _backward_exact(L, d, M, C, act, parts):
    ref =B.backward_saved(d["x"], d["dy"], d["gamma"], d["beta"], d["mean"], d["invstd"], act)
    two_launch = bool(C % 4) or not fuse_ok(parts, M, C)
    if (C, M) in BIG:
        assert two_launch == (M == 66000)
    outs = []
    for inplace in (False, True):
        b = Bufs()
        dx = b.new((M, C), d["dy"] if inplace else None)
        dga, dbe, co, ws = b.new((C,)), b.new((C,)), b.new((3 * C,)), b.new((parts * 2 * C,))
        L.spnet_bn_bwd(d["x"].data_ptr(), dx.data_ptr() if inplace else d["dy"].data_ptr(), M, C, d["gamma"].data_ptr(),
                       d["beta"].data_ptr(), d["mean"].data_ptr(), d["invstd"].data_ptr(), act, dx.data_ptr(), dga.data_ptr(),
                       dbe.data_ptr(), co.data_ptr(), ws.data_ptr(), st())
        assert b.guards_untouched()
        assert bits_equal(dga, ref["dgamma"].float()) and bits_equal(dbe, ref["dbeta"].float())        # (2)
        assert torch.equal(dga.double(), ref["dgamma"]) and torch.equal(dbe.double(), ref["dbeta"])    # ... which is the exact sum
        if two_launch:                              # the coefficients are only materialised by the finalize kernel
            assert bits_equal(co, torch.cat([ref["k1"], ref["k2"], ref["k3"]]).float())                # (1) one cast each
        outs.append(dx)
    # (3) xhat and g are exact; k1, k2, k3 are cast from double (one rounding each), then two fma: the longest chain is 3
    sa = (ref["k1"] * ref["g"]).abs() + (ref["k2"] * ref["xhat"]).abs() + ref["k3"].abs()
    within(outs[0], ref["dx"], sa, 3, "dx")
    assert torch.equal(outs[0], outs[1])                            # (1) "dx may alias dy"


# ---------------------------------------------------------------------------- entries that take `partial`
def _partials(x, P, second=None):
    p = B.row_group_sums(x, P, second)
    assert float(p.abs().max()) < 2 ** 24
    return p.float().contiguous()                  # exact


# (M, C, P): bn_fuse_ok on both sides of each limit, bn_fuse_rows_per_slab at M = 1, 2, M < 64 and M no multiple of the
# slab, and the two-stage slicing from BN_SLICE_MIN_P (1087: 63 remainder rows beyond 64 * (P / 64) in the last slice)
FUSE = [(66000, 64, 128), (66000, 64, 129), (1000, 64, 512), (1000, 64, 513), (65000, 64, 200), (66000, 64, 200),
        (1, 4, 1), (2, 36, 2), (63, 260, 5), (1000, 36, 7), (65, 4, 128), (4097, 36, 3)]
SLICED = [(2174, 36, 1023), (2174, 36, 1024), (2174, 36, 1087), (300, 260, 1087)]


@pytest.mark.parametrize("M,C,P", FUSE + SLICED)
def test_finalize_and_apply_from_partial_rows(L, M, C, P):
    """spnet_bn_finalize_fwd (bn_fwd_finalize_kernel direct, or bn_slice_partials_kernel + combine_slices from P = 1024),
    spnet_bn_finalize_apply (bn_fwd_fused_vec_kernel while bn_fuse_ok, else the two launches) and its `_ld` form at
    ldy = C + 4 and 2C.  The partial rows are exact float64 sums of row groups of x."""
    d = exact_case(M, C)
    act, rform = _variant(M, P)
    res = None if rform == "none" else d["res"]
    part0 = _partials(d["x"], P)
    exp = expected_stats(d["x"], d["gamma"], d["beta"])
    for kind, ldy in (("finalize", C), ("apply", C), ("apply_ld", C + 4), ("apply_ld", 2 * C)):
        o = FwdOut(C, M if kind != "finalize" else 1, ldy=ldy if kind != "finalize" else 1)
        part = o.b.new((P, 2, C), part0)
        if kind == "finalize":
            L.spnet_bn_finalize_fwd(part.data_ptr(), P, M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(), o.mm.data_ptr(),
                                    o.mv.data_ptr(), o.save.data_ptr(), o.save[C:].data_ptr(), o.ss.data_ptr(), EPS, MOM, st())
        elif kind == "apply":
            L.spnet_bn_finalize_apply(part.data_ptr(), P, d["x"].data_ptr(), M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(),
                                      o.mm.data_ptr(), o.mv.data_ptr(), o.save.data_ptr(), o.save[C:].data_ptr(), o.ss.data_ptr(),
                                      act, None if res is None else res.data_ptr(), o.y.data_ptr(), EPS, MOM, st())
        else:
            L.spnet_bn_finalize_apply_ld(part.data_ptr(), P, d["x"].data_ptr(), M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(),
                                         o.mm.data_ptr(), o.mv.data_ptr(), o.save.data_ptr(), o.save[C:].data_ptr(), o.ss.data_ptr(),
                                         act, None if res is None else res.data_ptr(), o.y.data_ptr(), ldy, EPS, MOM, st())
        o.check_stats(exp)                                          # (2): hi + lo of an integer below 2^24 is that integer
        if kind != "finalize":
            o.check_y(d["x"], exp, act, res, what="%s ldy %d" % (kind, ldy))                           # (3)
        else:
            assert bool(torch.isnan(o.y).all())
        # the header: `partial` is consumed from P = 1024 on (slice sums left in its own rows); below it is only read
        assert torch.equal(part, part0) == (P < 1024), "partial consumed"


@pytest.mark.parametrize("M,C,P", FUSE)
def test_backward_from_partial_rows(L, M, C, P):
    """spnet_bn_bwd_from_partials: bn_bwd_fused_vec_kernel while bn_fuse_ok, else bn_bwd_finalize_kernel<0> +
    bn_bwd_apply_vec_kernel; g already carries the mask (act 3 here), the entry itself applies none.  Out of place and
    with dx == dy.  spnet_bn_bwd_coeffs_from_partials on the same rows."""
    d = exact_case(M, C)
    r3 = B.backward_saved(d["x"], d["dy"], d["gamma"], d["beta"], d["mean"], d["invstd"], 3)
    g = r3["g"].float().contiguous()
    assert 0 < float((g != d["dy"]).double().mean()) < 1 or M < 3
    ref = B.backward_saved(d["x"], g, d["gamma"], d["beta"], d["mean"], d["invstd"], 0)
    part = _partials(g, P, second=ref["xhat"])
    outs = []
    for inplace in (False, True):
        b = Bufs()
        dx = b.new((M, C), g if inplace else None)
        dga, dbe, co = b.new((C,)), b.new((C,)), b.new((3 * C,))
        pp = b.new((P, 2, C), part)
        L.spnet_bn_bwd_from_partials(d["x"].data_ptr(), dx.data_ptr() if inplace else g.data_ptr(), M, C, d["gamma"].data_ptr(),
                                     d["beta"].data_ptr(), d["mean"].data_ptr(), d["invstd"].data_ptr(), P, pp.data_ptr(),
                                     dx.data_ptr(), dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), st())
        assert b.guards_untouched() and torch.equal(pp, part)
        assert bits_equal(dga, ref["dgamma"].float()) and bits_equal(dbe, ref["dbeta"].float())        # (2)
        assert torch.equal(dga.double(), ref["dgamma"]) and torch.equal(dbe.double(), ref["dbeta"])
        outs.append(dx)
    sa = (ref["k1"] * ref["g"]).abs() + (ref["k2"] * ref["xhat"]).abs() + ref["k3"].abs()
    within(outs[0], ref["dx"], sa, 3, "dx")                         # (3) three casts, two fma: the longest chain is 3
    assert torch.equal(outs[0], outs[1])                            # (1) dx == dy
    _check_coeffs(L, d, M, C, g, ref, P, part)


def _check_coeffs(L, d, M, C, g, ref, P=None, part=None):
    """spnet_bn_bwd_coeffs (own reduction pass, P None) / spnet_bn_bwd_coeffs_from_partials: bn_bwd_finalize_kernel<1>.
    dgamma / dbeta (2); the coefficients by their identity dx = k1*g + k2'*x + k3' against the reference dx (3): evaluated
    in float64 on the kernel's fp32 coefficients, so n = 1 (the cast of each); and against bn_ref.bwd_coeffs (one cast)."""
    cld = C + 4
    b = Bufs()
    dga, dbe, coef = b.new((C,)), b.new((C,)), b.new((3, cld))
    if P is None:
        parts = bn_parts(M, C)
        ws = b.new((parts * 2 * C,))
        L.spnet_bn_bwd_coeffs(d["x"].data_ptr(), g.data_ptr(), M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(), d["mean"].data_ptr(),
                              d["invstd"].data_ptr(), dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), cld, ws.data_ptr(), st())
    else:
        L.spnet_bn_bwd_coeffs_from_partials(P, part.data_ptr(), M, C, d["gamma"].data_ptr(), d["mean"].data_ptr(),
                                            d["invstd"].data_ptr(), dga.data_ptr(), dbe.data_ptr(), coef.data_ptr(), cld, st())
    assert b.guards_untouched()
    assert bool(torch.isnan(coef[:, C:]).all())                     # the tail beyond C is the caller's
    assert bits_equal(dga, ref["dgamma"].float()) and bits_equal(dbe, ref["dbeta"].float())            # (2)
    k1, k2, k3 = (coef[i, :C].double() for i in range(3))
    xd = d["x"].double()
    sa = (k1 * ref["g"]).abs() + (k2 * xd).abs() + k3.abs()
    within((k1 * ref["g"] + k2 * xd + k3), ref["dx"], sa, 1, "dx from the blend coefficients")
    w1, w2, w3 = B.bwd_coeffs(ref["dbeta"], ref["dgamma"], M, d["gamma"], d["mean"], d["invstd"])
    for got, want, name in ((k1, w1, "k1"), (k2, w2, "k2'"), (k3, w3, "k3'")):
        # k3' = d - b*invstd*mean is a difference: its rounding errors scale with the operands, not the result
        sab = want.abs() if name != "k3'" else (ref["k3"].abs() + (w2 * d["mean"].double()).abs())
        within(got, want, sab, 4, name)             # (3) a handful of double roundings (negligible) and one cast


@pytest.mark.parametrize("C,M", [(4, 1), (4, 1000), (36, 65), (36, 16 * 8 * 256 + 1), (260, 1000), (64, 66000)])
def test_backward_coefficients_from_an_own_reduction(L, C, M):
    """spnet_bn_bwd_coeffs: bn_partial_vec_kernel<1> with act 0, then bn_bwd_finalize_kernel<1>."""
    d = exact_case(M, C)
    ref = B.backward_saved(d["x"], d["dy"], d["gamma"], d["beta"], d["mean"], d["invstd"], 0)
    _check_coeffs(L, d, M, C, d["dy"], ref)


@pytest.mark.parametrize("C,P", [(3, 1), (36, 17), (3, 300)])
def test_backward_coefficients_from_partials_at_any_channel_count(L, C, P):
    """spnet_bn_bwd_coeffs_from_partials has no C % 4 requirement: the finalize kernel's channel guard (c < C)."""
    M = 1001
    d = exact_case(M, C)
    ref = B.backward_saved(d["x"], d["dy"], d["gamma"], d["beta"], d["mean"], d["invstd"], 0)
    _check_coeffs(L, d, M, C, d["dy"], ref, P, _partials(d["dy"], P, second=ref["xhat"]))


@pytest.mark.parametrize("C,ldy", [(4, 8), (36, 40), (36, 72), (260, 264)])
def test_training_and_inference_forward_into_a_column_block(L, C, ldy):
    """spnet_bn_fwd_train_ld / spnet_bn_fwd_infer_ld at ldy = C + 4 and 2C (bn_apply_vec_kernel's strided store)."""
    M = 65
    d = exact_case(M, C)
    parts = bn_parts(M, C)
    o = FwdOut(C, M, ldy=ldy, ws=parts * 2 * C)
    L.spnet_bn_fwd_train_ld(d["x"].data_ptr(), M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(),
                            o.save.data_ptr(), o.save[C:].data_ptr(), o.ss.data_ptr(), 3, d["res"].data_ptr(), 0, o.y.data_ptr(), ldy,
                            EPS, MOM, o.ws.data_ptr(), st())
    exp = expected_stats(d["x"], d["gamma"], d["beta"])
    o.check_stats(exp)                                              # (2)
    o.check_y(d["x"], exp, 3, d["res"])                             # (3), and the gap columns stay NaN
    b = Bufs()
    y, ss = b.new((M, ldy)), b.new((2 * C,))
    mm, mv = dev(np.arange(C) % 5 - 2.0), dev(2.0 ** (np.arange(C) % 4))
    L.spnet_bn_fwd_infer_ld(d["x"].data_ptr(), M, C, d["gamma"].data_ptr(), d["beta"].data_ptr(), mm.data_ptr(), mv.data_ptr(),
                            ss.data_ptr(), 1, None, 0, y.data_ptr(), ldy, EPS, st())
    assert b.guards_untouched() and bool(torch.isnan(y[:, C:]).all())
    sc, sh = ss[:C].double(), ss[C:].double()
    within(y[:, :C], act64(d["x"].double() * sc + sh, 1), (d["x"].double() * sc).abs() + sh.abs(), 1, "y (inference)")   # (3) one fma


def test_depthwise_prologue_finalize_exact_sums(L):
    """spnet_dwconv3x3_tiled_fwd_bnfin, the per-channel outputs only: the header claims the bits of spnet_bn_finalize_fwd."""
    Bn, H, W, C, P = 2, 6, 8, 36, 7
    M = Bn * H * W
    d = exact_case(M, C)
    o = FwdOut(C, M)
    part = o.b.new((P, 2, C), _partials(d["x"], P))
    w = ints((3, 3, C), -2, 2, 5)
    L.spnet_dwconv3x3_tiled_fwd_bnfin(d["x"].data_ptr(), w.data_ptr(), o.y.data_ptr(), Bn, H, W, C, 1, part.data_ptr(), P, M,
                                      d["gamma"].data_ptr(), d["beta"].data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(), o.save.data_ptr(),
                                      o.save[C:].data_ptr(), o.ss.data_ptr(), EPS, MOM, st())
    o.check_stats(expected_stats(d["x"], d["gamma"], d["beta"]))    # (2)
    assert bool(torch.isfinite(o.y).all())


# ============================================================================================ 3. activation edges
TN, SUB = float(np.float32(2.0 ** -126)), float(np.float32(2.0 ** -149))         # smallest positive normal / subnormal
SIX_UP, SIX_DN = float(np.nextafter(np.float32(6), np.float32(np.inf))), float(np.nextafter(np.float32(6), np.float32(-np.inf)))
INF = float("inf")
SLOPE = float(np.float32(0.1))
EDGE_X = [0.0, -0.0, TN, -TN, SUB, -SUB, 6.0, SIX_UP, SIX_DN, INF, -INF]
# y = act(x) for each of EDGE_X, written out: the convention a reader can check
EDGE_Y = {
    0: [0.0, -0.0, TN, -TN, SUB, -SUB, 6.0, SIX_UP, SIX_DN, INF, -INF],
    1: [0.0, 0.0, TN, 0.0, SUB, 0.0, 6.0, SIX_UP, SIX_DN, INF, 0.0],
    2: [0.0, -0.0, TN, float(np.float32(-TN) * np.float32(0.1)), SUB, float(np.float32(-SUB) * np.float32(0.1)), 6.0, SIX_UP, SIX_DN, INF, -INF],
    3: [0.0, 0.0, TN, 0.0, SUB, 0.0, 6.0, 6.0, SIX_DN, 6.0, 0.0],
}
# act'(x): ReLU 0 at 0; ReLU6 0 at 0 and at 6; LeakyReLU the slope at 0 (TF's ReluGrad / Relu6Grad; torch's float64 relu /
# hardtanh autograd gives the same, tests/test_bn_ref_cpu.py)
EDGE_G = {
    0: [1.0] * 11,
    1: [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0],
    2: [SLOPE, SLOPE, 1.0, SLOPE, 1.0, SLOPE, 1.0, 1.0, 1.0, 1.0, SLOPE],
    3: [0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0],
}
NV = len(EDGE_X)


def _edge_tensor(C, idx):
    """[len(idx)][C]: row r, channel c holds EDGE_X[idx[(r + c) % len(idx)]] -- every channel (every lane of a quad) sees
    every value"""
    n = len(idx)
    sel = np.array(idx)[(np.arange(n)[:, None] + np.arange(C)[None, :]) % n]
    return sel, dev(np.array(EDGE_X, np.float32)[sel])


@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activation_edges_forward(L, C, act):
    """spnet_bn_apply with scale 1, shift 0 (bn_apply_vec_kernel at C = 8, bn_apply_scalar_kernel at C = 3): out_pre =
    fmaf(x, 1, 0) = x.  Form (1) against the table, subnormals included: the kernels do not flush them (observed: the
    comparison is on the bits, only the sign of a zero is left open, fmaf(-0, 1, +0) being +0)."""
    sel, x = _edge_tensor(C, list(range(NV)))
    ss = dev(np.concatenate([np.ones(C), np.zeros(C)]))
    b = Bufs()
    y = b.new((NV, C))
    L.spnet_bn_apply(x.data_ptr(), NV, C, ss.data_ptr(), act, None, 0, y.data_ptr(), st())
    assert b.guards_untouched()
    got, want = y.cpu().numpy(), np.array(EDGE_Y[act], np.float32)[sel]
    print("act %d, C %d: y of (SUB, -SUB, -TN) = %r" % (act, C, [float(got[sel == k][0]) for k in (4, 5, 3)]))
    assert not np.isnan(got).any()
    assert np.array_equal(got, want), (got, want)                   # (1) values (+0 == -0)
    nz = want != 0
    assert np.array_equal(np.signbit(got[nz]), np.signbit(want[nz]))


@pytest.mark.parametrize("C", [8, 3])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_activation_edges_backward(L, C, act):
    """spnet_bn_bwd with mean 0, invstd 1, gamma 1, beta 0: out_pre = fmaf((x - 0) * 1, 1, 0) = x.  C = 8:
    bn_partial_vec_kernel<1> + bn_bwd_fused_vec_kernel; C = 3: bn_partial_small_kernel<1> + bn_bwd_apply_scalar_kernel.
    The mask of the SUMS kernel is read from dbeta with dy one-hot in row k (dbeta[c] = act'(x[k][c]), a single term);
    the mask of the APPLY kernel from dx with dy = +1 in row k and -1 in a second row holding the same x: both sums cancel
    exactly, k2 = k3 = 0 and dx = +-act'(x) (finite x only: 0 * inf poisons a channel's dx).  Form (1) against the table."""
    zero, one = dev(np.zeros(C)), dev(np.ones(C))
    table = np.array(EDGE_G[act], np.float32)

    def run(x, dy):
        M = x.shape[0]
        b = Bufs()
        dx, dga, dbe, co, ws = b.new((M, C)), b.new((C,)), b.new((C,)), b.new((3 * C,)), b.new((bn_parts(M, C) * 2 * C,))
        L.spnet_bn_bwd(x.data_ptr(), dy.data_ptr(), M, C, one.data_ptr(), zero.data_ptr(), zero.data_ptr(), one.data_ptr(), act,
                       dx.data_ptr(), dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), ws.data_ptr(), st())
        assert b.guards_untouched()
        return dx.cpu().numpy(), dbe.cpu().numpy()

    sel, x = _edge_tensor(C, list(range(NV)))                       # all values, infinities included: dbeta only
    for k in range(NV):
        dy = torch.zeros(NV, C, device="cuda")
        dy[k] = 1.0
        _, dbe = run(x, dy)
        assert np.array_equal(dbe, table[sel[k]]), (k, dbe, table[sel[k]])                     # (1)
    fin = list(range(9))
    sel, x = _edge_tensor(C, fin)
    x2 = torch.cat([x, x])
    for k in range(9):
        dy = torch.zeros(18, C, device="cuda")
        dy[k], dy[k + 9] = 1.0, -1.0
        dx, dbe = run(x2, dy)
        want = np.zeros((18, C), np.float32)
        want[k], want[k + 9] = table[sel[k]], -table[sel[k]]
        assert np.array_equal(dx, want) and not dbe.any(), (k, dx, want)                       # (1)


@pytest.mark.parametrize("C,M", [(32, 20000), (3, 20001)])
@pytest.mark.parametrize("act", [1, 3])
def test_forward_and_backward_agree_on_the_side_of_a_boundary(L, C, M, act):
    """The forward decides with fmaf(x, scale, shift), the backward with fmaf((x - mean) * invstd, gamma, beta).  The
    forward's side is read from y of spnet_bn_fwd_train (y > 0, and y < 6 for ReLU6), the backward's from dx of
    spnet_bn_bwd with dy = +-1: (dx - k2*xhat - k3) / (k1*dy) is 0 or 1 to 1e-3.  Asserted: every element on which they
    disagree lies within 4 * 2^-24 * (|x*scale| + |shift|) of the boundary in float64 -- the two forms differ by
    roundings of that size and nothing else.  Printed: the count, next to the count the same two expressions give when
    each is evaluated in float64 and rounded once.  Measured on the MI355X: 0 disagreements in all four cases (640,000 and
    60,003 elements; at most one element lies inside the band at all): a property now documented, not a defect."""
    rs = np.random.RandomState(C + act)
    mu, sd = rs.randn(C) * 2, np.exp(rs.randn(C) * 0.5)
    x = dev(rs.randn(M, C) * sd + mu)
    gamma, beta = dev((rs.rand(C) + 0.5) * (3.5 if act == 3 else 1.0)), dev(rs.randn(C) * 0.3 + (1.5 if act == 3 else 0.0))
    g = torch.Generator(device="cuda").manual_seed(7)
    dy = torch.randint(0, 2, (M, C), device="cuda", generator=g).float() * 2 - 1
    parts = bn_parts(M, C)
    o = FwdOut(C, M, ws=parts * 2 * C)
    L.spnet_bn_fwd_train(x.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(), o.save.data_ptr(),
                         o.save[C:].data_ptr(), o.ss.data_ptr(), act, None, 0, o.y.data_ptr(), EPS, MOM, o.ws.data_ptr(), st())
    b = Bufs()
    dx, dga, dbe, co = b.new((M, C)), b.new((C,)), b.new((C,)), b.new((3 * C,))
    L.spnet_bn_bwd(x.data_ptr(), dy.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), o.save.data_ptr(), o.save[C:].data_ptr(), act,
                   dx.data_ptr(), dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), o.ws.data_ptr(), st())
    assert o.b.guards_untouched() and b.guards_untouched()
    mean, invstd, sc, sh = o.save[:C].double(), o.save[C:].double(), o.ss[:C].double(), o.ss[C:].double()
    xd, ga, be = x.double(), gamma.double(), beta.double()
    k1 = ga * invstd
    k2, k3 = -k1 * dga.double() / M, -k1 * dbe.double() / M
    xh = (xd - mean) * invstd
    mask = (dx.double() - k2 * xh - k3) / (k1 * dy.double())
    assert float((mask - mask.round()).abs().max()) < 1e-3 and bool(((mask.round() == 0) | (mask.round() == 1)).all())
    bwd_in = mask.round() == 1
    fwd_in = (o.y > 0) & ((o.y < 6) if act == 3 else True)
    differ = fwd_in != bwd_in
    pre = xd * sc + sh
    dist = pre.abs() if act == 1 else torch.minimum(pre.abs(), (pre - 6).abs())
    near = dist < 4 * U * ((xd * sc).abs() + sh.abs())

    def inside(t):
        return (t > 0) & ((t < 6) if act == 3 else True)
    f32 = pre.float()                                                                        # each form in float64, rounded once
    b32 = (((x - o.save[:C]) * o.save[C:]).double() * ga + be).float()
    print("act %d, C %d: %d of %d elements decided differently by the forward and the backward kernel (%d within the band; "
          "the two expressions rounded from float64: %d)" % (act, C, int(differ.sum()), M * C, int(near.sum()),
                                                             int((inside(f32) != inside(b32)).sum())))
    assert int((differ & ~near).sum()) == 0
    frac_in = float(fwd_in.double().mean())
    assert 0.2 < frac_in < 0.9                                      # both sides are populated


# ============================================================================================ 4. conditioning
def _conditioned(M, seed):
    """[M][32] fp32.  Channel patterns (mean, std), repeated with fresh draws: mean/std 0, 3, 30, 300; a nonzero constant;
    a zero constant; std 1e-4 around 0; std 1e3; one float4 whose neighbours differ by 1e6 in scale."""
    rs = np.random.RandomState(seed)
    pat = [(0.0, 1.0), (3.0, 1.0), (30.0, 1.0), (300.0, 1.0), (0.7, 0.0), (0.0, 0.0), (0.0, 1e-4), (0.0, 1e3),
           (0.0, 1e-3), (0.0, 1e3), (0.0, 1e-3), (0.0, 1e3),
           (0.0, 2.0), (-6.0, 2.0), (60.0, 2.0), (-600.0, 2.0), (-123.456, 0.0), (0.0, 0.0), (1.0, 1e-4), (5.0, 1e3),
           (1e-3, 1e-3), (0.0, 1e3), (0.0, 1e-3), (1e3, 1e3),
           (0.0, 0.5), (1.5, 0.5), (15.0, 0.5), (150.0, 0.5), (300.0, 1.0), (-300.0, 1.0), (30.0, 1.0), (-30.0, 1.0)]
    assert len(pat) == 32
    x = np.stack([(rs.randn(M) * s + m) for m, s in pat], 1).astype(np.float32)
    return pat, dev(x)


def _stat_bounds(x, n):
    """float64 two-pass statistics of the fp32 data and the bounds of a one-pass fp32 summation with chains of n:
    |dmean| <= (n + 2) U sum|x| / M, |dvar| <= (n + 2) U (sum x^2 + 2 |mean| sum|x|) / M, dinvstd = invstd^3 dvar / 2 plus
    the cast of invstd itself."""
    xd = x.double()
    M = x.shape[0]
    mean, var = B.batch_stats(xd)
    inv = torch.rsqrt(var + float(np.float32(EPS)))
    sabs, sq = xd.abs().sum(0), (xd * xd).sum(0)
    dmean = (n + 2) * U * sabs / M
    dvar = (n + 2) * U * (sq + 2 * mean.abs() * sabs) / M
    dinv = 0.5 * inv ** 3 * dvar + U * inv
    return mean, var, inv, dmean, dvar, dinv


def _report(pat, name, got, want, bound):
    err = (got.double() - want).abs()
    share = (err / bound.clamp_min(1e-300)).cpu().numpy()
    rel = (err / want.abs().clamp_min(1e-300)).cpu().numpy()
    for ratio in (30.0, 300.0):
        ch = [i for i, (m, s) in enumerate(pat) if s > 0 and abs(abs(m) / s - ratio) < 1e-9]
        print("%s, |mean|/std = %g: largest share of the bound %.3f, largest relative error %.3e" % (name, ratio, share[ch].max(), rel[ch].max()))


@pytest.mark.parametrize("M", [1000, 20000])
@pytest.mark.parametrize("route", ["fwd_train", "colstats"])
def test_conditioning_of_the_forward_statistics(L, M, route):
    """One-pass fp32 sums against the two-pass float64 statistics of the same fp32 data (form (3), propagated).
    fwd_train: bn_partial_vec_kernel<0> at C = 32 (8 channel lanes x 32 row lanes): a thread adds ceil(M / (parts * 32)) = 8
    rows, then 31 adds fold the workgroup: n = 39.  colstats: spnet_gemm_f32_colstats with an identity B (C == x bit for
    bit) on the 32 x 32 tile (tile 10, 2 x 2 waves): 4 rows per lane, 2 shuffles, 1 add across the two wave rows: n = 7;
    then spnet_bn_finalize_fwd.  Everything after the partial rows is double.
    Measured on the MI355X (the documented limit of the one-pass form, NOT a defect: every channel is inside its bound,
    the largest share used is 0.50, by y): relative error of the variance against the two-pass reference at
    |mean|/std = 30: 4.2e-5 (fwd_train, M 1000), 1.5e-5 (M 20000), 1.2e-5 / 2.9e-6 (colstats); at |mean|/std = 300:
    2.2e-2 / 3.5e-3 (fwd_train), 3.0e-3 / 5.2e-4 (colstats) -- two to three digits; invstd loses half of that
    (1.1e-2 at worst), shares of the bound 0.002 ... 0.035."""
    pat, x = _conditioned(M, M)
    C = 32
    rs = np.random.RandomState(1)
    gamma, beta = dev(rs.rand(C) + 0.5), dev(rs.randn(C) * 0.3)
    o = FwdOut(C, M, ws=bn_parts(M, C) * 2 * C)
    o.mv.zero_()                                    # moving_var' = fl((1 - momentum) * unbiased var): the variance is readable
    if route == "fwd_train":
        n = vec_chain(M, C)
        assert n == 39
        L.spnet_bn_fwd_train(x.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(), o.save.data_ptr(),
                             o.save[C:].data_ptr(), o.ss.data_ptr(), 0, None, 0, o.y.data_ptr(), EPS, MOM, o.ws.data_ptr(), st())
    else:
        n = 4 + 2 + 1
        rows_max = (M + 31) // 32
        part = o.b.new((rows_max, 2, C))
        c = o.b.new((M, C))
        eye = torch.eye(C, device="cuda")
        rows = ctypes.c_int(0)
        L.spnet_gemm_f32_colstats(x.data_ptr(), 0, C, eye.data_ptr(), 1, C, c.data_ptr(), C, M, C, C, 10, part.data_ptr(),
                                  ctypes.addressof(rows), st())
        assert rows.value == rows_max and torch.equal(c, x)         # (1) x * 1 + 0 * ...: the statistics are those of x
        L.spnet_bn_finalize_fwd(part.data_ptr(), rows.value, M, C, gamma.data_ptr(), beta.data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(),
                                o.save.data_ptr(), o.save[C:].data_ptr(), o.ss.data_ptr(), EPS, MOM, st())
    assert o.b.guards_untouched()
    mean, var, inv, dmean, dvar, dinv = _stat_bounds(x, n)
    name = "%s M %d" % (route, M)
    bounded(o.save[:C], mean, dmean, name + " mean")                # (3)
    bounded(o.save[C:], inv, dinv, name + " invstd")                # (3)
    one_m = float(np.float32(1) - np.float32(MOM))
    var_k = o.mv.double() / one_m * (M - 1) / M                     # two roundings away from the kernel's double variance
    assert bool((var_k >= 0).all())
    bounded(var_k, var, dvar + 3 * U * var, name + " var")          # (3)
    _report(pat, name + " var", var_k, var, dvar + 3 * U * var)
    _report(pat, name + " invstd", o.save[C:], inv, dinv)
    const = [i for i, (m, s) in enumerate(pat) if s == 0.0]
    assert bool(torch.isfinite(o.save).all() and torch.isfinite(o.ss).all() and torch.isfinite(o.mm).all() and torch.isfinite(o.mv).all())
    assert bool((var[const] == 0).all()) and bool((o.save[C:][const] <= float(np.float32(1 / np.sqrt(np.float64(np.float32(EPS)))))).all())
    if route == "fwd_train":
        # y = fmaf(x, scale, shift): the errors of scale = gamma*invstd and shift = beta - mean*scale, then its own two roundings
        ga, be, xd = gamma.double(), beta.double(), x.double()
        sc, sh = ga * inv, be - mean * ga * inv
        dsc = ga.abs() * dinv + U * sc.abs()
        dsh = dmean * (sc.abs() + dsc) + mean.abs() * dsc + 2 * U * (mean * sc).abs() + U * (be.abs() + (mean * sc).abs())
        assert bool(torch.isfinite(o.y).all())
        bounded(o.y, xd * sc + sh, xd.abs() * dsc + dsh + 2 * U * ((xd * sc).abs() + sh.abs() + xd.abs() * dsc + dsh), name + " y")   # (3)


@pytest.mark.parametrize("M", [1000, 20000])
def test_conditioning_of_the_backward(L, M):
    """spnet_bn_bwd (bn_partial_vec_kernel<1> + bn_bwd_fused_vec_kernel, act 0) on the ill-conditioned channels, saved
    statistics = the two-pass float64 ones rounded to fp32 (for a constant channel invstd = 1/sqrt(eps)).  Reference: the
    closed form in float64 on exactly those fp32 inputs.  xhat = (x - mean) * invstd carries two roundings, so the chain
    of sum g*xhat is n + 2 with n = 39 as in the forward; dx through its coefficients (form (3), propagated)."""
    pat, x = _conditioned(M, M + 1)
    C = 32
    rs = np.random.RandomState(2)
    gamma, beta = dev(rs.rand(C) + 0.5), dev(rs.randn(C) * 0.3)
    dy = dev(rs.randn(M, C))
    mean64, var64 = B.batch_stats(x)
    mean, invstd = mean64.float(), torch.rsqrt(var64 + float(np.float32(EPS))).float()
    n = vec_chain(M, C)
    b = Bufs()
    dx, dga, dbe, co, ws = b.new((M, C)), b.new((C,)), b.new((C,)), b.new((3 * C,)), b.new((bn_parts(M, C) * 2 * C,))
    L.spnet_bn_bwd(x.data_ptr(), dy.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), invstd.data_ptr(), 0,
                   dx.data_ptr(), dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), ws.data_ptr(), st())
    assert b.guards_untouched()
    r = B.backward_saved(x, dy, gamma, beta, mean, invstd, 0)
    a = B.backward_saved(x, dy, gamma, beta, mean, invstd, 0, absolute=True)
    within(dbe, r["dbeta"], a["dbeta"], n, "M %d dbeta" % M)                                  # (3)
    within(dga, r["dgamma"], a["dgamma"], n + 2, "M %d dgamma" % M)                           # (3)
    dsg, dsgx = (n + 2) * U * a["dbeta"], (n + 4) * U * a["dgamma"]
    k1, k2, k3, xh, g = r["k1"].abs(), r["k2"].abs(), r["k3"].abs(), r["xhat"].abs(), r["g"].abs()
    dk2, dk3 = k1 / M * dsgx + U * k2, k1 / M * dsg + U * k3
    bound = U * k1 * g + xh * dk2 + 2 * U * k2 * xh + dk3 + 2 * U * (k1 * g + (k2 + dk2) * xh * (1 + 2 * U) + k3 + dk3)
    assert bool(torch.isfinite(dx).all())
    bounded(dx, r["dx"], bound, "M %d dx" % M)                                                # (3)


# ============================================================================================ 5. small things
def test_refusals_write_nothing(L):
    """hipErrorInvalidValue, and every output still NaN: res_bcast with C = 4 (the header: C in {1, 2, 3}), C = 5, 6, 7, a
    row stride below C or no multiple of 4, cld < C, coef NULL, `_x3` entries with NULL or misaligned planes."""
    M = 16
    x = ints((M, 8), -2, 2, 1)
    b = Bufs()
    y, save, ss, dga, dbe, co, ws = b.new((M, 16)), b.new((16,)), b.new((16,)), b.new((8,)), b.new((8,)), b.new((3, 8)), b.new((4096,))
    mm, mv = b.new((8,)), b.new((8,))
    part = torch.ones(4, 2, 8, device="cuda")
    g = torch.ones(8, device="cuda")
    X, Y, G, S1, S2, SS, WS, ST = x.data_ptr(), y.data_ptr(), g.data_ptr(), save.data_ptr(), save[8:].data_ptr(), ss.data_ptr(), ws.data_ptr(), st()
    MMp, MVp = mm.data_ptr(), mv.data_ptr()
    calls = []
    for C, bc in ((4, 1), (5, 0), (6, 0), (7, 0), (5, 1)):
        calls += [lambda C=C, bc=bc: L.spnet_bn_fwd_train(X, M, C, G, G, MMp, MVp, S1, S2, SS, 1, X, bc, Y, EPS, MOM, WS, ST),
                  lambda C=C, bc=bc: L.spnet_bn_fwd_infer(X, M, C, G, G, G, G, SS, 1, X, bc, Y, EPS, ST),
                  lambda C=C, bc=bc: L.spnet_bn_apply(X, M, C, G, 1, X, bc, Y, ST)]
        if C != 4:
            calls += [lambda C=C: L.spnet_bn_bwd(X, X, M, C, G, G, G, G, 1, Y, dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), WS, ST)]
    for C, ldy in ((8, 4), (8, 10), (8, 7), (3, 4)):                # stride below C, no multiple of 4; a stride at C % 4 != 0
        calls += [lambda C=C, ldy=ldy: L.spnet_bn_fwd_train_ld(X, M, C, G, G, MMp, MVp, S1, S2, SS, 1, None, 0, Y, ldy, EPS, MOM, WS, ST),
                  lambda C=C, ldy=ldy: L.spnet_bn_fwd_infer_ld(X, M, C, G, G, G, G, SS, 1, None, 0, Y, ldy, EPS, ST),
                  lambda C=C, ldy=ldy: L.spnet_bn_finalize_apply_ld(part.data_ptr(), 4, X, M, C, G, G, MMp, MVp, S1, S2, SS, 1, None, Y, ldy,
                                                                    EPS, MOM, ST)]
    for cld, cp in ((7, co.data_ptr()), (4, co.data_ptr()), (8, None)):
        calls += [lambda cld=cld, cp=cp: L.spnet_bn_bwd_coeffs_from_partials(4, part.data_ptr(), M, 8, G, G, G, dga.data_ptr(), dbe.data_ptr(), cp, cld, ST),
                  lambda cld=cld, cp=cp: L.spnet_bn_bwd_coeffs(X, X, M, 8, G, G, G, G, dga.data_ptr(), dbe.data_ptr(), cp, cld, WS, ST)]
    calls += [lambda: L.spnet_bn_bwd_coeffs(X, X, M, 6, G, G, G, G, dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), 8, WS, ST)]
    planes = b.new((8192,))
    for pp in (None, planes.data_ptr() + 4):
        calls += [lambda pp=pp: L.spnet_bn_bwd_x3(X, X, M, 8, G, G, G, G, 0, pp, dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), WS, ST),
                  lambda pp=pp: L.spnet_bn_bwd_from_partials_x3(X, X, M, 8, G, G, G, G, 4, part.data_ptr(), pp, dga.data_ptr(), dbe.data_ptr(),
                                                                co.data_ptr(), ST)]
    calls += [lambda: L.spnet_bn_bwd_x3(X, X, 4, 3, G, G, G, G, 0, planes.data_ptr(), dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), WS, ST),
              lambda: L.spnet_bn_bwd_from_partials(X, X, 4, 3, G, G, G, G, 4, part.data_ptr(), Y, dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), ST),
              lambda: L.spnet_bn_finalize_apply(part.data_ptr(), 0, X, M, 8, G, G, MMp, MVp, S1, S2, SS, 1, None, Y, EPS, MOM, ST)]
    for i, call in enumerate(calls):
        with pytest.raises(L.HipError, match="hipError_t 1$"):      # hipErrorInvalidValue
            call()
    torch.cuda.synchronize()
    assert b.all_nan()
    # ... and res_bcast is accepted at C = 1, 2, 3 (bn_apply_scalar_kernel reads residual[i / C])
    for C in (1, 2, 3):
        d = exact_case(63, C)
        bb = Bufs()
        yy = bb.new((63, C))
        ssc = dev(np.concatenate([np.full(C, 2.0), np.full(C, -1.0)]))
        r = d["res"][:, 0].contiguous()
        L.spnet_bn_apply(d["x"].data_ptr(), 63, C, ssc.data_ptr(), 3, r.data_ptr(), 1, yy.data_ptr(), st())
        assert bb.guards_untouched()
        assert torch.equal(yy.double(), act64(d["x"].double() * 2 - 1, 3) + r.double().reshape(-1, 1))                  # (2) integers


@pytest.mark.parametrize("C", [1, 3, 36, 256, 300])
def test_inference_coefficients(L, C):
    """spnet_bn_infer_coeffs (bn_infer_coeffs_kernel; 300 channels: a second workgroup, 256: none to spare).  Form (3)
    against gamma * rsqrt(mv + eps): the add, rsqrtf (one ulp = two units), the product: n = 4; shift = beta - mm*scale
    adds a product and a difference (or one fma): n = 6.  Form (1): the scale_shift spnet_bn_fwd_infer leaves."""
    rs = np.random.RandomState(C)
    gamma, beta = dev(rs.rand(C) + 0.5), dev(rs.randn(C))
    mm, mv = dev(rs.randn(C) * 3), dev(np.exp(rs.randn(C) * 3))
    mv[0] = 0.0
    b = Bufs()
    ss, ss2, y = b.new((2 * C,)), b.new((2 * C,)), b.new((5, C))
    L.spnet_bn_infer_coeffs(C, gamma.data_ptr(), beta.data_ptr(), mm.data_ptr(), mv.data_ptr(), ss.data_ptr(), EPS, st())
    assert b.guards_untouched()
    sc = gamma.double() * torch.rsqrt(mv.double() + float(np.float32(EPS)))
    within(ss[:C], sc, sc.abs(), 4, "scale")
    within(ss[C:], beta.double() - mm.double() * sc, beta.double().abs() + (mm.double() * sc).abs(), 6, "shift")
    if C % 4 == 0 or C < 4:
        x = ints((5, C), -3, 3, C)
        L.spnet_bn_fwd_infer(x.data_ptr(), 5, C, gamma.data_ptr(), beta.data_ptr(), mm.data_ptr(), mv.data_ptr(), ss2.data_ptr(), 0,
                             None, 0, y.data_ptr(), EPS, st())
        assert b.guards_untouched() and torch.equal(ss, ss2)        # (1)


@pytest.mark.parametrize("M,C", [(3000, 32), (1001, 3), (4100, 3)])
def test_relu6_training_forward_and_backward(L, M, C):
    """act 3 through spnet_bn_fwd_train and spnet_bn_bwd on random data (vec, small and c3 partial kernels) against the
    float64 reference at the tolerances of test_batchnorm_train_and_backward.  gamma = 3.5, beta = 1.5 (+- 5 %): of a
    unit Gaussian, P(3.5 z + 1.5 < 0) = 0.33 and P(3.5 z + 1.5 > 6) = 0.10; both shares are asserted on the reference."""
    rs = np.random.RandomState(M + C)
    x = dev(rs.randn(M, C) * 1.5 + 0.3)
    gamma, beta = dev(3.5 * (1 + 0.05 * rs.randn(C))), dev(1.5 * (1 + 0.05 * rs.randn(C)))
    res, dy = dev(rs.randn(M, C)), dev(rs.randn(M, C))
    f = B.forward(x, gamma, beta, 3, residual=res)
    above, below = float((f["out_pre"] > 6).double().mean()), float((f["out_pre"] < 0).double().mean())
    print("share above 6: %.3f, below 0: %.3f" % (above, below))
    assert 0.07 < above < 0.13 and 0.28 < below < 0.39
    dx64, dg64, db64 = B.backward(x, dy, gamma, beta, 3)
    parts = bn_parts(M, C)
    o = FwdOut(C, M, ws=parts * 2 * C)
    L.spnet_bn_fwd_train(x.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), o.mm.data_ptr(), o.mv.data_ptr(), o.save.data_ptr(),
                         o.save[C:].data_ptr(), o.ss.data_ptr(), 3, res.data_ptr(), 0, o.y.data_ptr(), EPS, MOM, o.ws.data_ptr(), st())
    b = Bufs()
    dx, dga, dbe, co = b.new((M, C)), b.new((C,)), b.new((C,)), b.new((3 * C,))
    L.spnet_bn_bwd(x.data_ptr(), dy.data_ptr(), M, C, gamma.data_ptr(), beta.data_ptr(), o.save.data_ptr(), o.save[C:].data_ptr(), 3,
                   dx.data_ptr(), dga.data_ptr(), dbe.data_ptr(), co.data_ptr(), o.ws.data_ptr(), st())
    assert o.b.guards_untouched() and b.guards_untouched()

    def close(got, want, rtol, atol):
        np.testing.assert_allclose(got.detach().cpu().double().numpy(), want.cpu().numpy(), rtol=rtol, atol=atol)
    close(o.y, f["y"], 2e-5, 2e-5)
    close(dx, dx64, 1e-4, 2e-5)
    close(dga, dg64, 1e-4, 1e-4 * np.sqrt(M))
    close(dbe, db64, 1e-4, 1e-4 * np.sqrt(M))
