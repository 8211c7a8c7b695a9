"""The DenseNet121 glue (csrc/densenet.hip) entry by entry against tests/helpers/glue_ref.py, behind guards.

Integer operands (values in +-3, integer means, invstd from {0.5, 1, 2}, scales and gammas that are powers of two or small
integers; scale*x + shift lands on exactly 0 for a good share of the elements), so every sum is exact in fp32 whatever its
order: every partial row (row p = the pixels 64p .. 64p+63), G, the outputs and the gaps of the strided tensors are demanded
bit for bit.  spnet_dense_coeffs and spnet_dense_consumer_fin run on arbitrary fp32 values against the helper's
rounding-by-rounding restatement.  The one bound of this file is spnet_dense_producer_fin off its exact cases (M no power
of two), derived per element in glue_ref.producer_fin_bound.  Guards as in tests/test_irv2_glue_gpu.py.

Not covered: the grid cap of spnet_pad_nhwc (65536 workgroups: a tensor of 64 Mi floats), and NULL-tensor refusals -- no
shape of these entries is both accepted and empty, so a launch that went through a lost NULL check could not be kept in
bounds by sizing buffers."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.helpers import gemm_ref as G
from tests.helpers import glue_ref as R
from tests.test_dwconv_gpu import Dev, out, st, tag, work
from tests.test_irv2_glue_gpu import Block, outblock, run_refusals, seed_of


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


# ---- tables ------------------------------------------------------------------------------------------------------------------
SUM_C = (4, 252, 256, 260)                      # 1, 63, 64 and 65 quads: on both sides of one workgroup of 64
SUM_M = (1, 3, 4, 5, 63, 64, 65, 129)           # the four row lanes, one slab, one slab and a row, two slabs and a row
COEF_C = (1, 5, 256, 257)
APPLY_CASES = [(5, 4), (65, 36), (33, 260)]     # (M, C)
APPLY_CAP = (16400, 1024)                       # 16400 * 256 = 4,198,400 float4 items > 16384 * 256
FIN_P, FIN_C = (1, 31, 32, 33, 70), (1, 7, 8, 9)
PRODUCER_EXACT = [(4, 4, 12), (64, 8, 44), (1, 4, 8)]       # (M, c0, c1), M a power of two
PRODUCER_BOUND = [(3, 4, 12), (65, 8, 44)]
PAD_CASES = [(1, 3, 4, 4, 0, 0, 0, 0), (2, 3, 5, 12, 1, 2, 0, 3), (1, 2, 2, 4, 3, 4, 5, 3), (2, 1, 1, 12, 0, 1, 2, 0)]   # B H W C pt pb pl pr
CONV7_CASES = [(1, 1, 1), (2, 1, 2), (3, 2, 6), (1, 6, 7), (2, 7, 8), (1, 8, 13), (2, 13, 1), (1, 13, 13), (3, 7, 2), (1, 6, 6)]  # B H W
CONV7_WGRAD_SLABS = (1, 91, 91)                 # 46 x 46 = 2116 output pixels: two slabs of 1058, 1058 % 32 == 2
CONV7_FWD_CAP = (1, 725, 725)                   # 363 x 363 = 131,769 output pixels > 8192 * 16
CONV7_DGRAD_CAP = (1, 1449, 1449)               # 2,099,601 input pixels > 8192 * 256


@functools.lru_cache(maxsize=None)
def dense_case(M, c):
    """x with planted roots of the affine, the consumer's operands, G before the call"""
    seed = seed_of(M, c, 1)
    x, scale, shift = R.draw_affine(R.ints((M, c), seed), seed + 1)
    d = dict(x=x, scale=scale, shift=shift, dz=R.ints((M, c), seed + 2), G0=R.ints((M, c), seed + 3), gamma=R.draw_gamma(c, seed + 4))
    d["mean"], d["invstd"] = R.draw_stats(c, seed + 5)
    R.assert_exact_dense(x, scale, shift, d["dz"], d["mean"], d["invstd"], d["gamma"], d["G0"], calls=2)
    return d


def coef_operand(scale, shift, cld):
    """[scale | NaN | shift], cld floats each, zero from channel c on: the middle third is never read"""
    c = len(scale)
    coef = np.zeros(3 * cld, np.float32)
    coef[:c], coef[cld:2 * cld], coef[2 * cld:2 * cld + c] = scale, np.nan, shift
    return coef


def f32s(n, seed, lo=None):
    a = np.random.RandomState(seed).randn(n).astype(np.float32)
    return a if lo is None else np.abs(a) + np.float32(lo)


# ---- column sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", SUM_C)
def test_dense_colsums(L, C):
    found = []
    for M in SUM_M:
        x = dense_case(M, C)["x"]
        P = int(L.spnet_dense_rows(M))
        want = R.dense_colsums(x)
        assert want.shape == (P, 2, C)
        xb, part = Block(x, C + 8, 4), out(P * 2 * C)
        L.spnet_dense_colsums_ld(xb.ptr, C + 8, M, C, part.ptr, st())
        found += tag(part.check(want), "M %d" % M)
    assert found == []


# ---- per-consumer affine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", COEF_C)
@pytest.mark.parametrize("training", [1, 0])
def test_dense_coeffs(L, c, training):
    """arbitrary fp32 operands: scale, shift and the moving statistics bit for bit; the zero tail and the zero middle third of
    coef; mm / mv untouched from channel c on, and not modified at all in inference"""
    cld, n, seed = c + 7, c + 5, seed_of(c, training)
    gamma, beta, mean, bmean, mm = (f32s(n, seed + k) for k in range(5))
    invstd, bvar, mv = (f32s(n, seed + 5 + k, 0.25) for k in range(3))
    eps, momentum = 1.001e-5, 0.99
    coef_ref, mm_ref, mv_ref = R.dense_coeffs(c, cld, gamma, beta, mean, invstd, bmean, bvar, mm, mv, eps, momentum, training)
    assert training or (np.array_equal(mm_ref, mm) and np.array_equal(mv_ref, mv))
    dev = [Dev(a) for a in (gamma, beta, mean, invstd, bmean, bvar)]
    mmd, mvd, coef = Dev(mm, R.SENTINEL), Dev(mv, R.SENTINEL), out(3 * cld)
    L.spnet_dense_coeffs(c, cld, *(t.ptr for t in dev), mmd.ptr, mvd.ptr, coef.ptr, eps, momentum, training, st())
    found = tag(coef.check(coef_ref), "coef") + tag(mmd.check(mm_ref), "moving mean") + tag(mvd.check(mv_ref), "moving variance")
    if not training:                                        # the batch statistics may be NULL
        coef = out(3 * cld)
        L.spnet_dense_coeffs(c, cld, dev[0].ptr, dev[1].ptr, None, None, None, None, mmd.ptr, mvd.ptr, coef.ptr, eps, momentum, 0, st())
        found += tag(coef.check(coef_ref), "coef without batch statistics")
    assert found == []


# ---- apply -----------------------------------------------------------------------------------------------------------------------
def apply_findings(L, M, C, relus=(0, 1)):
    seed = seed_of(M, C, 2)
    x, scale, shift = R.draw_affine(R.ints((M, C), seed), seed + 1)
    R.assert_exact_dense(x, scale, shift)
    cld = C + 4
    xb, cd = Block(x, C + 8, 4), Dev(coef_operand(scale, shift, cld))
    found = []
    for relu in relus:
        y = outblock(M, C, C + 12, 8)
        L.spnet_dense_apply_ld(xb.ptr, C + 8, M, C, cd.ptr, cld, relu, y.ptr, C + 12, st())
        found += tag(y.check(R.dense_apply(x, scale, shift, relu)), "relu %d" % relu)
    return found


@pytest.mark.parametrize("M,C", APPLY_CASES)
def test_dense_apply(L, M, C):
    assert apply_findings(L, M, C) == []


def test_dense_apply_past_the_grid_cap(L):
    M, C = APPLY_CAP
    assert M * (C // 4) > R.APPLY_CAP_ITEMS
    assert apply_findings(L, M, C, relus=(1,)) == []


# ---- consumer backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SUM_C)
def test_dense_consumer_bwd(L, c):
    """called twice on the same G: G0 + 2*gamma*g shows `+=`; the partial rows are those of one call"""
    found = []
    cld = c + 4
    for M in SUM_M:
        d = dense_case(M, c)
        P = int(L.spnet_dense_rows(M))
        zb, xb, cd = Block(d["dz"], c + 8, 4), Block(d["x"], c + 12, 8), Dev(coef_operand(d["scale"], d["shift"], cld))
        mud, isd, gad = Dev(d["mean"]), Dev(d["invstd"]), Dev(d["gamma"])
        for relu in (0, 1):
            g, G1, part_ref = R.dense_consumer_bwd(d["dz"], d["x"], d["scale"], d["shift"], d["mean"], d["invstd"], d["gamma"], relu, d["G0"])
            _, G2, _ = R.dense_consumer_bwd(d["dz"], d["x"], d["scale"], d["shift"], d["mean"], d["invstd"], d["gamma"], relu, G1)
            Gb, part = Block(d["G0"], c + 16, 4, poison=R.SENTINEL), out(P * 2 * c)
            name = "M %d relu %d " % (M, relu)
            for k, want in enumerate((G1, G2)):
                L.spnet_dense_consumer_bwd(zb.ptr, c + 8, xb.ptr, c + 12, M, c, cd.ptr, cld, mud.ptr, isd.ptr, gad.ptr, relu, Gb.ptr, c + 16, part.ptr, st())
                found += tag(Gb.check(want), name + "G after call %d" % (k + 1)) + tag(part.check(part_ref), name + "partial after call %d" % (k + 1))
    assert found == []


@pytest.mark.parametrize("c", FIN_C)
def test_dense_consumer_fin(L, c):
    """integer partial rows (their double sum is exact in any order), arbitrary fp32 gamma, u and v: dbeta, dgamma and the two
    fmaf bit for bit"""
    found = []
    for P in FIN_P:
        seed = seed_of(P, c, 3)
        part = G.int_operands((P, 2, c), -50, 50, seed)
        gamma, u0, v0 = f32s(c, seed + 1), f32s(c, seed + 2), f32s(c, seed + 3)
        dgamma, dbeta, u, v = R.dense_consumer_fin(part, gamma, u0, v0)
        pd, gd = Dev(part), Dev(gamma)
        dgd, dbd, ud, vd = out(c), out(c), Dev(u0, R.SENTINEL), Dev(v0, R.SENTINEL)
        L.spnet_dense_consumer_fin(pd.ptr, P, c, gd.ptr, dgd.ptr, dbd.ptr, ud.ptr, vd.ptr, st())
        name = "P %d " % P
        found += tag(dgd.check(dgamma), name + "dgamma") + tag(dbd.check(dbeta), name + "dbeta") + tag(ud.check(u), name + "u") + tag(vd.check(v), name + "v")
    assert found == []


# ---- producer finalize -------------------------------------------------------------------------------------------------------------
def producer_case(M, c0, c1):
    """G, x [M][c1], u, v, mean, invstd [c1]: integers (invstd from {0.5, 1, 2}); NaN in the channels below c0, which the
    call must not read"""
    seed = seed_of(M, c0, c1)
    d = dict(G=R.ints((M, c1), seed), x=R.ints((M, c1), seed + 1), u=R.ints((c1,), seed + 2, 9), v=R.ints((c1,), seed + 3, 9))
    d["mean"], d["invstd"] = R.draw_stats(c1, seed + 4)
    ref = {k: a[..., c0:] for k, a in d.items()}
    for a in d.values():
        a[..., :c0] = np.nan
    return d, ref


def producer_run(L, d, M, c0, c1):
    n = c1 - c0
    Gb, xb = Block(d["G"], c1 + 8, 4), Block(d["x"], c1 + 12, 8)
    ud, vd, mud, isd = Dev(d["u"]), Dev(d["v"]), Dev(d["mean"]), Dev(d["invstd"])
    o = outblock(M, n, n + 8, 4)
    L.spnet_dense_producer_fin(Gb.ptr, c1 + 8, ud.ptr, vd.ptr, xb.ptr, c1 + 12, mud.ptr, isd.ptr, M, c0, c1, o.ptr, n + 8, st())
    return o


@pytest.mark.parametrize("M,c0,c1", PRODUCER_EXACT)
def test_dense_producer_fin_exact(L, M, c0, c1):
    d, r = producer_case(M, c0, c1)
    R.assert_exact_producer_fin(r["G"], r["u"], r["v"], r["x"], r["mean"], r["invstd"], M)
    o = producer_run(L, d, M, c0, c1)
    assert o.check(R.dense_producer_fin(r["G"], r["u"], r["v"], r["x"], r["mean"], r["invstd"], M)) == []


@pytest.mark.parametrize("M,c0,c1", PRODUCER_BOUND)
def test_dense_producer_fin_within_its_derived_bound(L, M, c0, c1):
    """M = 3 and 65 (1/M is not an fp32): |got - ref| <= 8 * 2^-24 * invstd * (|G| + |u|/M + |xhat|*|v|/M) per element
    (glue_ref.producer_fin_bound: six fp32 roundings, contracted or not); the gaps of the strided output untouched"""
    d, r = producer_case(M, c0, c1)
    n = c1 - c0
    o = producer_run(L, d, M, c0, c1)
    args = (r["G"], r["u"], r["v"], r["x"], r["mean"], r["invstd"], M)
    want, bound = R.dense_producer_fin(*args), R.producer_fin_bound(*args)
    buf = o.t.cpu().numpy()
    got = buf[1:1 + M, 4:4 + n].astype(np.float64)
    err = np.abs(got - want)
    print("producer_fin M %d: largest error / bound %.3f" % (M, float(np.max(err / np.maximum(bound, 1e-300)))))
    beyond = np.argwhere(~(err <= bound))
    assert beyond.tolist() == []
    buf[1:1 + M, 4:4 + n] = R.SENTINEL
    assert bool((buf == np.float32(R.SENTINEL)).all())


# ---- zero padding ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C,pt,pb,pl,pr", PAD_CASES)
def test_pad_nhwc(L, B, H, W, C, pt, pb, pl, pr):
    """forward on a ramp of distinct integers, and the backward crop of a padded ramp.  (The grid cap of this entry, 65536
    workgroups of 256 float4, needs a tensor of 64 Mi floats: left out.)"""
    x = R.ramp((B, H, W, C))
    want = R.pad_nhwc(x, pt, pb, pl, pr)
    xd, y = Dev(x), out(want.size)
    L.spnet_pad_nhwc(xd.ptr, y.ptr, B, H, W, C, pt, pb, pl, pr, 0, st())
    found = tag(y.check(want), "forward")
    g = R.ramp(want.shape)
    gd, dx = Dev(g), out(x.size)
    L.spnet_pad_nhwc(gd.ptr, dx.ptr, B, H, W, C, pt, pb, pl, pr, 1, st())
    found += tag(dx.check(R.pad_nhwc(g, pt, pb, pl, pr, backward=True)), "backward")
    assert found == []


# ---- conv1/conv ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv7_case(B, H, W):
    seed = seed_of(B, H, W, 7)
    x, w = R.ints((B, H, W, 3), seed), R.ints((7, 7, 3, R.CONV7_CO), seed + 1)
    dy = R.ints((B, R.conv7_out(H), R.conv7_out(W), R.CONV7_CO), seed + 2)
    R.assert_exact_conv7(x, w, dy)
    return x, w, dy


def conv7_findings(L, B, H, W, ops=(0, 1, 2)):
    x, w, dy = conv7_case(B, H, W)
    xd, wd, dyd = Dev(x), Dev(w), Dev(dy)
    found = []
    if 0 in ops:
        y = out(dy.size)
        L.spnet_dense_conv7(0, xd.ptr, wd.ptr, y.ptr, B, H, W, None, 0, st())
        found += tag(y.check(R.conv7_fwd(x, w)), "forward")
    if 1 in ops:
        dx = out(x.size)
        L.spnet_dense_conv7(1, dyd.ptr, wd.ptr, dx.ptr, B, H, W, None, 0, st())
        found += tag(dx.check(R.conv7_dgrad(dy, w, H, W)), "data gradient")
    if 2 in ops:
        n = int(L.spnet_dense_conv7_ws(B, H, W))
        ws, dw = work(n), out(w.size)
        L.spnet_dense_conv7(2, xd.ptr, dyd.ptr, dw.ptr, B, H, W, ws.ptr, n, st())
        found += tag(dw.check(R.conv7_wgrad(x, dy)), "weight gradient") + tag(ws.guards(), "workspace")
    return found


@pytest.mark.parametrize("B,H,W", CONV7_CASES)
def test_dense_conv7(L, B, H, W):
    assert conv7_findings(L, B, H, W) == []


def test_dense_conv7_weight_gradient_over_two_slabs(L):
    B, H, W = CONV7_WGRAD_SLABS
    assert int(L.spnet_dense_conv7_ws(B, H, W)) == 2 * R.CONV7_K * R.CONV7_CO
    assert conv7_findings(L, B, H, W, ops=(2,)) == []


def conv7_fwd_cap_points(H, W):
    """x is zero except where it feeds the first output pixel, the last one and both sides of the wrap of the pixel loop
    (output pixels 8192*16 - 1 and 8192*16), through the centre tap: (b, h, w, ci, value)"""
    OW = R.conv7_out(W)
    a, b = R.CONV7_FWD_CAP_PIXELS - 1, R.CONV7_FWD_CAP_PIXELS
    return [(0, 0, 0, 0, 1), (0, H - 1, W - 1, 2, 3), (0, 2 * (a // OW), 2 * (a % OW), 1, 2), (0, 2 * (b // OW), 2 * (b % OW), 0, -2)]


def conv7_dgrad_cap_points(H, W):
    """dy is zero except at the windows over the first input pixel, the last one and both sides of the wrap (input pixels
    8192*256 - 1 and 8192*256): (b, oh, ow, co, value)"""
    a, b = R.CONV7_DGRAD_CAP_PIXELS - 1, R.CONV7_DGRAD_CAP_PIXELS
    assert a // W == b // W and (a % W) // 2 == (b % W) // 2
    return [(0, 0, 0, 0, 1), (0, R.conv7_out(H) - 1, R.conv7_out(W) - 1, 63, 3), (0, (a // W) // 2, (a % W) // 2, 5, -2)]


def test_dense_conv7_forward_past_the_grid_cap(L):
    B, H, W = CONV7_FWD_CAP
    w = G.nonzero_operands((7, 7, 3, R.CONV7_CO), 3, 11)
    pts = conv7_fwd_cap_points(H, W)
    x = np.zeros((B, H, W, 3))
    for b, h, ww, ci, v in pts:
        x[b, h, ww, ci] = v
    R.assert_exact_conv7(bound=16 * 3 * 3 * len(pts))
    want = R.conv7_fwd_scatter(pts, w, B, H, W)
    flat = want.reshape(-1, R.CONV7_CO)
    assert flat.shape[0] > R.CONV7_FWD_CAP_PIXELS and all(flat[p].any() for p in (0, R.CONV7_FWD_CAP_PIXELS - 1, R.CONV7_FWD_CAP_PIXELS, flat.shape[0] - 1))
    xd, wd, y = Dev(x), Dev(w), out(want.size)
    L.spnet_dense_conv7(0, xd.ptr, wd.ptr, y.ptr, B, H, W, None, 0, st())
    assert y.check(want) == []


def test_dense_conv7_data_gradient_past_the_grid_cap(L):
    B, H, W = CONV7_DGRAD_CAP
    w = G.nonzero_operands((7, 7, 3, R.CONV7_CO), 3, 12)
    pts = conv7_dgrad_cap_points(H, W)
    dy = np.zeros((B, R.conv7_out(H), R.conv7_out(W), R.CONV7_CO), np.float32)
    for b, oh, ow, co, v in pts:
        dy[b, oh, ow, co] = v
    R.assert_exact_conv7(bound=3 * 3 * len(pts))
    want = R.conv7_dgrad_scatter(pts, w, B, H, W)
    flat = want.reshape(-1, 3)
    assert flat.shape[0] > R.CONV7_DGRAD_CAP_PIXELS and all(flat[p].any() for p in (0, R.CONV7_DGRAD_CAP_PIXELS - 1, R.CONV7_DGRAD_CAP_PIXELS, flat.shape[0] - 1))
    dyd, wd, dx = Dev(dy), Dev(w), out(want.size)
    L.spnet_dense_conv7(1, dyd.ptr, wd.ptr, dx.ptr, B, H, W, None, 0, st())
    assert dx.check(want) == []


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def dense_refusal_table(L, z, o, o2):
    """the extent, alignment and stride refusals each entry states in densenet.hip, on shapes of at most 5 rows x 16 floats:
    z (16384 zeros), o (16384 sentinels) and o2 (8192) hold whatever such a launch would read and write if it went through"""
    s = st()
    pad = lambda B=1, H=2, W=2, C=4, pt=1, pb=1, pl=1, pr=1: L.spnet_pad_nhwc(z.ptr, o.ptr, B, H, W, C, pt, pb, pl, pr, 0, s)
    conv = lambda op=0, B=1, H=2, W=2, ws=z.ptr, n=16384: L.spnet_dense_conv7(op, z.ptr, z.ptr, o.ptr, B, H, W, ws, n, s)
    sums = lambda ldx=8, M=5, C=8: L.spnet_dense_colsums_ld(z.ptr, ldx, M, C, o.ptr, s)
    coef = lambda c=4, cld=8: L.spnet_dense_coeffs(c, cld, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, z.ptr, o2.ptr, o2.ptr + 256, o.ptr, 1e-3, 0.99, 1, s)
    app = lambda ldx=8, M=5, C=8, cld=8, ldy=8: L.spnet_dense_apply_ld(z.ptr, ldx, M, C, z.ptr, cld, 1, o.ptr, ldy, s)
    cb = lambda ldz=8, ldx=8, M=5, c=8, cld=8, ldg=8: L.spnet_dense_consumer_bwd(z.ptr, ldz, z.ptr, ldx, M, c, z.ptr, cld, z.ptr, z.ptr, z.ptr, 1, o.ptr, ldg, o2.ptr, s)
    fin = lambda P=2, c=4: L.spnet_dense_consumer_fin(z.ptr, P, c, z.ptr, o.ptr, o.ptr + 256, o2.ptr, o2.ptr + 256, s)
    pf = lambda ldg=16, ldx=16, M=5, c0=4, c1=12, ldo=8: L.spnet_dense_producer_fin(z.ptr, ldg, z.ptr, z.ptr, z.ptr, ldx, z.ptr, z.ptr, M, c0, c1, o.ptr, ldo, s)
    return [("pad, B 0", lambda: pad(B=0)), ("pad, H 0", lambda: pad(H=0)), ("pad, W 0", lambda: pad(W=0)), ("pad, C 0", lambda: pad(C=0)),
            ("pad, C % 4", lambda: pad(C=6)), ("pad, pt < 0", lambda: pad(pt=-1)), ("pad, pb < 0", lambda: pad(pb=-1)),
            ("pad, pl < 0", lambda: pad(pl=-1)), ("pad, pr < 0", lambda: pad(pr=-1)),
            ("conv7, op 3", lambda: conv(op=3)), ("conv7, op -1", lambda: conv(op=-1)), ("conv7, B 0", lambda: conv(B=0)),
            ("conv7, H 0", lambda: conv(H=0)), ("conv7, W 0", lambda: conv(W=0)),
            ("conv7, workspace one float short", lambda: conv(op=2, n=R.conv7_ws(1, 2, 2) - 1)),
            ("colsums, M 0", lambda: sums(M=0)), ("colsums, C 0", lambda: sums(C=0)), ("colsums, C % 4", lambda: sums(C=6)),
            ("colsums, ldx % 4", lambda: sums(ldx=10)), ("colsums, ldx < C", lambda: sums(ldx=4)),
            ("coeffs, c 0", lambda: coef(c=0)), ("coeffs, cld < c", lambda: coef(c=8, cld=4)),
            ("apply, M 0", lambda: app(M=0)), ("apply, C 0", lambda: app(C=0)), ("apply, C % 4", lambda: app(C=6)),
            ("apply, ldx % 4", lambda: app(ldx=10)), ("apply, ldy % 4", lambda: app(ldy=10)), ("apply, cld % 4", lambda: app(cld=10)),
            ("apply, cld < C", lambda: app(cld=4)), ("apply, ldx < C", lambda: app(ldx=4)), ("apply, ldy < C", lambda: app(ldy=4)),
            ("consumer_bwd, M 0", lambda: cb(M=0)), ("consumer_bwd, c 0", lambda: cb(c=0)), ("consumer_bwd, c % 4", lambda: cb(c=6)),
            ("consumer_bwd, cld < c", lambda: cb(cld=4)), ("consumer_bwd, cld % 4", lambda: cb(cld=10)),
            ("consumer_bwd, ldz % 4", lambda: cb(ldz=10)), ("consumer_bwd, ldx % 4", lambda: cb(ldx=10)), ("consumer_bwd, ldg % 4", lambda: cb(ldg=10)),
            ("consumer_bwd, ldz < c", lambda: cb(ldz=4)), ("consumer_bwd, ldx < c", lambda: cb(ldx=4)), ("consumer_bwd, ldg < c", lambda: cb(ldg=4)),
            ("consumer_fin, P 0", lambda: fin(P=0)), ("consumer_fin, c 0", lambda: fin(c=0)),
            ("producer_fin, M 0", lambda: pf(M=0)), ("producer_fin, c0 < 0", lambda: pf(c0=-4)), ("producer_fin, no channels", lambda: pf(c0=12)),
            ("producer_fin, n % 4", lambda: pf(c1=10)), ("producer_fin, c0 % 4", lambda: pf(c0=2, c1=10)),
            ("producer_fin, ldg % 4", lambda: pf(ldg=18)), ("producer_fin, ldx % 4", lambda: pf(ldx=18)), ("producer_fin, ldo % 4", lambda: pf(ldo=10)),
            ("producer_fin, ldg < c1", lambda: pf(ldg=8)), ("producer_fin, ldx < c1", lambda: pf(ldx=8)), ("producer_fin, ldo < n", lambda: pf(ldo=4))]


def test_dense_refusals_launch_nothing(L):
    z, o, o2 = Dev(np.zeros(16384, np.float32)), out(16384), out(8192)          # (o: the 147 x 64 weight gradient fits)
    assert run_refusals(L, dense_refusal_table(L, z, o, o2), (o, o2)) == []
