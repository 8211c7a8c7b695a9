"""TEST INFRASTRUCTURE -- the fused Adam + l2 step (csrc/optim.hip) restated in float64 on inputs for which EVERY intermediate
is a small dyadic number, so that the kernel must return these values bit for bit whatever the compiler contracts.

Arbitrary floats cannot be demanded exactly (a*b + c may or may not become one fma).  The table therefore fixes

    beta1 = 0.5, beta2 = 0.75, eps = 1, l2 = 0.25, grad_scale = 0.5, lr_t = 0.25 (argument) or 0.125 (device memory)

and draws, per element, integers p (non-zero, |p| <= 7), m (|m| <= 8), a root r in {1, 3, 7} and an effective gradient gj
with gj^2 <= 4 r^2 and gj^2 = r^2 (mod 3).  From these

    g = 2 gj - p [element in the l2 prefix]      so that g * grad_scale + 2 l2 p = gj,
    v = (4 r^2 - gj^2) / 3                       an integer >= 0, so that beta2 v + (1 - beta2) gj^2 = r^2,

and sqrt(v') + eps = r + 1 is 2, 4 or 8: the quotient is exact, and eps moved inside the root gives sqrt(2), sqrt(10) or
sqrt(50) instead.  adam(..., check=True) asserts after every product and every sum that the value is an fp32 number, which
is the whole proof: an exact product plus an exact sum is the same with and without contraction.  The sums of squares are
integers below 2^24 per workgroup (asserted), so any order of the fp32 additions gives them; the total is an integer far
below 2^53, exact in sum_partials_kernel's double accumulation, and l2 * total is rounded to fp32 once.

Workgroup b of a launch over n elements with G = parts(n) workgroups sums the float4 items b * 256 + t + k * 256 * G
(t < 256, k = 0, 1, ..): partials() restates that assignment.

DEFECTS names one-line variants of adam(); tests/test_optim_ref_cpu.py shows that the table notices each.  Arbitrary-float
Adam (rounding behaviour, many steps) stays with the tolerance tests of tests/test_kernels_gpu.py."""
import functools

import numpy as np

BETA1, BETA2, EPS, L2, GRAD_SCALE = 0.5, 0.75, 1.0, 0.25, 0.5
LR_ARG, LR_DEV = 0.25, 0.125
ADAM_BLOCKS = 2048
SIZES = (4, 8, 1020, 1024, 1028, 2048 * 1024, 2048 * 1024 + 4 * 257)
SMALL = tuple(n for n in SIZES if n <= 1028)
MASKS = ("none", "ones", "zeros", "checkered")
L2_SUM_COUNTS = (1, 255, 256, 257, 4096)
L2_SUM_MAX = 32768
DEFECTS = ("l2 boundary off by one", "l2 boundary rounded to the float4", "eps inside the root", "grad_scale after the penalty",
           "penalty l2 * p", "sq after the update", "sq skips frozen elements", "mask does not restore m",
           "mask does not restore v", "beta1 and beta2 swapped", "lr_dev ignored")

_GJ = {1: np.array([-2, -1, 1, 2]), 3: np.array([-6, -3, 0, 3, 6]),
       7: np.array([s * k for k in (1, 2, 4, 5, 7, 8, 10, 11, 13, 14) for s in (-1, 1)])}


def parts(n):
    """spnet_adam_parts"""
    return 0 if n < 4 else min(ADAM_BLOCKS, max(1, (n // 4 + 255) // 256))


def l2_prefixes(n):
    return sorted({0, 1, 2, 3, 5, n - 1, n, n + 7})


def cases():
    """(n, l2_n, mask, lr_from_device).  The small sizes take every combination; the two sizes of 2048 and more workgroups
    take every l2 prefix once, with the mask and the source of the step size changing from row to row."""
    t = [(n, l2n, mk, dev) for n in SMALL for l2n in l2_prefixes(n) for mk in MASKS for dev in (False, True)]
    for n in SIZES[len(SMALL):]:
        t += [(n, l2n, MASKS[k % 4], bool((k // 2) % 2)) for k, l2n in enumerate(l2_prefixes(n))]
    return t


@functools.lru_cache(maxsize=2)
def _draw(n):
    rs = np.random.RandomState(1000 + n % 9973)
    p = rs.randint(1, 8, n) * rs.choice((-1, 1), n)
    m = rs.randint(-8, 9, n)
    root = np.array([1, 3, 7])[rs.randint(0, 3, n)]
    gj = np.zeros(n, np.int64)
    for r, allowed in _GJ.items():
        k = root == r
        gj[k] = allowed[rs.randint(0, allowed.size, int(k.sum()))]
    for a in (p, m, root, gj):
        a.setflags(write=False)
    return p, m, root, gj


def mask_of(kind, n):
    if kind == "none":
        return None
    if kind == "checkered":                 # period 5 against the float4's 4: every lane is frozen alone somewhere
        return np.where(np.arange(n) % 5 == 0, 0.0, 1.0).astype(np.float32)
    return np.full(n, 1.0 if kind == "ones" else 0.0, np.float32)


def inputs(n, l2_n, mask="none", lr_from_device=False):
    p, m, root, gj = _draw(n)
    inside = np.arange(n) < l2_n
    g = 2 * gj - np.where(inside, p, 0)
    v = (4 * root * root - gj * gj) // 3
    assert (3 * v == 4 * root * root - gj * gj).all() and (v >= 0).all()
    f = lambda a: a.astype(np.float32)
    return dict(n=n, l2_n=l2_n, p=f(p), g=f(g), m=f(m), v=f(v), mask=mask_of(mask, n), lr_arg=LR_ARG,
                lr_dev=LR_DEV if lr_from_device else None)


def _fp32(x, what, check):
    if check:
        x = np.asarray(x, np.float64)
        assert np.array_equal(x, x.astype(np.float32).astype(np.float64)) and np.isfinite(x).all(), what + " is not an fp32 number"
    return x


def partials(sq_terms, n, G=None):
    """sq_partial[b] of a launch of G (default parts(n)) workgroups over per-element terms"""
    G = parts(n) if G is None else G
    block = ((np.arange(n) // 4) % (G * 256)) // 256
    return np.bincount(block, weights=sq_terms, minlength=G)


def adam(inp, defect=None, check=False, beta1=BETA1, beta2=BETA2):
    """dict p, m, v (float64 arrays), sq_partial (float64 per workgroup), total (Python int or float), l2_loss (np.float32)"""
    assert defect is None or defect in DEFECTS
    n, l2_n = inp["n"], inp["l2_n"]
    p, g, m, v = (inp[k].astype(np.float64) for k in "pgmv")
    lr = inp["lr_arg"] if inp["lr_dev"] is None or defect == "lr_dev ignored" else inp["lr_dev"]
    if defect == "beta1 and beta2 swapped":
        beta1, beta2 = beta2, beta1
    bound = l2_n
    if defect == "l2 boundary off by one":
        bound = l2_n - 1
    if defect == "l2 boundary rounded to the float4":
        bound = l2_n // 4 * 4
    inside = np.arange(n) < bound
    c = lambda x, what: _fp32(x, what, check)
    twol2 = c(2.0 * L2, "2 l2")
    if defect == "penalty l2 * p":
        twol2 = L2
    if defect == "grad_scale after the penalty":
        gj = np.where(inside, (g + twol2 * p) * GRAD_SCALE, g * GRAD_SCALE)
    else:
        gj = c(g * GRAD_SCALE, "g grad_scale")
        pen = c(twol2 * p, "2 l2 p")
        gj = c(np.where(inside, pen + gj, gj), "gj")
    one_b1, one_b2 = c(1.0 - beta1, "1 - beta1"), c(1.0 - beta2, "1 - beta2")
    m1 = c(c(beta1 * m, "beta1 m") + c(one_b1 * gj, "(1 - beta1) gj"), "m'")
    v1 = c(c(beta2 * v, "beta2 v") + c(c(one_b2 * gj, "(1 - beta2) gj") * gj, "(1 - beta2) gj gj"), "v'")
    if defect == "eps inside the root":
        den = np.sqrt(v1 + EPS)
    else:
        root = np.sqrt(v1)
        if check:
            assert np.array_equal(root * root, v1), "v' is not a perfect square"
        den = c(root + EPS, "sqrt(v') + eps")
        if check:
            assert np.array_equal(np.log2(den), np.round(np.log2(den))), "sqrt(v') + eps is not a power of two"
    p1 = c(p - c(c(lr * m1, "lr m'") / den, "lr m' / den"), "p'")
    frozen = np.zeros(n, bool) if inp["mask"] is None else inp["mask"] == 0
    sq_src = p1 if defect == "sq after the update" else p
    terms = c(np.where(inside, sq_src * sq_src, 0.0), "p p")
    if defect == "sq skips frozen elements":
        terms = np.where(frozen, 0.0, terms)
    p1 = np.where(frozen, p, p1)
    if defect != "mask does not restore m":
        m1 = np.where(frozen, m, m1)
    if defect != "mask does not restore v":
        v1 = np.where(frozen, v, v1)
    sq = partials(terms, n)
    if check:
        assert np.array_equal(sq, np.round(sq)) and sq.max() < 2.0 ** 24, "a workgroup's sum of squares reaches 2^24"
        assert sq.sum() < 2.0 ** 53
    return dict(p=p1, m=m1, v=v1, sq_partial=sq, total=float(sq.sum()), l2_loss=l2_sum(sq, L2))


def l2_sum(partial_sums, l2):
    """sum_partials_kernel: the partials in double, times (double)(float)l2, rounded to fp32 once.  Exact for integer partials
    whose sum stays below 2^53."""
    total = float(np.asarray(partial_sums, np.float64).sum())
    return np.float32(total * float(np.float32(l2)))


def l2_sum_partials(count):
    """integer partials for spnet_adam_l2_sum: up to 2^20 each, so that `count` of them pass 2^24 and the fp32 sum of the
    same numbers would not be exact while the double one is"""
    rs = np.random.RandomState(300 + count)
    return rs.randint(0, 1 << 20, count).astype(np.float32)


def ranges(n, cuts):
    """[(lo, hi)] of spnet_adam_part calls over [0, n) cut at `cuts`; an empty range is skipped, as the engine does"""
    edges = [0] + list(cuts) + [n]
    return [(lo, hi) for lo, hi in zip(edges[:-1], edges[1:]) if hi > lo]


def range_l2(l2_n, lo, hi):
    return max(0, min(l2_n, hi) - lo)


def adam_in_ranges(inp, cuts):
    """the same step as spnet_adam_part calls over ranges(): p, m, v as adam() (the update is element-wise); sq_partial is
    the concatenation of every range's own partials"""
    whole = adam(inp)
    sq = []
    for lo, hi in ranges(inp["n"], cuts):
        sub = dict(inp, n=hi - lo, l2_n=range_l2(inp["l2_n"], lo, hi), p=inp["p"][lo:hi], g=inp["g"][lo:hi], m=inp["m"][lo:hi],
                   v=inp["v"][lo:hi], mask=None if inp["mask"] is None else inp["mask"][lo:hi])
        part = adam(sub)
        for k in "pmv":
            assert np.array_equal(part[k], whole[k][lo:hi])
        sq.append(part["sq_partial"])
    sq = np.concatenate(sq)
    assert sq.sum() == whole["total"]
    return dict(whole, sq_partial=sq)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def outputs_differ(a, b):
    """True when any of p, m, v, sq_partial, l2_loss differs in its fp32 bits"""
    return any(not np.array_equal(bits(a[k]), bits(b[k])) for k in ("p", "m", "v", "sq_partial", "l2_loss"))
