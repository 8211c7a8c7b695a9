"""The references of tests/helpers/bn_ref.py against what the project already trusts (no GPU needed): finalize_bits
against a two-pass float64 mean / variance, the float64 forward / backward against oracle/torch_ref.py's batchnorm and
torch's own activations, the closed form on saved statistics and the blend coefficients against autograd, and the
explicit ReLU6 derivative against a central difference."""
import numpy as np
import pytest
import torch

from oracle import torch_ref as T
from tests.helpers import bn_ref as B

U = B.U


@pytest.mark.parametrize("M,C,loc,scale", [(1, 5, 0.3, 1.5), (2, 5, 0.3, 1.5), (1000, 7, 0.3, 1.5), (1000, 7, 30.0, 1.0), (4096, 3, -2.0, 1e-2)])
def test_finalize_bits_against_the_two_pass_statistics(M, C, loc, scale):
    """s and q are formed in float64 from fp32 data (relative error <= M * 2^-53 each); from there finalize_bits performs
    a dozen roundings.  The variance q/M - mean^2 cancels, so its error is measured against q/M: 4 * 2^-53 * q/M covers the
    two divisions, the product, the difference and the sums' own error for M <= 4096.  Every fp32 result is then within
    one rounding per step of the float64 value of the same expression."""
    rs = np.random.RandomState(M + C)
    x = (rs.randn(M, C) * scale + loc).astype(np.float32)
    gamma, beta = (rs.rand(C) + 0.5).astype(np.float32), rs.randn(C).astype(np.float32)
    mm, mv = rs.randn(C).astype(np.float32), (rs.rand(C) + 0.5).astype(np.float32)
    x64 = x.astype(np.float64)
    eps32, mom32 = np.float32(1e-3), np.float32(0.99)
    mean, invstd, sc, sh, nmm, nmv = B.finalize_bits(x64.sum(0), (x64 * x64).sum(0), M, gamma, beta, 1e-3, 0.99, mm, mv)
    mu = x64.mean(0)
    var = ((x64 - mu) ** 2).mean(0)
    q_m = (x64 * x64).mean(0)
    dvar = (4 + 2 * M) * 2.0 ** -53 * q_m                                   # what the one-pass form loses, in float64
    inv = 1.0 / np.sqrt(var + np.float64(eps32))
    dinv = 0.5 * inv ** 3 * dvar
    assert (np.abs(mean - mu) <= U * np.abs(mu) * (1 + 1e-6)).all()                      # one rounding to fp32
    assert (np.abs(invstd - inv) <= U * inv * (1 + 1e-6) + 2 * dinv).all()
    assert (np.abs(sc - gamma * inv) <= 2 * U * np.abs(gamma * inv) * (1 + 1e-6) + 2 * np.abs(gamma) * dinv).all()   # invstd, product
    # shift: the roundings of mean, scale (two), the product and the difference
    sh_ref = beta - mu * gamma * inv
    sh_abs = np.abs(beta) + np.abs(mu * gamma * inv)
    assert (np.abs(sh - sh_ref) <= 5 * U * sh_abs + 2 * np.abs(mu * gamma) * dinv).all()
    unb = var * M / max(M - 1, 1)
    one_m = np.float64(np.float32(1) - mom32)
    mm_ref, mv_ref = np.float64(mom32) * mm + one_m * mu, np.float64(mom32) * mv + one_m * unb
    assert (np.abs(nmm - mm_ref) <= 3 * U * (np.abs(mom32 * mm) + np.abs(one_m * mu))).all()          # value, product, sum
    assert (np.abs(nmv - mv_ref) <= 3 * U * (np.abs(mom32 * mv) + np.abs(one_m * unb)) + one_m * dvar * 2).all()
    if M == 1:
        assert (nmv == (mom32 * mv + (np.float32(1) - mom32) * np.float32(0))).all()     # M = 1: no Bessel factor, var = 0


def test_fused_operations_round_once():
    """fma32 / fma64 against cases where rounding the product first, or rounding through float64, gives another result."""
    a = np.float32(1 + 2.0 ** -12)
    assert B.fma32(a, a, -1.0)[()] == np.float32(2.0 ** -11 + 2.0 ** -24)                  # the product's low bit survives
    assert np.float32(a * a) - np.float32(1) == np.float32(2.0 ** -11)                     # ... and is lost unfused
    # 1 + 2^-24 + 2^-60 lies above the tie: fp32 must round up, float64 first rounds the tail away and then ties to even
    assert B.fma32(np.float32(2.0 ** -30), np.float32(2.0 ** -30), np.float32(1))[()] == np.float32(1)
    x = np.float32(1 + 2.0 ** -23)
    assert B.fma32(np.float32(2.0 ** -24 + 2.0 ** -47), np.float32(1), x)[()] == np.nextafter(x, np.float32(2))
    b = 1 + 2.0 ** -30
    assert B.fma64(b, b, -1.0)[()] == 2.0 ** -29 + 2.0 ** -60 and b * b - 1.0 == 2.0 ** -29
    rs = np.random.RandomState(0)
    u, v, w = (rs.randn(200).astype(np.float32) for _ in range(3))
    exact = u.astype(np.float64) * v + w                                                   # one float64 rounding
    assert (np.abs(B.fma32(u, v, w) - exact) <= B.U * np.abs(exact) * (1 + 1e-6)).all()


def test_finalize_bits_clamps_a_negative_variance():
    """sums that leave q/M - mean^2 slightly negative: var = 0, invstd = float32(1/sqrt(eps))"""
    M = 1000
    s = np.array([700.0, 0.0])
    q = np.array([490.0 - 1e-9, 0.0])
    one = np.ones(2, np.float32)
    mean, invstd, sc, sh, nmm, nmv = B.finalize_bits(s, q, M, one, 0 * one, 1e-3, 0.99, 0 * one, one)
    want = np.float32(1.0 / np.sqrt(np.float64(np.float32(1e-3))))
    assert (invstd == want).all() and (nmv == np.float32(0.99) * one).all()


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,C", [(50, 8), (7, 3)])
def test_forward_and_backward_equal_the_oracle(M, C, act):
    """oracle/torch_ref.py's batchnorm + torch's relu / leaky_relu and their autograd, in float64.  (The oracle's slope is
    the double 0.1, the port's float32(0.1): the reference is given the oracle's for this comparison.)"""
    rs = np.random.RandomState(M + act)
    x = torch.tensor(rs.randn(M, C) * 1.5 + 0.3, dtype=torch.float64, requires_grad=True)
    gamma = torch.tensor(rs.rand(C) + 0.5, dtype=torch.float64, requires_grad=True)
    beta = torch.tensor(rs.randn(C) * 0.2, dtype=torch.float64, requires_grad=True)
    mm, mv = torch.tensor(rs.randn(C), dtype=torch.float64), torch.tensor(rs.rand(C) + 0.5, dtype=torch.float64)
    res, dy = torch.tensor(rs.randn(M, C), dtype=torch.float64), torch.tensor(rs.randn(M, C), dtype=torch.float64)
    f = {0: lambda t: t, 1: torch.relu, 2: lambda t: torch.nn.functional.leaky_relu(t, 0.1)}[act]
    leak, B.LEAK = B.LEAK, 0.1
    try:
        for training in (True, False):
            for t in (x, gamma, beta):
                t.grad = None
            y = f(T.batchnorm(x, gamma, beta, mm.clone(), mv.clone(), training=training)) + res
            y.backward(dy)
            got = B.forward(x, gamma, beta, act, residual=res, training=training, moving_mean=mm, moving_var=mv, eps=T.BN_EPS)
            dx, dg, db = B.backward(x, dy, gamma, beta, act, training=training, moving_mean=mm, moving_var=mv, eps=T.BN_EPS)
            np.testing.assert_allclose(got["y"].numpy(), y.detach().numpy(), rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(dx.numpy(), x.grad.numpy(), rtol=1e-11, atol=1e-12)
            np.testing.assert_allclose(dg.numpy(), gamma.grad.numpy(), rtol=1e-11, atol=1e-11)
            np.testing.assert_allclose(db.numpy(), beta.grad.numpy(), rtol=1e-11, atol=1e-11)
    finally:
        B.LEAK = leak


def test_broadcast_residual():
    rs = np.random.RandomState(3)
    x, r = rs.randn(9, 3), rs.randn(9)
    g, b = np.ones(3), np.zeros(3)
    a = B.forward(x, g, b, 1, residual=r, res_bcast=True)["y"]
    c = B.forward(x, g, b, 1, residual=np.repeat(r[:, None], 3, 1))["y"]
    assert torch.equal(a, c)


@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_closed_form_on_saved_statistics_and_blend_coefficients(act):
    """On the batch's own statistics backward_saved is autograd's gradient; dx = k1*g + k2'*x + k3' reproduces it."""
    rs = np.random.RandomState(act)
    M, C = 40, 6
    x, dy = rs.randn(M, C) * 2 + 1, rs.randn(M, C)
    gamma, beta = rs.rand(C) * 3 + 0.5, rs.randn(C) + 2
    dx, dg, db = B.backward(x, dy, gamma, beta, act)
    mean, var = B.batch_stats(x)
    invstd = torch.rsqrt(var + float(np.float32(1e-3)))
    r = B.backward_saved(x, dy, gamma, beta, mean, invstd, act)
    np.testing.assert_allclose(r["dx"].numpy(), dx.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(r["dgamma"].numpy(), dg.numpy(), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(r["dbeta"].numpy(), db.numpy(), rtol=1e-11, atol=1e-12)
    k1, k2, k3 = B.bwd_coeffs(r["dbeta"], r["dgamma"], M, gamma, mean, invstd)
    np.testing.assert_allclose((k1 * r["g"] + k2 * torch.as_tensor(x) + k3).numpy(), dx.numpy(), rtol=1e-10, atol=1e-11)
    if act == 3:
        share = (r["out_pre"] >= 6).double().mean()
        assert 0.02 < float(share) < 0.5                  # the upper clamp takes part
    ra = B.backward_saved(x, dy, gamma, beta, mean, invstd, act, absolute=True)
    assert bool((ra["dx"] >= r["dx"].abs() - 1e-12).all()) and bool((ra["dgamma"] >= r["dgamma"].abs() - 1e-12).all())


def test_relu6_derivative_against_a_central_difference():
    """away from the kinks (|t| and |t - 6| >= 0.01, h = 1e-3) the explicit derivative is the slope of act_fwd; at the
    kinks it is the convention: 0 at 0 and at 6 (and equals torch's hardtanh / relu6 autograd everywhere)."""
    t = torch.linspace(-3, 9, 2401, dtype=torch.float64)
    t = t[((t.abs() >= 0.01) & ((t - 6).abs() >= 0.01))]
    h = 1e-3
    fd = (B.act_fwd(t + h, 3) - B.act_fwd(t - h, 3)) / (2 * h)
    assert float((fd - B.act_grad(t, 3)).abs().max()) < 1e-9
    k = torch.tensor([0.0, -0.0, 6.0], dtype=torch.float64)
    assert B.act_grad(k, 3).tolist() == [0.0, 0.0, 0.0]
    assert B.act_grad(k, 1).tolist() == [0.0, 0.0, 1.0]
    assert B.act_grad(k, 2).tolist() == [B.LEAK, B.LEAK, 1.0]
    tt = torch.cat([t, k]).requires_grad_(True)
    torch.nn.functional.relu6(tt).sum().backward()
    assert torch.equal(tt.grad, B.act_grad(tt.detach(), 3))
    tt.grad = None
    torch.relu(tt).sum().backward()
    assert torch.equal(tt.grad, B.act_grad(tt.detach(), 1))


def test_row_group_sums():
    x = torch.arange(35, dtype=torch.float64).reshape(7, 5)
    for P in (1, 3, 7, 10):
        p = B.row_group_sums(x, P)
        assert p.shape == (P, 2, 5)
        assert torch.equal(p.sum(0)[0], x.sum(0)) and torch.equal(p.sum(0)[1], (x * x).sum(0))
