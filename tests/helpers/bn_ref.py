"""Plain high-precision references for the BatchNorm family of csrc/bn.hip (TEST INFRASTRUCTURE).  They restate the
operation, not the kernels: no tiling, no summation order.  tests/test_bn_ref_cpu.py pins them against the oracle
(oracle/torch_ref.py), a two-pass mean / variance and a central difference.

  finalize_bits   the one place that follows the device code rounding by rounding: bn_channel_stats + bn_moving_update +
                  bn_shift of csrc/common.h, which pin every rounding so that three kernels give the same bits
  forward         float64 act(BN(x)) + residual, training (two-pass batch statistics) or inference (moving statistics)
  backward        the same through torch autograd in float64; the activation's derivative is supplied explicitly
                  (act_grad), because its value AT a kink is a convention and the convention is what is under test
  backward_saved  the closed form the kernels evaluate, on GIVEN saved statistics (spnet_bn_bwd takes save_mean /
                  save_invstd as inputs and never checks that they are the batch's); == backward on the batch's own
  bwd_coeffs      [k1 | k2' | k3'] of bn_bwd_finalize_kernel<1>: dx = k1*g + k2'*x + k3' on the raw x
Acts: 0 none, 1 ReLU, 2 LeakyReLU(float32(0.1)), 3 ReLU6."""
from fractions import Fraction

import numpy as np
import torch

U =2.0 ** -24                      # unit roundoff of fp32
LEAK = float(np.float32(0.1))       # the slope the kernels multiply by (0.1f), exactly


# ----------------------------------------------------------------------------- the finalize step, rounding by rounding
def _round_f32(fr):
    """the fp32 nearest to the exact rational fr, ties to even (no double rounding through float64)"""
    c = np.float32(float(fr))
    cands = [np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))]
    cands = [k for k in cands if np.isfinite(k)]
    return min(cands, key=lambda k: (abs(Fraction(float(k)) - fr), int(np.array(k, np.float32).view(np.uint32)) & 1))


def fma32(a, b, c):
    """fmaf(a, b, c) elementwise on fp32 arrays, exactly: one rounding of the exact a*b + c"""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32) for v in (a, b, c)))
    out = [_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())]
    return np.array(out, np.float32).reshape(a.shape)


def fma64(a, b, c):
    """fma(a, b, c) elementwise on float64 arrays, exactly (Fraction -> float rounds correctly)"""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (a, b, c)))
    out = [float(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())]
    return np.array(out, np.float64).reshape(a.shape)


def finalize_bits(s, q, M, gamma, beta, eps, momentum, mm, mv):
    """(mean, invstd, scale, shift, moving_mean, moving_var) as fp32 from the column sums s, q (float64) over M values.
    Double: s/M, q/M, var = fma(-mean, mean, q/M) (ONE rounding; clamped at 0), var + eps, sqrt, reciprocal,
    var * (M/(M-1)).  fp32: gamma*invstd, shift = fmaf(-mean, scale, beta) (ONE rounding), 1 - momentum, the two products
    and the sum of the moving update, each rounded on its own.  numpy rounds every plain operation on its own (IEEE, no
    contraction), sqrt and division correctly; the two fused operations are evaluated exactly and rounded once."""
    s, q = np.asarray(s, np.float64), np.asarray(q, np.float64)
    f32 = np.float32
    gamma, beta, mm, mv = (np.asarray(a, f32) for a in (gamma, beta, mm, mv))
    eps, momentum = f32(eps), f32(momentum)
    Md = np.float64(M)
    mean = s / Md
    var = fma64(-mean, mean, q / Md)
    var = np.where(var < 0.0, 0.0, var)
    mean32 = mean.astype(f32)
    invstd = (1.0 / np.sqrt(var + np.float64(eps))).astype(f32)
    scale = gamma * invstd
    shift = fma32(-mean32, scale, beta)
    unbiased = (var * (Md / np.float64(M - 1)) if M > 1 else var).astype(f32)
    one_m = f32(1.0) - momentum
    new_mm = momentum * mm + one_m * mean32
    new_mv = momentum * mv + one_m * unbiased
    out = (mean32, invstd, scale, shift, new_mm, new_mv)
    assert all(a.dtype == f32 for a in out)
    return out


# ----------------------------------------------------------------------------- activations and their conventions
def act_fwd(t, act):
    if act == 1:
        return torch.clamp_min(t, 0.0)
    if act == 2:
        return torch.where(t > 0, t, LEAK * t)
    if act == 3:
        return torch.clamp(t, 0.0, 6.0)
    return t


def act_grad(t, act):
    """The derivative the port uses, kinks included: ReLU 0 at 0; ReLU6 0 at 0 and at 6; LeakyReLU the slope at 0 (what
    TF's ReluGrad / Relu6Grad / LeakyReluGrad compute)."""
    one = torch.ones_like(t)
    if act == 1:
        return torch.where(t > 0, one, 0.0 * one)
    if act == 2:
        return torch.where(t > 0, one, LEAK * one)
    if act == 3:
        return torch.where((t > 0) & (t < 6), one, 0.0 * one)
    return one


class _Act(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, act):
        ctx.save_for_backward(t)
        ctx.act = act
        return act_fwd(t, act)

    @staticmethod
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        return g * act_grad(t, ctx.act), None


def _d(a):
    return torch.as_tensor(a).detach().double()


def batch_stats(x):
    """two-pass mean and biased variance over the rows of [M][C], float64"""
    x = _d(x)
    mu = x.mean(0)
    return mu, ((x - mu) ** 2).mean(0)


def _bn(x, gamma, beta, mean, var, eps):
    return (x - mean) * torch.rsqrt(var + eps) * gamma + beta


def forward(x, gamma, beta, act, residual=None, res_bcast=False, training=True, moving_mean=None, moving_var=None,
            eps=float(np.float32(1e-3))):
    """float64 y = act(BN(x)) + residual for x [M][C]; res_bcast: residual [M], one value per pixel.  Returns a dict:
    y, out_pre (the activation's argument), mean, var (the statistics used), invstd."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    mean, var = batch_stats(x) if training else (_d(moving_mean), _d(moving_var))
    pre = _bn(x, gamma, beta, mean, var, eps)
    y = act_fwd(pre, act)
    if residual is not None:
        r = _d(residual)
        y = y + (r.reshape(-1, 1) if res_bcast else r)
    return dict(y=y, out_pre=pre, mean=mean, var=var, invstd=torch.rsqrt(var + eps))


def backward(x, dy, gamma, beta, act, training=True, moving_mean=None, moving_var=None, eps=float(np.float32(1e-3))):
    """(dx, dgamma, dbeta) of sum(dy * act(BN(x))) by autograd in float64 (a residual passes dy through unchanged)."""
    x, gamma, beta = (_d(a).requires_grad_(True) for a in (x, gamma, beta))
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = _d(moving_mean), _d(moving_var)
    y = _Act.apply(_bn(x, gamma, beta, mean, var, eps), act)
    y.backward(_d(dy))
    return x.grad, gamma.grad, beta.grad


def backward_saved(x, dy, gamma, beta, mean, invstd, act, absolute=False):
    """The training backward on GIVEN statistics, float64: xhat = (x - mean)*invstd, g = dy * act'(xhat*gamma + beta),
    dbeta = sum g, dgamma = sum g*xhat, dx = gamma*invstd*(g - dbeta/M - xhat*dgamma/M).  Returns a dict with those and
    xhat, g, out_pre, k1, k2, k3 (dx = k1*g + k2*xhat + k3).
    absolute=True: the companion of form (3) -- the same sums over |terms| (the mask still from the signed out_pre):
    sg = sum|g|, sgx = sum|g*xhat|, dx = |k1 g| + |xhat| a sum|g xhat|/M + a sum|g|/M."""
    x, dy, gamma, beta, mean, invstd = (_d(a) for a in (x, dy, gamma, beta, mean, invstd))
    M = x.shape[0]
    xh = (x - mean) * invstd
    pre = xh * gamma + beta
    g = dy * act_grad(pre, act)
    a = gamma * invstd
    if absolute:
        g, xh, a = g.abs(), xh.abs(), a.abs()
    sg, sgx = g.sum(0), (g * xh).sum(0)
    if absolute:
        k1, k2, k3 = a, a * sgx / M, a * sg / M
    else:
        k1, k2, k3 = a, -a * sgx / M, -a * sg / M
    return dict(dx=k1 * g + k2 * xh + k3, dgamma=sgx, dbeta=sg, xhat=xh, g=g, out_pre=pre, k1=k1, k2=k2, k3=k3)


def bwd_coeffs(sg, sgx, M, gamma, mean, invstd):
    """float64 (k1, k2', k3') with dx = k1*g + k2'*x + k3' on the RAW x: k2' = k2*invstd, k3' = k3 - k2*invstd*mean."""
    sg, sgx, gamma, mean, invstd = (_d(a) for a in (sg, sgx, gamma, mean, invstd))
    a = gamma * invstd
    k2, k3 = -a * sgx / M, -a * sg / M
    return a, k2 * invstd, k3 - k2 * invstd * mean


def row_group_sums(x, P, second=None):
    """partial[P][2][C] in float64: rows of x [M][C] dealt to P contiguous groups (row r -> group r*P // M; groups may be
    empty), per group the column sums of x and of x*x (second=None) or of x and x*second."""
    x = _d(x)
    M, C = x.shape
    gid = (torch.arange(M, device=x.device) * P) // M
    out = torch.zeros(P, 2, C, dtype=torch.float64, device=x.device)
    out[:, 0].index_add_(0, gid, x)
    out[:, 1].index_add_(0, gid, x * (x if second is None else _d(second)))
    return out
