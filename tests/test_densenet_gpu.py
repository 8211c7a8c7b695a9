"""DenseNet121 backbone on the device: every new kernel against fp64 torch, the whole network against the independent fp64
restatement (tests/helpers/densenet_ref.py), determinism, the 384x512 geometry, freshness after a load, the Model API and
the training CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.helpers import densenet_ref as R
from tests.parity_util import dropout_mask, rel_err

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")


def _L():
    from spnet_amd import _lib as L
    return L


def _st():
    return _L().current_stream()


def _coef(scale, shift):
    c = scale.numel()
    cld = (c + 31) // 32 * 32
    coef = torch.zeros(3 * cld, dtype=torch.float32)
    coef[:c] = scale
    coef[2 * cld:2 * cld + c] = shift
    return coef.cuda(), cld


# GEMM tolerance: the fp32 MFMA chain is a k-ordered fp32 dot product; against fp64 its error is ~sqrt(K) * 2^-24 of the
# row norm -- 1e-5 relative to the largest output covers K <= 992 with a wide margin (measured below 2e-6).
GEMM_TOL = 1e-5


@pytest.mark.parametrize("M,c,ldx,N", [(1000, 64, 96, 128), (517, 96, 96, 128), (2016, 480, 512, 128),
                                       (333, 992, 1024, 496)])
@pytest.mark.parametrize("stats", [False, True])
def test_bnrelu_gemm_against_fp64(M, c, ldx, N, stats):
    _need_gpu()
    L = _L()
    g = torch.Generator().manual_seed(M + c)
    x = torch.randn(M, ldx, generator=g)
    W = torch.randn(c, N, generator=g) / np.sqrt(c)
    scale, shift = 0.5 + torch.rand(c, generator=g), 0.3 * torch.randn(c, generator=g)
    coef, cld = _coef(scale, shift)
    ldy = N + 32
    Y = torch.full((M, ldy), 7.0).cuda()
    xd, Wd = x.cuda(), W.cuda()
    part = torch.zeros((M + 31) // 32 * 2 * N).cuda()
    import ctypes
    rows = ctypes.c_int(0)
    L.spnet_gemm_f32_bnrelu(xd.data_ptr(), ldx, coef.data_ptr(), cld, Wd.data_ptr(), N, Y.data_ptr(), ldy, M, N, c, 0,
                            part.data_ptr() if stats else None, ctypes.addressof(rows) if stats else None, _st())
    torch.cuda.synchronize()
    z = torch.relu(x[:, :c].double() * scale.double() + shift.double())
    want = z @ W.double()
    got = Y.cpu().double()
    assert rel_err(got[:, :N], want) < GEMM_TOL
    assert bool((got[:, N:] == 7.0).all())                      # nothing written past N in the strided output
    if stats:
        p = part.cpu().double()[:rows.value * 2 * N].reshape(rows.value, 2, N).sum(0)
        np.testing.assert_allclose(p[0].numpy(), want.sum(0).numpy(), rtol=1e-4, atol=1e-3 * float(want.abs().max()))
        np.testing.assert_allclose(p[1].numpy(), (want ** 2).sum(0).numpy(), rtol=1e-4)


@pytest.mark.parametrize("M,c", [(517, 64), (1000, 96), (777, 480), (300, 992)])
def test_consumer_backward_and_producer_finalize(M, c):
    """Two consumers of one concat buffer (c and c/2 channels; the first with ReLU, the second without) against fp64
    autograd of the summed BatchNorm backward: dgamma, dbeta of each and the finalized gradient of the channels."""
    _need_gpu()
    L = _L()
    g = torch.Generator().manual_seed(c)
    Cb = c + 32
    x = torch.randn(M, Cb, generator=g).double() * 1.5 + 0.3
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + R.EPS)
    cons = []
    for k, (cc, relu) in enumerate(((c, 1), (c // 2, 0))):
        gamma, beta = 0.5 + torch.rand(cc, generator=g).double(), 0.2 * torch.randn(cc, generator=g).double()
        dz = torch.randn(M, cc, generator=g).double()
        cons.append((cc, relu, gamma, beta, dz))
    # fp64 reference: y_l = act(BN_l(x[:, :c_l])) with the batch statistics, loss = sum(dz_l * y_l)
    xr = x.clone().requires_grad_(True)
    ps = [(gm.clone().requires_grad_(True), bt.clone().requires_grad_(True)) for _, _, gm, bt, _ in cons]
    loss = 0
    for (cc, relu, _, _, dz), (gm, bt) in zip(cons, ps):
        xs = xr[:, :cc]
        y = (xs - xs.mean(0)) / torch.sqrt(xs.var(0, unbiased=False) + R.EPS) * gm + bt
        loss = loss + (dz * (torch.relu(y) if relu else y)).sum()
    loss.backward()
    # device
    xd = x.float().cuda()
    G = torch.zeros(M, Cb).cuda()
    u, v = torch.zeros(Cb).cuda(), torch.zeros(Cb).cuda()
    meand, invd = mean.float().cuda(), invstd.float().cuda()
    P = int(L.spnet_dense_rows(M))
    part = torch.zeros(P * 2 * c).cuda()
    got_params = []
    for cc, relu, gamma, beta, dz in cons:
        sc = gamma * invstd[:cc]
        coef, cld = _coef(sc.float(), (beta - mean[:cc] * sc).float())
        gd, dzd = gamma.float().cuda(), dz.float().cuda()
        dgam, dbet = torch.zeros(cc).cuda(), torch.zeros(cc).cuda()
        L.spnet_dense_consumer_bwd(dzd.data_ptr(), cc, xd.data_ptr(), Cb, M, cc, coef.data_ptr(), cld, meand.data_ptr(),
                                   invd.data_ptr(), gd.data_ptr(), relu, G.data_ptr(), Cb, part.data_ptr(), _st())
        L.spnet_dense_consumer_fin(part.data_ptr(), P, cc, gd.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), u.data_ptr(),
                                   v.data_ptr(), _st())
        got_params.append((dgam, dbet))
    out = torch.full((M, c + 8), 5.0).cuda()
    L.spnet_dense_producer_fin(G.data_ptr(), Cb, u.data_ptr(), v.data_ptr(), xd.data_ptr(), Cb, meand.data_ptr(),
                               invd.data_ptr(), M, 0, c, out.data_ptr(), c + 8, _st())
    torch.cuda.synchronize()
    for (dgam, dbet), (gm, bt) in zip(got_params, ps):
        assert rel_err(dgam.cpu(), gm.grad) < 1e-4
        assert rel_err(dbet.cpu(), bt.grad) < 1e-4
    assert rel_err(out.cpu()[:, :c], xr.grad[:, :c]) < 1e-4
    assert bool((out.cpu()[:, c:] == 5.0).all())


@pytest.mark.parametrize("B,H,W", [(2, 33, 41), (3, 32, 40)])
def test_stem_conv7_and_padded_maxpool(B, H, W):
    """conv1/conv (explicit pad 3) and ZeroPadding2D(1) + the 3x3/2 valid max pool at odd and even planes: the even plane
    catches a TF-SAME substitution (SAME would pad 2/3 and 0/1 there)."""
    _need_gpu()
    L = _L()
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, H, W, 3, generator=g)
    w = torch.randn(7, 7, 3, 64, generator=g) / 12
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    xd, wd = x.cuda(), w.cuda()
    y = torch.zeros(B, OH, OW, 64).cuda()
    L.spnet_dense_conv7(0, xd.data_ptr(), wd.data_ptr(), y.data_ptr(), B, H, W, None, 0, _st())
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    yr = R.conv(F.pad(xr.permute(0, 3, 1, 2), (3, 3, 3, 3)).permute(0, 2, 3, 1), wr, stride=2)
    dy = torch.randn(yr.shape, generator=g).double()
    (yr * dy).sum().backward()
    dyd = dy.float().cuda()
    dx, dw = torch.zeros(B, H, W, 3).cuda(), torch.zeros(7, 7, 3, 64).cuda()
    ws = torch.zeros(int(L.spnet_dense_conv7_ws(B, H, W))).cuda()
    L.spnet_dense_conv7(1, dyd.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, H, W, None, 0, _st())
    L.spnet_dense_conv7(2, xd.data_ptr(), dyd.data_ptr(), dw.data_ptr(), B, H, W, ws.data_ptr(), ws.numel(), _st())
    torch.cuda.synchronize()
    assert y.shape[1:3] == yr.shape[1:3]
    assert rel_err(y.cpu(), yr.detach()) < GEMM_TOL
    assert rel_err(dx.cpu(), xr.grad) < GEMM_TOL
    assert rel_err(dw.cpu(), wr.grad) < 1e-5
    # padded max pool on a post-ReLU tensor (many ties at zero)
    z = torch.relu(torch.randn(B, H, W, 64, generator=g))
    zd = z.cuda()
    zp = torch.zeros(B, H + 2, W + 2, 64).cuda()
    L.spnet_pad_nhwc(zd.data_ptr(), zp.data_ptr(), B, H, W, 64, 1, 1, 1, 1, 0, _st())
    PH, PW = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1
    p = torch.zeros(B, PH, PW, 64).cuda()
    idx = torch.zeros(B * PH * PW * 16, dtype=torch.int32).cuda()
    L.spnet_maxpool3x3s2_valid_fwd(zp.data_ptr(), p.data_ptr(), idx.data_ptr(), B, H + 2, W + 2, 64, _st())
    want = R.maxpool_pad1(z.double())
    assert torch.equal(p.cpu().double(), want)
    # backward: the gradient lands on the recorded tap; cropped back to the unpadded plane.  Only windows whose maximum
    # is unique and positive carry a gradient, so that the routing is the only one possible (no tie order assumed).
    cols = F.unfold(F.pad(z.double().permute(0, 3, 1, 2), (1, 1, 1, 1)), 3, stride=2).reshape(B, 64, 9, PH, PW)
    mx = cols.max(2, keepdim=True).values
    uniq = (((cols == mx).sum(2) == 1) & (mx.squeeze(2) > 0)).permute(0, 2, 3, 1)
    assert float(uniq.double().mean()) > 0.5
    gp = (torch.randn(B, PH, PW, 64, generator=g) * uniq).cuda()
    dzp = torch.zeros(B, H + 2, W + 2, 64).cuda()
    dz = torch.zeros(B, H, W, 64).cuda()
    L.spnet_maxpool3x3s2_valid_bwd(gp.data_ptr(), idx.data_ptr(), dzp.data_ptr(), B, H + 2, W + 2, 64, _st())
    L.spnet_pad_nhwc(dzp.data_ptr(), dz.data_ptr(), B, H, W, 64, 1, 1, 1, 1, 1, _st())
    torch.cuda.synchronize()
    assert torch.equal(dz.cpu(), dzp.cpu()[:, 1:H + 1, 1:W + 1])
    zr = z.double().requires_grad_(True)
    (R.maxpool_pad1(zr) * gp.cpu().double()).sum().backward()
    assert rel_err(dz.cpu(), zr.grad) < 1e-6             # (an element may be the maximum of up to four windows)


def _case(H, W, B, seed):
    from spnet_amd.engine import param_specs
    specs = param_specs(H, W, backbone="DenseNet121")
    P = R.random_params([(n, s) for n, s, _, _ in specs], 100 + seed)
    rs = np.random.RandomState(seed)
    X = torch.tensor(rs.rand(B, H, W, 1) * 2 - 1, dtype=torch.float32)
    Y = torch.tensor(rs.rand(B, 576), dtype=torch.float32)
    Y[:, 6::8] = (Y[:, 6::8] > 0.5).float()
    dseed = 777 + seed
    mask = torch.tensor(dropout_mask(B * (H // 2) * (W // 2) * 3, dseed).reshape(B, H // 2, W // 2, 3))
    return P, X, Y, mask, dseed


def densenet_decisions(eng):
    """The discrete decisions of the engine's last TRAINING forward, rebuilt from the tensors it keeps, in the order
    tests/helpers/densenet_ref.py applies them (after the stem's, which parity_util.device_decisions rebuilds):
      conv1/relu      sign of fmaf(y0, scale, shift) as spnet_bn_apply computes it (y0 and the batch affine are kept)
      pool1           the byte arg-max taps the pool kernel saved for backward (windows of the zero-padded plane)
      _0_relu, pool*_relu   the consumer's BN+ReLU is applied on load, relu(fmaf(scale, x, shift)), from the concat
                      buffer X and the consumer's coefficients
      _1_relu         sign of the materialised bottleneck activation z1
    x * scale + shift in float64 has the sign of the exact value, which is the sign fmaf rounds to."""
    from tests.parity_util import device_decisions
    base = device_decisions(eng)
    net = eng._densenet
    cpu = lambda t: t.detach().cpu()
    relu, pool = list(base.relu), list(base.pool)
    C = 64
    ss = cpu(net.bn0.ss).double()
    relu.append((cpu(net.y0).double() * ss[:C] + ss[C:]) > 0)
    B = net.B
    taps = cpu(net.idx).view(torch.uint8).reshape(B, net.h2, net.w2, C).long()
    pool.append(taps.permute(0, 3, 1, 2).unsqueeze(2))

    def lazy(blk, cons, c):
        coef = cpu(cons.coef).double()
        x = cpu(blk.X).double()[:, :c]
        return ((x * coef[:c] + coef[2 * cons.cld:2 * cons.cld + c]) > 0).reshape(B, blk.h, blk.w, c)

    for blk in net.blocks:
        for lay in blk.layers:
            relu.append(lazy(blk, lay["cons"], lay["c"]))
            relu.append((cpu(lay["z1"]) > 0).reshape(B, blk.h, blk.w, -1))
        if blk.trans:
            relu.append(lazy(blk, blk.tcons, blk.Cb))
    from oracle import torch_ref as T
    return T.Decisions(relu, pool)


# Whole-network gradients against the fp64 restatement evaluated on the DEVICE's ReLU masks and pool taps (as the other
# backbones' parity tests do): every tensor within parity_util.GRAD_TOL, and every decision the device took differently
# from fp64 must have been a tie at fp32 resolution.  (Without the device's decisions the comparison measures the
# network's rounding sensitivity, not the kernels: plain fp32 torch deviates from fp64 by up to 0.19 per tensor here.)
@pytest.mark.parametrize("H,W,B,seed", [(288, 224, 2, 0), (235, 301, 3, 1)])
def test_densenet_forward_and_gradients(H, W, B, seed):
    _need_gpu()
    from spnet_amd.engine import Engine
    from tests.parity_util import GRAD_TOL
    P, X, Y, mask, dseed = _case(H, W, B, seed)
    eng = Engine(H, W, B, device="cuda:0", seed=1, backbone="DenseNet121")
    assert sorted(eng.state_dict().keys()) == sorted(P.keys())
    eng.load_state_dict(P)
    with torch.no_grad():
        want = R.forward({k: v.double() for k, v in P.items()}, X.double(), training=False)
    got = eng.forward(X.cuda(), training=False).cpu()
    assert rel_err(got, want) < 1e-4
    eng.set_drop_seed(dseed)
    out = eng.forward(X.cuda(), training=True)
    loss = eng.loss(Y.cuda())
    eng.backward()
    torch.cuda.synchronize()
    dec = densenet_decisions(eng)
    data64, g64, yp64, P64 = R.grads(P, X, Y, mask, decisions=dec)
    assert dec._ri == len(dec.relu) and dec._pi == len(dec.pool), "decision sites out of step with the helper"
    far = [f for f in dec.flips if f[2] > 1e-5]
    assert not far, "device decisions differ from fp64's away from ties: %s" % far[:8]
    assert rel_err(out.cpu(), yp64) < 1e-4
    np.testing.assert_allclose(float(loss[5]), data64, rtol=1e-4)
    sd = eng.state_dict()
    for k in P:
        if k.endswith("moving_mean") or k.endswith("moving_variance"):
            np.testing.assert_allclose(sd[k].numpy(), P64[k].numpy(), rtol=1e-4, atol=1e-5, err_msg=k)
    gd = eng.grad_dict()
    assert set(g64) == {k for k in P if not (k.endswith("moving_mean") or k.endswith("moving_variance"))}
    bad = {k: rel_err(gd[k], g64[k]) for k in g64 if not rel_err(gd[k], g64[k]) < GRAD_TOL}
    assert not bad, sorted(bad.items(), key=lambda kv: -kv[1])[:8]


def test_densenet_step_is_bit_exact():
    _need_gpu()
    from spnet_amd.engine import Engine
    H, W, B = 160, 192, 2
    P, X, Y, mask, dseed = _case(H, W, B, 3)
    eng = Engine(H, W, B, device="cuda:0", seed=1, backbone="DenseNet121")
    res = []
    for _ in range(2):
        eng.load_state_dict(P)
        eng.set_drop_seed(dseed)
        eng.forward(X.cuda(), training=True)
        loss = eng.loss(Y.cuda()).clone()
        eng.backward()
        torch.cuda.synchronize()
        res.append((loss.cpu(), eng.grad.clone().cpu()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_densenet_bench_geometry_and_freshness():
    """384x512, batch 16: inference against the fp64 model on two frames, batch 16 == batch 2 to rounding, captured
    predict_step == eager, a load between two predict_steps is seen; training: finite gradients, loss falls over 8
    steps."""
    _need_gpu()
    from spnet_amd.engine import Engine
    H, W = 384, 512
    P, X2, _, _, _ = _case(H, W, 2, 5)
    rs = np.random.RandomState(6)
    X = torch.tensor(rs.rand(16, H, W, 1) * 2 - 1, dtype=torch.float32)
    X[:2] = X2
    e16 = Engine(H, W, 16, device="cuda:0", seed=1, backbone="DenseNet121", train=False)
    assert e16.backbone_out.shape == (16, 6, 8, 1024)
    e16.load_state_dict(P)
    y16 = e16.forward(X.cuda(), training=False).cpu().clone()
    assert bool(torch.isfinite(y16).all())
    with torch.no_grad():
        want = R.forward({k: v.double() for k, v in P.items()}, X2.double(), training=False)
    assert rel_err(y16[:2], want) < 1e-4
    e2 = Engine(H, W, 2, device="cuda:0", share_from=e16, backbone="DenseNet121", train=False)
    scale = float(y16.abs().max())
    for lo in range(0, 16, 4):
        y2 = e2.forward(X[lo:lo + 2].cuda(), training=False).cpu()
        np.testing.assert_allclose(y16[lo:lo + 2].numpy(), y2.numpy(), rtol=1e-4, atol=1e-5 * scale)
    e16.x_in.copy_(X.cuda())
    a = e16.predict_step().clone()
    b = e16.predict_step().clone()
    assert torch.equal(a, b) and torch.equal(a.cpu(), y16)
    # stale-weights check: new weights AND moving statistics between two replays
    P2, _, _, _, _ = _case(H, W, 2, 9)
    e16.load_state_dict(P2)
    c = e16.predict_step().clone().cpu()
    with torch.no_grad():
        want2 = R.forward({k: v.double() for k, v in P2.items()}, X2.double(), training=False)
    assert rel_err(c[:2], want2) < 1e-4
    del e2, e16
    torch.cuda.empty_cache()
    t16 = Engine(H, W, 16, device="cuda:0", seed=1, backbone="DenseNet121")
    t16.load_state_dict(P)
    Y = torch.tensor(rs.rand(16, 576), dtype=torch.float32)
    Y[:, 6::8] = (Y[:, 6::8] > 0.5).float()
    losses = []
    for i in range(8):
        t16.set_drop_seed(11 + i)
        lo = t16.train_step(X.cuda(), Y.cuda(), 1e-4)
        if i == 0:
            torch.cuda.synchronize()
            assert bool(torch.isfinite(t16.grad).all())
        losses.append(float(lo[5]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_densenet_model_api_and_cli(tmp_path):
    _need_gpu()
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as FE
    from spnet_amd import models as M
    old = cf.basemodel
    cf.basemodel = "DenseNet121"
    try:
        m = M.Model((160, 192, 1), Y0size=576, seed=3)
        assert m.basemodel == "DenseNet121"
        rs = np.random.RandomState(0)
        X = (rs.rand(8, 160, 192, 1) * 2 - 1).astype(np.float32)
        Y = rs.rand(8, 576).astype(np.float32)
        m.fit(X, Y, batch_size=4, epochs=1, verbose=0)
        p = m.predict(X[:4], batch_size=4)
        path = str(tmp_path / "m.safetensors")
        m.save(path)
    finally:
        cf.basemodel = old
    m2 = M.load_model(path)
    assert m2.basemodel == "DenseNet121"
    np.testing.assert_array_equal(m2.predict(X[:4], batch_size=4), p)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = tmp_path / "data"
    FE.write_dataset(str(data / "Train"), 16, seed=1)
    FE.write_dataset(str(data / "Val"), 8, seed=2)
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([sys.executable, os.path.join(root, "train_spnet.py"), "-d", str(data), "-b", "8", "-e", "1",
                        "--name", "dn", "--backbone", "DenseNet121"], cwd=str(work), env=dict(os.environ, PYTHONPATH=root),
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + "\n" + r.stderr[-3000:]
    assert "cf.basemodel = DenseNet121" in r.stdout and "SPNet execution completed." in r.stdout
