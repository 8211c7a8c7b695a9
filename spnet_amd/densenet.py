"""keras.applications.densenet.DenseNet121(include_top=False) behind the stem (Keras 2.1.3; call site spnet/models.py:357-359
with cf.basemodel = 'DenseNet121'): the network definition and the DenseNetBackbone node of the engine.

Layer recipe (Keras 2.1.3):
  stem         ZeroPadding2D(3) - Conv2D(64, 7, 2, valid) 'conv1/conv' - BN 'conv1/bn' - ReLU - ZeroPadding2D(1) -
               MaxPooling2D(3, 2, valid) 'pool1'
  dense blocks conv2..conv5 with 6, 12, 24, 16 layers; layer convB_blockI = BN _0_bn - ReLU - Conv2D(128, 1) _1_conv -
               BN _1_bn - ReLU - Conv2D(32, 3, same) _2_conv - Concatenate([x, new])
  transitions  pool2..pool4 = BN _bn - ReLU - Conv2D(C/2, 1) _conv - AveragePooling2D(2, 2)
  closing      BN 'bn' (no ReLU in Keras 2.1.3)
Every DenseNet BatchNormalization has eps 1.001e-5, momentum 0.99 and a gamma.

Execution (DenseNetBackbone): a block's Concatenate buffer X [M][Cb] is allocated once at its final width; every
layer's 3x3 convolution writes its 32 channels straight into their column slice (spnet_conv_gemm_f32, ldy = Cb) and
its GEMM epilogue leaves their batch statistics.  Those statistics are shared by every consumer BatchNorm of the channel;
each consumer's BN + ReLU is applied while its 1x1 GEMM stages the A tile (spnet_gemm_f32_bnrelu), so the
pre-activation tensor is never written.  Backward accumulates the consumers' BatchNorm backward in G / u / v and turns it
into the true gradient of a producer's channels in one pass (csrc/densenet.hip)."""
import ctypes

import torch

from . import _lib as L

DN_EPS = 1.001e-5
DN_MOMENTUM = 0.99
DN_BLOCKS = (6, 12, 24, 16)
DN_GROWTH = 32
DN_BOTTLENECK = 128


def densenet_out_hw(H, W):
    """Output plane of DenseNet121 behind the stem for H x W frames."""
    h, w = H // 2, W // 2                                  # stem (AveragePooling2D(2))
    h, w = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1      # ZeroPadding2D(3) + conv 7x7 / 2
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1      # ZeroPadding2D(1) + max pool 3x3 / 2
    for _ in range(3):                                     # transitions: AveragePooling2D(2) floors
        h, w = h // 2, w // 2
    return h, w


def densenet_blocks():
    """[(block name, input channels, layers, transition name | None)] of the four dense blocks."""
    out, c = [], 64
    for i, n in enumerate(DN_BLOCKS):
        out.append(("conv%d" % (i + 2), c, n, "pool%d" % (i + 2) if i < 3 else None))
        c = (c + DN_GROWTH * n) // 2 if i < 3 else c + DN_GROWTH * n
    return out


def densenet_layers():
    """Keras layers of the backbone in creation order: [(name, kind, weight prefix | None)], kind in zeropad, conv, bn,
    relu, maxpool, concat, avgpool."""
    t = [("zero_padding2d_1", "zeropad", None), ("conv1/conv", "conv", "conv1/conv"), ("conv1/bn", "bn", "conv1/bn"),
         ("conv1/relu", "relu", None), ("zero_padding2d_2", "zeropad", None), ("pool1", "maxpool", None)]
    for name, _, n, trans in densenet_blocks():
        for i in range(1, n + 1):
            p = "%s_block%d" % (name, i)
            t += [(p + "_0_bn", "bn", p + "_0_bn"), (p + "_0_relu", "relu", None), (p + "_1_conv", "conv", p + "_1_conv"),
                  (p + "_1_bn", "bn", p + "_1_bn"), (p + "_1_relu", "relu", None), (p + "_2_conv", "conv", p + "_2_conv"),
                  (p + "_concat", "concat", None)]
        if trans:
            t += [(trans + "_bn", "bn", trans + "_bn"), (trans + "_relu", "relu", None),
                  (trans + "_conv", "conv", trans + "_conv"), (trans + "_pool", "avgpool", None)]
    t.append(("bn", "bn", "bn"))
    return t


def densenet_param_specs():
    """[(keras_name, shape, trainable, l2)] of the backbone in Keras weight order."""
    specs = []

    def bn(name, c):
        specs.append((name + "/gamma", (c,), True, False))
        specs.append((name + "/beta", (c,), True, False))
        specs.append((name + "/moving_mean", (c,), False, False))
        specs.append((name + "/moving_variance", (c,), False, False))

    specs.append(("conv1/conv/kernel", (7, 7, 3, 64), True, True))
    bn("conv1/bn", 64)
    for name, c0, n, trans in densenet_blocks():
        c = c0
        for i in range(1, n + 1):
            p = "%s_block%d" % (name, i)
            bn(p + "_0_bn", c)
            specs.append((p + "_1_conv/kernel", (1, 1, c, DN_BOTTLENECK), True, True))
            bn(p + "_1_bn", DN_BOTTLENECK)
            specs.append((p + "_2_conv/kernel", (3, 3, DN_BOTTLENECK, DN_GROWTH), True, True))
            c += DN_GROWTH
        if trans:
            bn(trans + "_bn", c)
            specs.append((trans + "_conv/kernel", (1, 1, c, c // 2), True, True))
    bn("bn", 1024)
    return specs


def densenet_pnames():
    """Weight-name prefixes (the part before the last '/') of the backbone's parameters."""
    return sorted({n.rsplit("/", 1)[0] for n, _, _, _ in densenet_param_specs()})


_rows = ctypes.c_int(0)


def _cld(c):
    return (c + 31) // 32 * 32


class _Consumer:
    """One pre-activation BatchNorm over channels [0, c) of a block's Concatenate buffer: its parameters, statistics and
    operand coefficients [scale | 0 | shift]."""

    def __init__(self, eng, name, c):
        self.e, self.c, self.cld = eng, c, _cld(c)
        self.gamma, self.beta = eng.P(name + "/gamma"), eng.P(name + "/beta")
        self.mm, self.mv = eng.S(name + "/moving_mean"), eng.S(name + "/moving_variance")
        self.coef = torch.zeros(3 * self.cld, device=eng.dev, dtype=torch.float32)
        if eng.train_capable:
            self.ggamma, self.gbeta = eng.G(name + "/gamma"), eng.G(name + "/beta")

    def coeffs(self, blk, training):
        L.spnet_dense_coeffs(self.c, self.cld, L.ptr(self.gamma), L.ptr(self.beta), L.ptr(blk.mean), L.ptr(blk.invstd),
                             L.ptr(blk.bmean), L.ptr(blk.bvar), L.ptr(self.mm), L.ptr(self.mv), L.ptr(self.coef), DN_EPS,
                             DN_MOMENTUM, int(training), L.current_stream())

    def bwd(self, blk, dz, ldz, relu, region):
        """G += gamma*g, u/v += gamma*(sum g, sum g*x^), dgamma / dbeta of this BatchNorm."""
        e, st = self.e, L.current_stream()
        L.spnet_dense_consumer_bwd(L.ptr(dz), ldz, L.ptr(blk.X), blk.Cb, blk.M, self.c, L.ptr(self.coef), self.cld,
                                   L.ptr(blk.mean), L.ptr(blk.invstd), L.ptr(self.gamma), relu, L.ptr(blk.G), blk.Cb,
                                   e.ws_ptr(region), st)
        L.spnet_dense_consumer_fin(e.ws_ptr(region), blk.P, self.c, L.ptr(self.gamma), L.ptr(self.ggamma),
                                   L.ptr(self.gbeta), L.ptr(blk.u), L.ptr(blk.v), st)


class _Block:
    def __init__(self, eng, net, B, h, w, name, c0, n, trans):
        from .engine import BN
        tr = eng.train_capable
        self.e, self.name, self.c0, self.n, self.trans = eng, name, c0, n, trans
        self.B, self.h, self.w = B, h, w
        self.M = B * h * w
        self.Cb = c0 + DN_GROWTH * n
        self.P = int(L.spnet_dense_rows(self.M))
        self.X = eng.new(self.M, self.Cb)
        # shared batch statistics of the concat channels: mean / invstd (normalisation) and mean / unbiased variance
        # (the moving-statistics update), as spnet_bn_finalize_fwd leaves them with momentum 0
        self.mean, self.invstd, self.bmean, self.bvar = (torch.zeros(self.Cb, device=eng.dev) for _ in range(4))
        self.layers = []
        for i in range(1, n + 1):
            p = "%s_block%d" % (name, i)
            c = c0 + DN_GROWTH * (i - 1)
            lay = dict(c=c, cons=_Consumer(eng, p + "_0_bn", c), w1=eng.P(p + "_1_conv/kernel"),
                       bn1=BN(eng, DN_BOTTLENECK, self.M, p + "_1_bn", eps=DN_EPS), w2=eng.P(p + "_2_conv/kernel"))
            if tr:
                lay.update(y1=eng.new(self.M, DN_BOTTLENECK), z1=eng.new(self.M, DN_BOTTLENECK),
                           gw1=eng.G(p + "_1_conv/kernel"), gw2=eng.G(p + "_2_conv/kernel"))
            else:
                lay.update(y1=net.y1_scr[:self.M * DN_BOTTLENECK], z1=net.z1_scr[:self.M * DN_BOTTLENECK])
            self.layers.append(lay)
        if trans:
            self.tcons = _Consumer(eng, trans + "_bn", self.Cb)
            self.tw = eng.P(trans + "_conv/kernel")
            self.ty = eng.new(self.M, self.Cb // 2)
            if tr:
                self.tgw = eng.G(trans + "_conv/kernel")
        if tr:
            self.G = eng.new(self.M, self.Cb)
            self.u, self.v = eng.new(self.Cb), eng.new(self.Cb)

    def input_stats(self, region):
        e = self.e
        L.spnet_dense_colsums_ld(L.ptr(self.X), self.Cb, self.M, self.c0, e.ws_ptr(region), L.current_stream())
        self.finalize_stats(e.ws_ptr(region), self.P, 0, self.c0)

    def finalize_stats(self, part, rows, c0, n):
        net = self.e._densenet
        o = 4 * c0
        L.spnet_bn_finalize_fwd(part, rows, self.M, n, L.ptr(net.ones), L.ptr(net.zeros), self.bmean.data_ptr() + o,
                                self.bvar.data_ptr() + o, self.mean.data_ptr() + o, self.invstd.data_ptr() + o,
                                L.ptr(net.ss_scr), DN_EPS, 0.0, L.current_stream())


class DenseNetBackbone:
    """keras DenseNet121(include_top=False) behind the stem: see the module docstring."""

    def __init__(self, eng, x):
        from .engine import BN, WS_BNP, WS_MISC
        self.e, self.x = eng, x
        eng._densenet = self
        tr = eng.train_capable
        B, H2, W2, _ = x.shape
        self.B, self.H2, self.W2 = B, H2, W2
        self.pnames = [p.split("/")[0] for p in densenet_pnames()]
        self.ones = torch.ones(1024, device=eng.dev)
        self.zeros = torch.zeros(1024, device=eng.dev)
        self.ss_scr = eng.new(2 * 1024)
        # stem
        self.h1, self.w1 = (H2 - 1) // 2 + 1, (W2 - 1) // 2 + 1
        self.h2, self.w2 = (self.h1 - 1) // 2 + 1, (self.w1 - 1) // 2 + 1
        self.M1 = B * self.h1 * self.w1
        self.wc = eng.P("conv1/conv/kernel")
        self.y0 = eng.new(B, self.h1, self.w1, 64)
        self.z0 = eng.new(B, self.h1, self.w1, 64)
        self.zp = eng.new(B, self.h1 + 2, self.w1 + 2, 64)
        self.p1 = eng.new(B, self.h2, self.w2, 64)
        self.bn0 = BN(eng, 64, self.M1, "conv1/bn", eps=DN_EPS)
        self.idx = torch.empty(B * self.h2 * self.w2 * 16, device=eng.dev, dtype=torch.int32) if tr else None
        # blocks
        h, w = self.h2, self.w2
        plan, hw = densenet_blocks(), []
        for _, _, _, trans in plan:
            hw.append((h, w))
            if trans:
                h, w = h // 2, w // 2
        if not tr:      # inference: one scratch for every layer's bottleneck tensors
            mx = max(B * a * b_ for a, b_ in hw) * DN_BOTTLENECK
            self.y1_scr, self.z1_scr = eng.new(mx), eng.new(mx)
        self.blocks = [_Block(eng, self, B, a, b_, name, c0, n, trans) for (name, c0, n, trans), (a, b_) in zip(plan, hw)]
        # GEMM colstats (BN-on-load 1x1 convs: N = 128; growth convs: N = 32) go to WS_BNP: ceil(M/32) rows of 2 x N; the
        # consumers' backward sums and the statistics passes to WS_MISC: spnet_dense_rows(M) rows of 2 x Cb (2 x 64: stem)
        if tr and (max((b.M + 31) // 32 * 2 * DN_BOTTLENECK for b in self.blocks) > WS_BNP[1] or
                   max([b.P * 2 * b.Cb for b in self.blocks] + [int(L.spnet_dense_rows(self.M1)) * 2 * 64]) > WS_MISC[1]):
            raise RuntimeError("BatchNorm partial regions too small for DenseNet121 at batch %d, %dx%d" % (B, H2, W2))
        # the transitions' pooled output before its copy into the next block's buffer (training: the input-gradient
        # buffer, idle during forward)
        self.pool_scr = None if tr else eng.new(max(b.M * b.c0 for b in self.blocks))
        last = self.blocks[-1]
        self.fcons = _Consumer(eng, "bn", last.Cb)
        self.y = eng.new(B, last.h, last.w, last.Cb)
        if tr:
            mxm = max(b.M * b.Cb for b in self.blocks)
            self.dz = eng.new(mxm)                               # data gradient of a consumer's BN+ReLU output
            self.zb = eng.new(mxm)                               # BN+ReLU operand of a consumer's weight gradient
            self.dcol = eng.new(max(b.M for b in self.blocks) * 9 * DN_BOTTLENECK)
            self.dnew = eng.new(max(b.M for b in self.blocks) * DN_GROWTH)
            self.dy1 = eng.new(max(b.M for b in self.blocks) * DN_BOTTLENECK)
            self.din = eng.new(max(b.M * b.c0 for b in self.blocks))
            self.dty = eng.new(max(b.M * b.Cb // 2 for b in self.blocks))
            self.gwc = eng.G("conv1/conv/kernel")
            self.dzp = eng.new(B, self.h1 + 2, self.w1 + 2, 64)
            self.dx = eng.new(*x.shape)

    # ------------------------------------------------------------------ forward
    def fwd(self, training):
        from .engine import ACT_RELU, K_MAJOR, OUT_MAJOR, WS_BNP, WS_MISC, _tile_for
        e, B, st = self.e, self.B, L.current_stream()
        L.spnet_dense_conv7(0, L.ptr(self.x), L.ptr(self.wc), L.ptr(self.y0), B, self.H2, self.W2, None, 0, st)
        if training:
            L.spnet_dense_colsums_ld(L.ptr(self.y0), 64, self.M1, 64, e.ws_ptr(WS_MISC), st)
            self.bn0.finalize(int(L.spnet_dense_rows(self.M1)), region=WS_MISC)
        self.bn0.apply(self.y0, self.z0, ACT_RELU)
        L.spnet_pad_nhwc(L.ptr(self.z0), L.ptr(self.zp), B, self.h1, self.w1, 64, 1, 1, 1, 1, 0, st)
        L.spnet_maxpool3x3s2_valid_fwd(L.ptr(self.zp), L.ptr(self.p1), L.ptr(self.idx) if training else None, B,
                                       self.h1 + 2, self.w1 + 2, 64, st)
        src, src_c = self.p1, 64
        for blk in self.blocks:
            L.spnet_copy_cols(L.ptr(src), src_c, L.ptr(blk.X), blk.Cb, blk.M, src_c, 0, st)
            if training:
                blk.input_stats(WS_MISC)
            for lay in blk.layers:
                c, cons, bn1 = lay["c"], lay["cons"], lay["bn1"]
                cons.coeffs(blk, training)
                e.timed("dense_bnrelu_gemm", 2.0 * blk.M * DN_BOTTLENECK * c, ("bnrelu", blk.M, DN_BOTTLENECK, c),
                        L.spnet_gemm_f32_bnrelu, L.ptr(blk.X), blk.Cb, L.ptr(cons.coef), cons.cld, L.ptr(lay["w1"]),
                        DN_BOTTLENECK, L.ptr(lay["y1"]), DN_BOTTLENECK, blk.M, DN_BOTTLENECK, c, 0,
                        e.ws_ptr(WS_BNP) if training else None, ctypes.addressof(_rows) if training else None, st)
                if training:
                    bn1.finalize(_rows.value)
                bn1.apply(lay["y1"], lay["z1"], ACT_RELU)
                K = 9 * DN_BOTTLENECK
                e.timed("gemm", 2.0 * blk.M * DN_GROWTH * K, ("conv gathered", blk.M, DN_GROWTH, K),
                        L.spnet_conv_gemm_f32, L.ptr(lay["z1"]), DN_BOTTLENECK, L.ptr(lay["w2"]), blk.X.data_ptr() + 4 * c,
                        blk.Cb, B, blk.h, blk.w, DN_BOTTLENECK, DN_GROWTH, 3, 3, 1, 1, None,
                        _tile_for(K_MAJOR, OUT_MAJOR, 1 if training else 0, blk.M, DN_GROWTH, K, 0),
                        e.ws_ptr(WS_BNP) if training else None, ctypes.addressof(_rows) if training else None, st)
                if training:
                    blk.finalize_stats(e.ws_ptr(WS_BNP), _rows.value, c, DN_GROWTH)
            if blk.trans:
                tc = blk.tcons
                tc.coeffs(blk, training)
                e.timed("dense_bnrelu_gemm", 2.0 * blk.M * blk.Cb * blk.Cb // 2, ("bnrelu", blk.M, blk.Cb // 2, blk.Cb),
                        L.spnet_gemm_f32_bnrelu, L.ptr(blk.X), blk.Cb, L.ptr(tc.coef), tc.cld, L.ptr(blk.tw), blk.Cb // 2,
                        L.ptr(blk.ty), blk.Cb // 2, blk.M, blk.Cb // 2, blk.Cb, 0, None, None, st)
                nxt = self.blocks[self.blocks.index(blk) + 1]
                pooled = (self.din if e.train_capable else self.pool_scr)[:nxt.M * nxt.c0]
                L.spnet_avgpool2_fwd(L.ptr(blk.ty), L.ptr(pooled), B, blk.h, blk.w, blk.Cb // 2, st)
                src, src_c = pooled, nxt.c0
        last = self.blocks[-1]
        self.fcons.coeffs(last, training)
        L.spnet_dense_apply_ld(L.ptr(last.X), last.Cb, last.M, last.Cb, L.ptr(self.fcons.coef), self.fcons.cld, 0,
                               L.ptr(self.y), last.Cb, st)

    # ------------------------------------------------------------------ backward
    def bwd(self, g):
        from .engine import ACT_RELU, K_MAJOR, OUT_MAJOR, WS_BNP, WS_GEMM, WS_MISC, _gemm
        e, B, st = self.e, self.B, L.current_stream()
        last = self.blocks[-1]
        for blk in self.blocks:
            blk.G.zero_()
            blk.u.zero_()
            blk.v.zero_()
        self.fcons.bwd(last, g, last.Cb, 0, WS_MISC)
        for bi in range(len(self.blocks) - 1, -1, -1):
            blk = self.blocks[bi]
            M, Cb = blk.M, blk.Cb
            if blk.trans:                  # its transition: the next block's input gradient -> pool -> 1x1 conv
                nxt = self.blocks[bi + 1]
                din = self.din[:nxt.M * nxt.c0]
                dty = self.dty[:M * Cb // 2]
                L.spnet_avgpool2_bwd(L.ptr(din), L.ptr(dty), B, blk.h, blk.w, Cb // 2, st)
                tc = blk.tcons
                dz = self.dz[:M * Cb]
                _gemm(dty, K_MAJOR, Cb // 2, blk.tw, K_MAJOR, Cb // 2, dz, Cb, M, Cb, Cb // 2, e)
                tc.bwd(blk, dz, Cb, 1, WS_MISC)
                zb = self.zb[:M * Cb]
                L.spnet_dense_apply_ld(L.ptr(blk.X), Cb, M, Cb, L.ptr(tc.coef), tc.cld, 1, L.ptr(zb), Cb, st)
                _gemm(zb, OUT_MAJOR, Cb, dty, OUT_MAJOR, Cb // 2, blk.tgw, Cb // 2, Cb, Cb // 2, M, e, region=WS_GEMM)
            for lay in reversed(blk.layers):
                c, cons, bn1 = lay["c"], lay["cons"], lay["bn1"]
                dnew = self.dnew[:M * DN_GROWTH]
                L.spnet_dense_producer_fin(L.ptr(blk.G), Cb, L.ptr(blk.u), L.ptr(blk.v), L.ptr(blk.X), Cb, L.ptr(blk.mean),
                                           L.ptr(blk.invstd), M, c, c + DN_GROWTH, L.ptr(dnew), DN_GROWTH, st)
                K = 9 * DN_BOTTLENECK
                dcol = self.dcol[:M * K]
                _gemm(dnew, K_MAJOR, DN_GROWTH, lay["w2"], K_MAJOR, DN_GROWTH, dcol, K, M, K, DN_GROWTH, e)
                rows = int(L.spnet_grad_bnsums_rows(M, 512 if M * DN_BOTTLENECK <= (4 << 20) else 128))
                dy1 = self.dy1[:M * DN_BOTTLENECK]
                L.spnet_patches_bwd_bnsums(L.ptr(dcol), L.ptr(dy1), B, blk.h, blk.w, DN_BOTTLENECK, 3, 3, 1, 1,
                                           L.ptr(lay["z1"]), L.ptr(lay["y1"]), bn1.mean_ptr, bn1.invstd_ptr, 1,
                                           e.ws_ptr(WS_BNP), rows, st)
                bn1.bwd_from_partials(lay["y1"], dy1, dy1, rows)
                # weight gradient of the 3x3 conv: patch matrix of z1 (into dcol, consumed above) x dnew
                L.spnet_patches(L.ptr(lay["z1"]), L.ptr(dcol), B, blk.h, blk.w, DN_BOTTLENECK, 3, 3, 1, 1, 0, st)
                _gemm(dcol, OUT_MAJOR, K, dnew, OUT_MAJOR, DN_GROWTH, lay["gw2"], DN_GROWTH, K, DN_GROWTH, M, e,
                      region=WS_GEMM)
                # 1x1 conv: data gradient into the consumer's accumulation, weight gradient from relu(BN(x))
                dz = self.dz[:M * c]
                _gemm(dy1, K_MAJOR, DN_BOTTLENECK, lay["w1"], K_MAJOR, DN_BOTTLENECK, dz, c, M, c, DN_BOTTLENECK, e)
                cons.bwd(blk, dz, c, 1, WS_MISC)
                zb = self.zb[:M * c]
                L.spnet_dense_apply_ld(L.ptr(blk.X), Cb, M, c, L.ptr(cons.coef), cons.cld, 1, L.ptr(zb), c, st)
                _gemm(zb, OUT_MAJOR, c, dy1, OUT_MAJOR, DN_BOTTLENECK, lay["gw1"], DN_BOTTLENECK, c, DN_BOTTLENECK, M, e,
                      region=WS_GEMM)
            din = self.din[:M * blk.c0]
            L.spnet_dense_producer_fin(L.ptr(blk.G), Cb, L.ptr(blk.u), L.ptr(blk.v), L.ptr(blk.X), Cb, L.ptr(blk.mean),
                                       L.ptr(blk.invstd), M, 0, blk.c0, L.ptr(din), blk.c0, st)
        # stem: max pool (padded plane) -> crop -> conv1/bn + ReLU -> conv1/conv
        L.spnet_maxpool3x3s2_valid_bwd(L.ptr(self.din), L.ptr(self.idx), L.ptr(self.dzp), B, self.h1 + 2, self.w1 + 2, 64, st)
        L.spnet_pad_nhwc(L.ptr(self.dzp), L.ptr(self.z0), B, self.h1, self.w1, 64, 1, 1, 1, 1, 1, st)
        self.bn0.bwd_full(self.y0, self.z0, self.z0, ACT_RELU)
        L.spnet_dense_conv7(2, L.ptr(self.x), L.ptr(self.z0), L.ptr(self.gwc), B, self.H2, self.W2, e.ws_ptr(WS_GEMM),
                            WS_GEMM[1], st)
        L.spnet_dense_conv7(1, L.ptr(self.z0), L.ptr(self.wc), L.ptr(self.dx), B, self.H2, self.W2, None, 0, st)
        return self.dx
