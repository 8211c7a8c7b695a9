"""Independent fp64 restatement of keras.applications.densenet.DenseNet121(include_top=False) (Keras 2.1.3) behind the
SPNet stem, for the DenseNet parity tests.  Written from the Keras layer recipe, not from spnet_amd: the stem, the head
and the loss come from oracle.torch_ref."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import torch_ref as T

EPS = 1.001e-5
MOM = 0.99
BLOCKS = (6, 12, 24, 16)


def layer_list():
    """(name, kind) of the Keras layers in creation order (no final ReLU in Keras 2.1.3)."""
    out = [("zero_padding2d_1", "zeropad"), ("conv1/conv", "conv"), ("conv1/bn", "bn"), ("conv1/relu", "relu"),
           ("zero_padding2d_2", "zeropad"), ("pool1", "maxpool")]
    for b, n in enumerate(BLOCKS):
        for i in range(n):
            p = "conv%d_block%d" % (b + 2, i + 1)
            out += [(p + "_0_bn", "bn"), (p + "_0_relu", "relu"), (p + "_1_conv", "conv"), (p + "_1_bn", "bn"),
                    (p + "_1_relu", "relu"), (p + "_2_conv", "conv"), (p + "_concat", "concat")]
        if b < 3:
            q = "pool%d" % (b + 2)
            out += [(q + "_bn", "bn"), (q + "_relu", "relu"), (q + "_conv", "conv"), (q + "_pool", "avgpool")]
    out.append(("bn", "bn"))
    return out


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


def conv(x, w, stride=1, pad=0):
    return _nhwc(F.conv2d(_nchw(x), w.permute(3, 2, 0, 1), stride=stride, padding=pad))


def bn(P, name, x, training):
    C = x.shape[-1]
    g, b = P[name + "/gamma"], P[name + "/beta"]
    mm, mv = P[name + "/moving_mean"], P[name + "/moving_variance"]
    if training:
        flat = x.reshape(-1, C)
        mu, var = flat.mean(0), flat.var(0, unbiased=False)
        n = flat.shape[0]
        with torch.no_grad():
            mm.mul_(MOM).add_((1 - MOM) * mu.detach())
            mv.mul_(MOM).add_((1 - MOM) * var.detach() * (n / max(n - 1, 1)))
        return (x - mu) / torch.sqrt(var + EPS) * g + b
    return (x - mm) / torch.sqrt(mv + EPS) * g + b


def maxpool_pad1(x, decisions=None):
    """ZeroPadding2D(1) + MaxPooling2D(3, 2, valid); decisions (T.Decisions): the window arg-max taps to take."""
    xp = _nhwc(F.pad(_nchw(x), (1, 1, 1, 1)))
    if decisions is None:
        return _nhwc(F.max_pool2d(_nchw(xp), 3, 2))
    return T.maxpool3x3s2_valid(xp, decisions)


def _relu(x, decisions):
    return torch.relu(x) if decisions is None else decisions.act(x, 0.0)


def backbone(P, x, training, decisions=None):
    """decisions (T.Decisions, or None for the model's own): the ReLU masks in application order (conv1/relu, then
    _0_relu, _1_relu of every layer and the transitions' relu) and the taps of pool1."""
    t = F.pad(_nchw(x), (3, 3, 3, 3))
    t = _nhwc(F.conv2d(t, P["conv1/conv/kernel"].permute(3, 2, 0, 1), stride=2))
    t = _relu(bn(P, "conv1/bn", t, training), decisions)
    t = maxpool_pad1(t, decisions)
    for b, n in enumerate(BLOCKS):
        for i in range(n):
            p = "conv%d_block%d" % (b + 2, i + 1)
            u = _relu(bn(P, p + "_0_bn", t, training), decisions)
            u = conv(u, P[p + "_1_conv/kernel"])
            u = _relu(bn(P, p + "_1_bn", u, training), decisions)
            u = conv(u, P[p + "_2_conv/kernel"], pad=1)
            t = torch.cat([t, u], dim=-1)
        if b < 3:
            q = "pool%d" % (b + 2)
            t = _relu(bn(P, q + "_bn", t, training), decisions)
            t = conv(t, P[q + "_conv/kernel"])
            t = _nhwc(F.avg_pool2d(_nchw(t), 2))
    return bn(P, "bn", t, training)


def forward(P, X, training=False, drop_mask=None, decisions=None):
    x = T.stem(P, X, training, drop_mask, decisions=decisions)
    x = backbone(P, x, training, decisions)
    return x.reshape(x.shape[0], -1) @ P["FinalOutput/kernel"] + P["FinalOutput/bias"]


def grads(P, X, Y, drop_mask, dtype=torch.float64, decisions=None):
    """(data loss, {trainable name: grad}, y_pred, P with updated moving statistics) in `dtype` (fp64 by default),
    evaluated on the given discrete decisions (T.Decisions) if any."""
    Q = {k: v.to(dtype).clone() for k, v in P.items()}
    for k, v in Q.items():
        if not (k.endswith("moving_mean") or k.endswith("moving_variance")):
            v.requires_grad_(True)
    y = forward(Q, X.to(dtype), training=True, drop_mask=drop_mask.to(dtype), decisions=decisions)
    loss = T.custom_loss(Y.to(dtype), y)
    loss.backward()
    g = {k: v.grad for k, v in Q.items() if v.grad is not None}
    return float(loss.detach()), g, y.detach(), {k: v.detach() for k, v in Q.items()}


def random_params(names_shapes, seed):
    """Glorot-uniform kernels, randomised BatchNorm state (every term exercised)."""
    gen = torch.Generator().manual_seed(seed)
    P = {}
    for name, shape in names_shapes:
        if name.endswith("/gamma"):
            P[name] = 0.5 + torch.rand(shape, generator=gen)
        elif name.endswith("/beta") or name.endswith("/moving_mean") or name.endswith("/bias"):
            P[name] = 0.2 * torch.randn(shape, generator=gen)
        elif name.endswith("/moving_variance"):
            P[name] = 0.5 + torch.rand(shape, generator=gen)
        else:
            rf = int(np.prod(shape[:-2])) if len(shape) == 4 else 1
            fi, fo = shape[-2] * rf, shape[-1] * rf
            lim = float(np.sqrt(6.0 / (fi + fo)))
            P[name] = (torch.rand(shape, generator=gen) * 2 - 1) * lim
    return P
