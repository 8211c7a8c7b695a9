"""Plain float64 references for the small kernels around the backbone (TEST INFRASTRUCTURE): the stem's 3x3 convolutions
and its fused head, SelectiveSigmoid, the cutout / salt-and-pepper painters and the dropout mask.  Every function restates
the operation, not the kernel: no tiling, no summation order, no fused multiply-add.  The torch functions compute in
float64 on the device of their arguments (the cases with millions of pixels are evaluated where the data already is);
tests/test_small_kernels_cpu.py pins them against the oracle (oracle/torch_ref.py, oracle/numpy_ref.py)."""
import numpy as np
import torch
import torch.nn.functional as F


# ----------------------------------------------------------------------------- 3x3 convolutions, NHWC, weights HWIO
def conv3x3_same(x, w):
    """y[b,h,v,co] = sum_{kh,kw,ci} x[b,h+kh-1,v+kw-1,ci] * w[kh,kw,ci,co], zero outside the image (stride 1, 'same')."""
    x, w = x.double(), w.double()
    B, H, W, cin = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    y = torch.zeros(B, H, W, w.shape[3], dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            for ci in range(cin):
                y += xp[:, kh:kh + H, kw:kw + W, ci:ci + 1] * w[kh, kw, ci]
    return y


def conv3x3_same_dgrad(dy, w):
    """dx[b,h,v,ci] = sum_{kh,kw,co} dy[b,h+1-kh,v+1-kw,co] * w[kh,kw,ci,co]: the same convolution with the taps mirrored
    and the channel axes exchanged."""
    return conv3x3_same(dy, w.flip(0, 1).permute(0, 1, 3, 2))


def avgpool2(x):
    """AveragePooling2D(2) of [B,H,W,C]: an odd last row / column is dropped."""
    x = x.double()
    B, H, W, C = x.shape
    oh, ow = H // 2, W // 2
    return x[:, :2 * oh, :2 * ow].reshape(B, oh, 2, ow, 2, C).sum((2, 4)) * 0.25


# ----------------------------------------------------------------------------- stem head (conv2d_1 + both poolings)
def stem_head_fwd(x, w):
    """x [B,H,W], w [3,3,1,3] -> p1 [B,H/2,W/2,3] = avgpool2(conv 'same'(x, w)), px [B,H/2,W/2] = avgpool2(x)."""
    x4 = x.double()[..., None]
    return avgpool2(conv3x3_same(x4, w)), avgpool2(x4)[..., 0]


def stem_head_wgrad(x, dp1):
    """dw [3,3,1,3] of conv2d_1 from the gradient dp1 of the POOLED output: the pooling backward hands a quarter of dp1 to
    each of the four pixels of a cell (none to a dropped last row / column), the convolution backward correlates that
    with the zero-padded frame."""
    x, dp1 = x.double(), dp1.double()
    B, H, W = x.shape
    oh, ow = H // 2, W // 2
    g = torch.zeros(B, H, W, 3, dtype=torch.float64, device=x.device)
    g[:, :2 * oh, :2 * ow] = 0.25 * dp1.repeat_interleave(2, 1).repeat_interleave(2, 2)
    xp = F.pad(x, (1, 1, 1, 1))
    dw = torch.zeros(3, 3, 1, 3, dtype=torch.float64, device=x.device)
    for kh in range(3):
        for kw in range(3):
            dw[kh, kw, 0] = (xp[:, kh:kh + H, kw:kw + W, None] * g).sum((0, 1, 2))
    return dw


# ----------------------------------------------------------------------------- SelectiveSigmoid
def selective_sigmoid_fwd(y, start, step):
    """y[:, start::step] = sigmoid(.), every other column unchanged (float64 numpy)."""
    out = np.array(y, np.float64, copy=True)
    out[:, start::step] = 1.0 / (1.0 + np.exp(-out[:, start::step]))
    return out


def selective_sigmoid_bwd(s, g, start, step):
    """g[:, start::step] *= s (1 - s), s the post-sigmoid output; every other column of g unchanged."""
    s = np.asarray(s, np.float64)
    out = np.array(g, np.float64, copy=True)
    out[:, start::step] *= s[:, start::step] * (1.0 - s[:, start::step])
    return out


# ----------------------------------------------------------------------------- augmentation painters
def paint_rects(img, rects):
    """cutout: img[r0:r1, c0:c1] = value for each (r0, r1, c0, c1, value) in order, so later rectangles win.  In place."""
    for r0, r1, c0, c1, val in rects:
        img[int(r0):int(r1), int(c0):int(c1)] = val
    return img


def paint_saltpepper(img, salt_rows, salt_cols, pepper_rows, pepper_cols, salt, pepper):
    """The reference's two fancy-index assignments: every salt point first, then every pepper point (pepper wins where
    both fall on a pixel).  In place."""
    img[np.asarray(salt_rows, np.int64), np.asarray(salt_cols, np.int64)] = salt
    img[np.asarray(pepper_rows, np.int64), np.asarray(pepper_cols, np.int64)] = pepper
    return img


# ----------------------------------------------------------------------------- dropout
def dropout_threshold(rate):
    """rate (held as float32) * 2^32, truncated, capped at 2^32 - 1."""
    return min(int(float(np.float32(rate)) * 4294967296.0), 4294967295)


def dropout_hash(n, seed):
    """hash(i * 0x9e3779b9 + seed) for i in [0, n), everything in uint32 arithmetic."""
    m = np.uint64(0xFFFFFFFF)
    h = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B9) + np.uint64(seed & 0xFFFFFFFF)) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & m
    h ^= h >> np.uint64(16)
    return h


def dropout_keep(n, seed, rate):
    """Element i survives iff hash(i * 0x9e3779b9 + seed) >= rate * 2^32."""
    return dropout_hash(n, seed) >= np.uint64(dropout_threshold(rate))


def dropout_scale(rate):
    """1 / (1 - rate) in float32 arithmetic: what survivors are multiplied by."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))
