"""The warp chain as three separate steps (TEST INFRASTRUCTURE): flip -> rotate -> translate composed from the numpy
restatements of oracle/warp_ref.py, one image and one metadata list at a time, as augment_one_file chains flip_image,
rotate_image and translate_image (flip code -2 and angle 0 return their input untouched).  The batched single-gather
kernel, its numpy restatement and the vectorised metadata / target code of spnet_amd.augmentation are checked against
this."""
from operator import itemgetter

import numpy as np

from oracle import warp_ref as WR


def shift(img, xt, yt):
    """dst(x, y) = img(x - xt, y - yt), zero where that lies outside: translate_image's warpAffine of [[1,0,xt],[0,1,yt]]."""
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    if abs(xt) >= W or abs(yt) >= H:
        return out
    out[max(yt, 0):H + min(yt, 0), max(xt, 0):W + min(xt, 0)] = img[max(-yt, 0):H + min(-yt, 0), max(-xt, 0):W + min(-xt, 0)]
    return out


def warp_image(img, flip, angle, xt, yt):
    """uint8 [H,W] or [H,W,C] through the three steps."""
    x = img[..., None] if img.ndim == 2 else img
    H, W = x.shape[:2]
    if flip != -2:
        x = WR.flip(x, flip)
    if angle != 0:
        x = WR.warp_affine_cv2(x, WR.rotation_matrix((W / 2, H / 2), angle))
    x = shift(np.ascontiguousarray(x), xt, yt)
    return x[..., 0] if img.ndim == 2 else x


def warp_meta(md, flip, angle, xt, yt, W, H):
    md = [list(r) for r in md]
    if flip != -2:
        md = WR.flip_meta(md, flip, W, H)
    if angle != 0:
        md = WR.rotate_meta(md, angle, W, H)
    return [[cx + xt, cy + yt, a, b, ang, rings] for cx, cy, a, b, ang, rings in md]


def targets(md, pred_grid=(6, 6, 2)):
    """The per-sample target path for in-memory rows: parse_meta_file's row processing, true_to_pred_grid, norm_Y."""
    from spnet_amd import config as cf
    from spnet_amd import utils
    out = []
    for cx, cy, a, b, angle, rings in md:
        angle = float(angle)
        if b > a:
            a, b, angle = b, a, angle + 90
        if rings > 0.0:
            t = 2 * np.deg2rad(angle)
            out.append([cx, cy, a, b, np.cos(t), np.sin(t), 0, rings])
    rows = np.array(sorted(out, key=itemgetter(0, 1)))
    pred_shape = np.array([pred_grid[0], pred_grid[1], pred_grid[2], cf.vars_per_pred], dtype=int)
    Y = np.zeros([1, int(np.prod(pred_shape))], dtype=cf.dtype)
    Y[0, :] = utils.true_to_pred_grid(rows, pred_shape).flatten()
    return utils.norm_Y(Y)[0]
