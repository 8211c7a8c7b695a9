"""The prediction overlays of utils.show_pred_ellipses as a host plan + one HIP launch per chunk (csrc/overlay.hip).

plan_overlays() is the loop of show_pred_ellipses without the drawing: the same selection (cleanup_antinode_vars, the
noobj / rings / a / b gate), the same order (predictor ascending, "True" before "Pred", each ellipse followed by its
label, the file name last) and the same CSV rows, turned into two kinds of command per frame:

  outline   the 72 vertices of utils.ellipse_polygon, float64 on the host, rounded to 1/16 pixel (int32), and a colour.
            The device paints pixel (x, y), centre C = (16 x + CENTER, 16 y + CENTER) in 1/16 pixel, if for one of the 72
            edges P -> Q (e = Q - P, v = C - P, t = v.e, L2 = e.e):
              C lies in the edge's box grown by RADIUS (a necessary condition of the three below), and
              t <= 0 and |v|^2 <= RADIUS^2,  or  t >= L2 and |C - Q|^2 <= RADIUS^2,  or  (v x e)^2 <= RADIUS^2 * L2
            -- a polyline of width 2 RADIUS with round joints, in integers only: no sine, cosine, division or square root
            on the device, so the numpy restatement (tests/helpers/overlay_ref.py) and the kernel agree bit for bit.
  blit      an 8-bit coverage mask from the font object ImageDraw.text uses (getmask2(text, "L", anchor="la")), its
            top-left pixel and an ink: out = muldiv255(dst * (255 - m) + ink * m) per channel, Pillow's paste of an "L"
            mask.  Equal strings share one mask in the blob.

Outlines replace (last writer wins), masks blend, both in command order; everything is clipped to the frame.  CENTER and
RADIUS were chosen on the CPU against ImageDraw.line(width=3, joint="curve") (DESIGN.md 5d has the table).

Nothing here imports torch or the HIP library until draw_overlays_device is called.
"""
import os

import numpy as np
from PIL import Image, ImageDraw

from . import config as cf
from . import utils

SUBPIXEL = 16               # vertex and pixel-centre coordinates are in 1/16 pixel
CENTER = 8                  # the centre of pixel (x, y) is (x + 1/2, y + 1/2) in the polygon's coordinates
RADIUS = 24                 # half the line width, 1.5 pixels
VERTS = 72                  # utils.ellipse_polygon's n
CMD_WORDS = 12              # int32 words per command (layout below)
KIND_OUTLINE, KIND_BLIT = 0, 1
# cmd[c] = kind, rgb (r | g << 8 | b << 16), box x0, y0, x1, y1 (pixels, x1 / y1 exclusive, clipped to the frame; empty:
#          x1 <= x0), data (outline: index of its first vertex in verts; blit: byte offset of its mask in the blob),
#          blit only: mask x, y (top-left pixel, may be negative), mask width, height; 0
# An edge longer than EDGE_LIMIT in x or y (semi-axes beyond about 5,800 pixels) would take the 64-bit products of the
# rule past 2^55; such an outline keeps its place in the list with an empty box (it is not painted).
EDGE_LIMIT = 1 << 13
COORD_LIMIT = 1 << 30


class OverlayPlan:
    """What plan_overlays returns.  csv [n]: the rows of frame j as one string.  frames [n]: the commands of frame j in
    paint order as tuples ("outline", rgb, vertices float64 [72,2]) | ("text", rgb, (x, y), string) -- the calls the host
    path makes.  frame_start int32 [n+1], cmd int32 [C,12], verts int32 [V,2], masks uint8 [B]: the same list packed for
    the kernel; commands of frame j are cmd[frame_start[j]:frame_start[j+1]].  sizes [n]: (H, W) of frame j."""

    def __init__(self, csv, frames, frame_start, cmd, verts, masks, sizes):
        self.csv, self.frames, self.frame_start, self.cmd, self.verts, self.masks, self.sizes = \
            csv, frames, frame_start, cmd, verts, masks, sizes

    def __len__(self):
        return len(self.csv)

    def chunk(self, lo, hi):
        """The plan of frames lo .. hi-1 alone: its own commands and vertices; the mask blob is shared whole."""
        s = self.frame_start
        cmd = self.cmd[s[lo]:s[hi]].copy()
        outl = cmd[:, 0] == KIND_OUTLINE
        v0 = int(cmd[outl, 6].min(initial=0))
        v1 = int(cmd[outl, 6].max(initial=-VERTS)) + VERTS
        cmd[outl, 6] -= v0
        return OverlayPlan(self.csv[lo:hi], self.frames[lo:hi], (s[lo:hi + 1] - s[lo]).astype(np.int32), cmd,
                           self.verts[v0:max(v1, v0)], self.masks, self.sizes[lo:hi])


def _rgb_word(rgb):
    return int(rgb[0]) | int(rgb[1]) << 8 | int(rgb[2]) << 16


def quantise_vertices(pts):
    """float64 [72,2] pixel coordinates -> int32 1/16 pixel, round half to even as numpy rounds."""
    q = np.rint(np.asarray(pts, np.float64) * SUBPIXEL)
    return np.clip(q, -COORD_LIMIT, COORD_LIMIT).astype(np.int32)


def outline_box(q, H, W, center=CENTER, radius=RADIUS):
    """Pixels whose centre can lie within `radius` of the closed polygon q (int 1/16 pixel), clipped to the frame."""
    q = q.astype(np.int64)
    e = np.abs(np.roll(q, -1, axis=0) - q)
    if e.max(initial=0) >= EDGE_LIMIT or np.abs(q).max(initial=0) >= COORD_LIMIT:
        return 0, 0, 0, 0
    x0 = -((-(int(q[:, 0].min()) - radius - center)) // SUBPIXEL)
    y0 = -((-(int(q[:, 1].min()) - radius - center)) // SUBPIXEL)
    x1 = (int(q[:, 0].max()) + radius - center) // SUBPIXEL + 1
    y1 = (int(q[:, 1].max()) + radius - center) // SUBPIXEL + 1
    return max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)


_RENDERED = {}              # string -> (coverage uint8 [h*w], offset x, y, w, h): ring counts recur from plan to plan


def render_mask(text):
    """The mask ImageDraw.text pastes for `text` with the default font at an integer position, and its offset."""
    hit = _RENDERED.get(text)
    if hit is None:
        font = ImageDraw.Draw(Image.new("RGB", (1, 1))).getfont()
        try:
            mask, (ox, oy) = font.getmask2(text, "L", anchor="la")
        except AttributeError:                      # a bitmap font (Pillow without FreeType): as ImageDraw.text falls back
            mask, ox, oy = font.getmask(text, "L"), 0, 0
        w, h = mask.size
        data = np.frombuffer(bytes(mask), np.uint8) if w * h else np.zeros(0, np.uint8)
        assert data.size == w * h
        if len(_RENDERED) >= 8192:                  # file names are one per frame: do not keep them for ever
            _RENDERED.clear()
        hit = _RENDERED[text] = (data, int(ox), int(oy), int(w), int(h))
    return hit


class _Masks:
    """The masks of one plan packed into one blob, equal strings once."""

    def __init__(self):
        self.known = {}
        self.parts = []
        self.used = 0

    def get(self, text):
        hit = self.known.get(text)
        if hit is None:
            data, ox, oy, w, h = render_mask(text)
            hit = self.known[text] = (self.used, ox, oy, w, h)
            self.parts.append(data)
            self.used += w * h
        return hit

    def blob(self):
        return np.concatenate(self.parts + [np.zeros(1, np.uint8)])         # never empty: the kernel is handed a pointer


def pack_commands(frames, sizes, csv=None):
    """frames [n]: per frame the commands in paint order, ("outline", rgb, vertices float [72,2] in pixels) | ("text", rgb,
    (x, y), string) with integer x, y as ImageDraw.text takes them; sizes [n]: (H, W).  The OverlayPlan of them."""
    masks = _Masks()
    frame_start, cmd, verts = [0], [], []
    for out, (H, W) in zip(frames, sizes):
        for c in out:
            if c[0] == "outline":
                q = quantise_vertices(c[2])
                if q.shape != (VERTS, 2):
                    raise ValueError("pack_commands: an outline has %d x 2 vertices, got %s" % (VERTS, q.shape))
                cmd.append((KIND_OUTLINE, _rgb_word(c[1])) + outline_box(q, H, W) + (len(verts) * VERTS, 0, 0, 0, 0, 0))
                verts.append(q)
            else:
                off, ox, oy, w, h = masks.get(c[3])
                x, y = int(c[2][0]) + ox, int(c[2][1]) + oy
                cmd.append((KIND_BLIT, _rgb_word(c[1]), max(x, 0), max(y, 0), min(x + w, W), min(y + h, H), off, x, y, w, h, 0))
        frame_start.append(len(cmd))
    return OverlayPlan(list(csv) if csv is not None else [''] * len(frames), list(frames), np.asarray(frame_start, np.int32),
                       np.asarray(cmd, np.int32).reshape(-1, CMD_WORDS),
                       np.concatenate(verts).astype(np.int32) if verts else np.zeros((0, 2), np.int32),
                       masks.blob(), [tuple(int(v) for v in s) for s in sizes])


def plan_overlays(Yt, Yp, file_list, show_true=True, size=None, num_draw=None, with_csv=True):
    """The overlays of frames 0 .. num_draw-1 (default: all of Yt / file_list) as an OverlayPlan.  size: (H, W) of every
    frame, or one (H, W) per frame; default utils.orig_img_dims.  Yt / Yp: de-normalised grids, as show_pred_ellipses
    takes them.  with_csv=False is show_pred_ellipses(out_csv=None): no rows are formed."""
    m = Yt.shape[0]
    n = min(m if num_draw is None else num_draw, m, len(file_list))
    if size is None:
        size = (utils.orig_img_dims[1], utils.orig_img_dims[0])
    sizes = [tuple(int(v) for v in size)] * n if np.ndim(size) == 1 else [tuple(int(v) for v in s) for s in size[:n]]
    if len(sizes) != n:
        raise ValueError("plan_overlays: %d sizes for %d frames" % (len(sizes), n))
    vpp = cf.vars_per_pred
    n_pred = int(Yt[0].size / vpp) if m else 0
    todraw = ([('True', Yt, tuple(cf.truecolor[::-1]))] if show_true else []) + [('Pred', Yp, tuple(cf.predcolor[::-1]))]
    csv, frames = [], []
    for j in range(n):
        base = os.path.basename(file_list[j])
        rows, out = '', []
        for an in range(n_pred):
            for name, Y, rgb in todraw:
                cx, cy, a, b, angle, noobj, rings = utils.cleanup_antinode_vars(Y[j, an * vpp:(an + 1) * vpp])
                if noobj == 0 and rings > 0 and a >= 0 and b >= 0:
                    out.append(("outline", rgb, utils.ellipse_polygon([cx, cy], [a, b], angle, n=VERTS)))
                    out.append(("text", rgb, (cx - 10, cy - 8 + (0 if name == 'True' else 14)), "{: >3.1f}".format(rings)))
                    if name == 'Pred' and with_csv:
                        rows += "{},{},{},{},{},{},{}\n".format(cx, cy, base, rings, a, b, angle)
        if with_csv and rows == '':
            rows = '0,0,' + base + ',0,0,0,0\n'
        out.append(("text", (255, 255, 255), (5, utils.orig_img_dims[1] - 14), base))
        csv.append(rows)
        frames.append(out)
    return pack_commands(frames, sizes, csv)


def draw_overlays_device(frames, plan):
    """frames: uint8 device tensor [N,H,W] | [N,H,W,1] (grey, replicated to three channels) or [N,H,W,3]; plan: the
    OverlayPlan of exactly these N frames (plan.chunk(lo, hi) of a longer one).  Returns a new uint8 [N,H,W,3] on the
    same device with every command painted, in ONE launch on the current stream.  No CPU fallback."""
    import torch
    from . import _lib as L
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or not frames.is_cuda:
        raise TypeError("draw_overlays_device expects a uint8 device tensor")
    if frames.dim() == 4 and frames.shape[-1] == 1:
        frames = frames[..., 0]
    if frames.dim() == 3:
        channels = 1
    elif frames.dim() == 4 and frames.shape[-1] == 3:
        channels = 3
    else:
        raise ValueError("draw_overlays_device expects frames [N,H,W], [N,H,W,1] or [N,H,W,3], got %s" % (tuple(frames.shape),))
    frames = frames.contiguous()
    N, H, W = (int(v) for v in frames.shape[:3])
    if len(plan) != N or any(s != (H, W) for s in plan.sizes):
        raise ValueError("draw_overlays_device: the plan is for %d frames of sizes %s, the tensor is %d x %d x %d"
                         % (len(plan), sorted(set(plan.sizes)), N, H, W))
    dev = frames.device
    out = torch.empty((N, H, W, 3), dtype=torch.uint8, device=dev)
    if N == 0:
        return out
    # one upload for the four arrays: int32 first (frame_start, cmd, verts), then the mask bytes
    nb = 4 * (plan.frame_start.size + plan.cmd.size + plan.verts.size)
    host = np.empty(nb + plan.masks.size, np.uint8)
    o0 = 4 * plan.frame_start.size
    o1 = o0 + 4 * plan.cmd.size
    host[:o0] = np.ascontiguousarray(plan.frame_start, np.int32).view(np.uint8)
    host[o0:o1] = np.ascontiguousarray(plan.cmd, np.int32).reshape(-1).view(np.uint8)
    host[o1:nb] = np.ascontiguousarray(plan.verts, np.int32).reshape(-1).view(np.uint8)
    host[nb:] = plan.masks
    blob = torch.from_numpy(host).to(dev)
    p = blob.data_ptr()
    with torch.cuda.device(dev):
        L.spnet_draw_overlays(frames.data_ptr(), N, H, W, channels, p, p + o0, int(plan.cmd.shape[0]), p + o1,
                              int(plan.verts.shape[0]), p + nb, int(plan.masks.size), out.data_ptr(), L.current_stream())
    return out
