"""numpy / int64 restatement of csrc/overlay.hip: the outline rule, the blit rule and the paint order, from the packed
arrays of an spnet_amd.overlay.OverlayPlan (frame_start, cmd, verts, masks) -- what the kernel is handed.

Outline (per pixel, centre C = (16 x + center, 16 y + center) in 1/16 pixel; for every edge P -> Q of the closed polygon,
e = Q - P, v = C - P, t = v.e, L2 = e.e, all int64):
    inside the edge's box grown by r, and
    (t <= 0 and v.v <= r^2)  or  (t >= L2 and |C - Q|^2 <= r^2)  or  (t in between and (v x e)^2 <= r^2 * L2)
    -> the pixel takes the colour (last writer wins).
Blit (per pixel under the mask, per channel):  t = dst * (255 - m) + ink * m + 128;  out = ((t >> 8) + t) >> 8.
Commands run in list order; a command whose box (clipped to the frame by the plan) is empty paints nothing; nothing outside
the box is touched."""
import numpy as np

from spnet_amd import overlay as O


def outline_cover(q, H, W, center=O.CENTER, r=O.RADIUS, box=None):
    """bool [H,W]: pixels the rule paints for the closed polygon q (int [n,2], 1/16 pixel)."""
    q = np.asarray(q, np.int64)
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else box
    cover = np.zeros((H, W), bool)
    if x1 <= x0 or y1 <= y0:
        return cover
    cx = (np.arange(x0, x1, dtype=np.int64) * O.SUBPIXEL + center)[None, :]
    cy = (np.arange(y0, y1, dtype=np.int64) * O.SUBPIXEL + center)[:, None]
    sub = np.zeros((y1 - y0, x1 - x0), bool)
    r2 = np.int64(r) * r
    for k in range(len(q)):
        px, py = q[k]
        qx, qy = q[(k + 1) % len(q)]
        ex, ey = qx - px, qy - py
        vx, vy = cx - px, cy - py
        inbox = (cx >= min(px, qx) - r) & (cx <= max(px, qx) + r) & (cy >= min(py, qy) - r) & (cy <= max(py, qy) + r)
        t = vx * ex + vy * ey
        L2 = ex * ex + ey * ey
        wx, wy = cx - qx, cy - qy
        cross = vx * ey - vy * ex
        hit = np.where(t <= 0, vx * vx + vy * vy <= r2,
                       np.where(t >= L2, wx * wx + wy * wy <= r2, cross * cross <= r2 * L2))
        sub |= inbox & hit
    cover[y0:y1, x0:x1] = sub
    return cover


def blend(dst, ink, m):
    t = dst.astype(np.int64) * (255 - m) + np.int64(ink) * m + 128
    return (((t >> 8) + t) >> 8).astype(np.uint8)


def draw(frames, frame_start, cmd, verts, masks, center=O.CENTER, r=O.RADIUS):
    """frames uint8 [N,H,W] | [N,H,W,3] -> uint8 [N,H,W,3] with every command painted, in order."""
    frames = np.asarray(frames)
    out = np.repeat(frames[..., None], 3, axis=-1) if frames.ndim == 3 else frames.copy()
    N, H, W = out.shape[:3]
    for n in range(N):
        for c in range(int(frame_start[n]), int(frame_start[n + 1])):
            kind, rgb, x0, y0, x1, y1, data, mx, my, mw, mh = (int(v) for v in cmd[c][:11])
            if x1 <= x0 or y1 <= y0:
                continue
            assert 0 <= x0 and 0 <= y0 and x1 <= W and y1 <= H
            ink = (rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255)
            if kind == O.KIND_OUTLINE:
                cover = outline_cover(verts[data:data + O.VERTS], H, W, center, r, (x0, y0, x1, y1))
                out[n][cover] = ink
            else:
                mask = np.asarray(masks[data:data + mw * mh], np.int64).reshape(mh, mw)
                ax0, ay0, ax1, ay1 = max(x0, mx), max(y0, my), min(x1, mx + mw), min(y1, my + mh)
                if ax1 <= ax0 or ay1 <= ay0:
                    continue
                m = mask[ay0 - my:ay1 - my, ax0 - mx:ax1 - mx]
                for ch in range(3):
                    out[n, ay0:ay1, ax0:ax1, ch] = blend(out[n, ay0:ay1, ax0:ax1, ch], ink[ch], m)
    return out


def draw_plan(frames, plan, **kw):
    return draw(frames, plan.frame_start, plan.cmd, plan.verts, plan.masks, **kw)


# ----------------------------------------------------------------------------- the fixed set the convention was chosen on
def seeded_ellipses(count=40, seed=20240, H=384, W=512):
    """(cx, cy, a, b, angle) of `count` ellipses as cleanup_antinode_vars hands them on: integer geometry, angle in (0,180]."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        out.append((int(rng.randint(20, W - 20)), int(rng.randint(20, H - 20)), int(rng.randint(3, 120)),
                    int(rng.randint(2, 80)), float(rng.uniform(0.0, 180.0)) or 180.0))
    return out


def pillow_outline(cx, cy, a, b, angle, H, W):
    """bool [H,W]: what utils.draw_ellipse(thickness=3) paints on an empty frame."""
    from PIL import Image
    from spnet_amd import utils
    img = Image.new("L", (W, H), 0)
    utils.draw_ellipse(img, [cx, cy], [a, b], angle, color=(255,), thickness=3)
    return np.asarray(img) != 0


def near(mask, d=2):
    """bool: pixels within (Euclidean) distance d of a set pixel."""
    H, W = mask.shape
    p = np.zeros((H + 2 * d, W + 2 * d), bool)
    p[d:d + H, d:d + W] = mask
    out = np.zeros_like(mask)
    for dy in range(2 * d + 1):
        for dx in range(2 * d + 1):
            if (dy - d) ** 2 + (dx - d) ** 2 > d * d:
                continue
            out |= p[dy:dy + H, dx:dx + W]
    return out


def compare_with_pillow(center, r, ellipses=None, H=384, W=512):
    """Over the set: (differing pixels, Pillow's outline pixels, differing pixels farther than 2 px from Pillow's outline)."""
    from spnet_amd import utils
    diff = total = far = 0
    for cx, cy, a, b, angle in (seeded_ellipses() if ellipses is None else ellipses):
        ref = pillow_outline(cx, cy, a, b, angle, H, W)
        q = O.quantise_vertices(utils.ellipse_polygon([cx, cy], [a, b], angle, n=O.VERTS))
        got = outline_cover(q, H, W, center, r, O.outline_box(q, H, W, center, r))
        d = ref != got
        diff += int(d.sum())
        total += int(ref.sum())
        far += int((d & ~near(ref, 2)).sum())
    return diff, total, far
