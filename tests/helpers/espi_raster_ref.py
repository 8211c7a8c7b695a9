"""The fake-ESPI device generator's specification in numpy (TEST INFRASTRUCTURE): what spnet_amd/csrc/espi.hip computes,
restated from its comment block and arithmetic -- the analytic wave bands, the ringed antinodes and the counter-based sensor
model -- in float64, with the distance by which every pixel's comparisons were decided (`margin`), so that the device canvas
can be required to EQUAL the reference wherever float32 cannot legitimately decide otherwise.

  canvas_ref   float64, every outline of every antinode tested (no window): the specification
  canvas_f32   the same formulas in float32, in the kernel's order of operations, with the kernel's four-outline window
               (or without): what float32 may do to the specification, measured on the CPU
  sensor_ref   the three chained hashes in uint32, u1 / u2 as the kernel forms them, Box-Muller in float64
  ring_runs    the colour runs along an antinode's major axis: the labelled ring count, read back from the pixels
  CASES        crafted launches (small frames chosen for the indexing, parameters chosen for the branches)
"""
import numpy as np

MAX_NODES, NODE_STRIDE, WAVE_STRIDE = 7, 8, 5        # cx, cy, a, b, angle_deg, rings, start, valid | amp, wl, thick, slope, spacing
GREY, BLACK, RING = 128, 0, 138
NEAR_TIE = 1e-3                 # pixels: a comparison decided by less than this may go either way in float32
NEAR_TIE_SHARE = 0.0005         # at most 0.05 % of the pixels may be that close to a threshold
DEG = 0.017453292519943295


# --------------------------------------------------------------------------------------------------------------- raster
def _frame(wv, nd, nn, H, W, dt, window):
    """One frame in the arithmetic `dt`: (canvas uint8 [H,W], margin [H,W]).  wv [5], nd [7,8] float32, nn int."""
    f = dt
    x = np.arange(W, dtype=dt)[None, :]
    y = np.arange(H, dtype=dt)[:, None]
    amp, wl, thick, slope, spacing = (f(v) for v in wv)
    base = slope * x + amp * np.cos(x / wl) - f(W) * abs(slope)
    dydx = slope - amp / wl * np.sin(x / wl)
    q = (y - base) / spacing
    j = np.rint(q)
    nl = 60 + int(f(H) / spacing)
    inb = (j >= 0) & (j < nl)
    dist = np.abs(y - (base + j * spacing)) / np.sqrt(f(1) + dydx * dydx)
    half = f(0.5) * thick
    val = np.where(inb & (dist <= half), BLACK, GREY).astype(np.uint8)
    margin = np.abs(np.abs(q - np.floor(q)) - f(0.5)) * spacing             # the rint tie between two lines
    margin = np.minimum(margin, np.where(inb, np.abs(dist - half), np.inf)).astype(np.float64)
    for a in range(int(nn)):
        if nd[a, 7] == 0:
            continue
        cx, cy, A, B = (f(v) for v in nd[a, :4])
        th = -f(nd[a, 4]) * f(DEG)
        rings, start = int(nd[a, 5]), int(nd[a, 6])
        nwb = max(2 * rings, 1)
        t = max(np.rint(min(A, B) / f(nwb)), f(1))
        # only pixels inside the reject circle can be painted: work on its bounding box
        R = float(A) + 8.0
        x0, x1 = max(int(np.floor(float(cx) - R)) - 1, 0), min(int(np.ceil(float(cx) + R)) + 2, W)
        y0, y1 = max(int(np.floor(float(cy) - R)) - 1, 0), min(int(np.ceil(float(cy) + R)) + 2, H)
        if x0 >= x1 or y0 >= y1:
            continue
        dx, dy = x[:, x0:x1] - cx, y[y0:y1] - cy
        passed = ~(dx * dx + dy * dy > (A + f(8)) * (A + f(8)))
        cs, sn = np.cos(th), np.sin(th)
        u, v = dx * cs + dy * sn, -dx * sn + dy * cs
        rho = np.sqrt((u / A) * (u / A) + (v / B) * (v / B))
        jc = np.floor(rho * f(nwb + 1)).astype(np.int64) - 1
        sub, msub = val[y0:y1, x0:x1], margin[y0:y1, x0:x1]
        open_ = passed.copy()                                                # not yet painted by this antinode
        for jj in range(nwb - 1, -1, -1):                                   # the outermost matching outline wins
            s = f(jj + 1) / f(nwb + 1)
            aj, bj = A * s, B * s
            gu, gv = u / (aj * aj), v / (bj * bj)
            F = np.sqrt(u * gu + v * gv)
            gn = np.sqrt(gu * gu + gv * gv)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(gn > 0, np.abs(F - f(1)) * F / gn, bj)
            th_ = f(0.5) * t
            hit = open_ & (d <= th_)
            if window:
                hit &= (jj <= jc + 2) & (jj >= jc - 1)
            sub[hit] = RING if (start + jj) & 1 else BLACK
            open_ &= ~hit
            np.minimum(msub, np.where(passed, np.abs(d - th_), np.inf), out=msub)
    return val, margin


def _launch(waves, nodes, nnode, H, W, dt, window):
    waves = np.asarray(waves, np.float32).reshape(-1, WAVE_STRIDE)
    nodes = np.asarray(nodes, np.float32).reshape(-1, MAX_NODES, NODE_STRIDE)
    nnode = np.asarray(nnode, np.int32).reshape(-1)
    out = [_frame(waves[k], nodes[k], nnode[k], H, W, dt, window) for k in range(len(nnode))]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def canvas_ref(waves, nodes, nnode, H, W):
    """The noise-free canvas of a launch: waves [N,5], nodes [N,7,8], nnode [N] as the kernel receives them (float32),
    evaluated in float64, every outline tested.  Returns (canvas uint8 [N,H,W], margin float64 [N,H,W]): margin is the
    smallest distance (pixels) by which any comparison made for the pixel was decided -- the band threshold, the rint tie
    of the band index, every outline threshold of every valid antinode whose reject test the pixel passed."""
    return _launch(waves, nodes, nnode, H, W, np.float64, False)


def canvas_f32(waves, nodes, nnode, H, W, window=True):
    """The same formulas in float32 (numpy's, not the device's, sin / cos); window: the kernel's jc-1 .. jc+2 outlines."""
    return _launch(waves, nodes, nnode, H, W, np.float32, window)[0]


def pack(frames):
    """[(waves5, [node7or8, ...])] -> (waves [N,5], nodes [N,7,8], nnode [N]) float32 / int32, as generate_device packs:
    valid = 1 unless the node tuple carries its own eighth value."""
    n = len(frames)
    waves, nodes, nn = np.zeros((n, 5), np.float32), np.zeros((n, MAX_NODES, NODE_STRIDE), np.float32), np.zeros(n, np.int32)
    for k, (w, nds) in enumerate(frames):
        waves[k] = w
        nn[k] = len(nds)
        for j, node in enumerate(nds):
            nodes[k, j, :len(node)] = node
            if len(node) == 7:
                nodes[k, j, 7] = 1.0
    return waves, nodes, nn


def drawn_launch(n, seed, count_range=(1, 7)):
    """The parameter table generate_device(n, seed, count_range=...) sends, and the per-frame node lists."""
    from spnet_amd import fake_espi as F
    drawn = [F.draw_params(s, count_range)[:2] for s in F.frame_seeds(n, seed)]
    return pack(drawn), [nd for _, nd in drawn]


# ------------------------------------------------------------------------------------------------------- labels in pixels
def ring_runs(canvas, node):
    """Colour runs [(value, r_first, r_last)] of the canvas [H,W] sampled at the nearest pixel along the major-axis ray
    (cx + r cos(-angle), cy + r sin(-angle)), r = 0, 1, ... up to the rim (or the frame's edge)."""
    cx, cy, A, _, ang = (float(v) for v in node[:5])
    th = -ang * DEG
    H, W = canvas.shape
    runs = []
    for r in range(int(np.floor(A)) + 1):
        px, py = int(np.rint(cx + r * np.cos(th))), int(np.rint(cy + r * np.sin(th)))
        if not (0 <= px < W and 0 <= py < H):
            break
        v = int(canvas[py, px])
        if runs and runs[-1][0] == v:
            runs[-1][2] = r
        else:
            runs.append([v, r, r])
    return [tuple(r) for r in runs]


def outline_colours(runs, node):
    """The outline colours centre -> rim that `runs` show: background runs dropped, black runs that lie wholly inside the
    innermost outline's inner edge or outside the outermost outline's outer edge (wave bands showing through: on the major
    axis the first-order distance is exact, so the edges are at A (j+1)/(nwb+1) -+ t/2; one pixel of slack for the nearest
    -pixel sampling) dropped, neighbours of one colour merged (a wave band showing in the gap between two outlines always
    touches a black one)."""
    A, B, rings = float(node[2]), float(node[3]), int(node[5])
    nwb = max(2 * rings, 1)
    t = max(float(np.rint(np.float32(min(A, B)) / np.float32(nwb))), 1.0)
    r_in, r_out = A / (nwb + 1) - t / 2, A * nwb / (nwb + 1) + t / 2
    out = []
    for v, r0, r1 in runs:
        if v == GREY or (v == BLACK and (r1 < r_in + 1 or r0 > r_out - 1)):
            continue
        if not out or out[-1] != v:
            out.append(v)
    return out


def expected_colours(node):
    rings, start = int(node[5]), int(node[6])
    return [RING if (start + j) & 1 else BLACK for j in range(max(2 * rings, 1))]


def _box(node):
    cx, cy, a, b, ang = (float(v) for v in node[:5])
    rad = np.radians(ang)
    dx = np.sqrt(a ** 2 * np.cos(rad) ** 2 + b ** 2 * np.sin(rad) ** 2)
    dy = np.sqrt(a ** 2 * np.sin(rad) ** 2 + b ** 2 * np.cos(rad) ** 2)
    return cx - dx, cy - dy, cx + dx, cy + dy


def uncovered_nodes(nodes):
    """The nodes of one frame whose bounding box no LATER node's box touches (a later antinode paints over earlier ones)."""
    keep = []
    for k, nd in enumerate(nodes):
        a = _box(nd)
        if not any(not (a[2] < b[0] or a[0] > b[2] or a[3] < b[1] or a[1] > b[3]) for b in map(_box, nodes[k + 1:])):
            keep.append(nd)
    return keep


def check_labels_in_pixels(canvas, node_lists):
    """Every uncovered node of every frame shows exactly 2*rings alternating outlines, the innermost black iff start == 0.
    Returns the number of nodes checked."""
    checked = 0
    for k, nodes in enumerate(node_lists):
        for nd in uncovered_nodes(nodes):
            runs = ring_runs(canvas[k], nd)
            got = outline_colours(runs, nd)
            assert got == expected_colours(nd), (k, tuple(nd), runs)
            assert len(got) == 2 * int(nd[5]) and (got[0] == BLACK) == (int(nd[6]) == 0)
            checked += 1
    return checked


# --------------------------------------------------------------------------------------------------------- sensor model
def espi_hash(x):
    """The kernel's 32-bit mixer on a uint32 array (products wrap modulo 2^32)."""
    x = np.array(x, dtype=np.uint32, ndmin=1)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    x = x ^ (x >> np.uint32(16))
    return x


def sensor_hashes(seed, N, H, W):
    """h1, h2, h3 [N,H,W] uint32 of a launch: the pixel counter (f*H + y)*W + x in uint32, chained as the kernel chains."""
    f = np.arange(N, dtype=np.uint32)[:, None, None]
    y = np.arange(H, dtype=np.uint32)[None, :, None]
    x = np.arange(W, dtype=np.uint32)[None, None, :]
    pix = (f * np.uint32(H) + y) * np.uint32(W) + x
    h1 = espi_hash(pix * np.uint32(0x9e3779b9) + np.uint32(seed))
    h2 = espi_hash(h1 ^ np.uint32(0x85ebca6b))
    h3 = espi_hash(h2 + np.uint32(0xc2b2ae35))
    return h1, h2, h3


def uniforms(h1, h2):
    """u1 in (0, 1], u2 in [0, 1): formed in float32 exactly as the kernel forms them (its constants are float32 literals:
    16777217 is not a float32 and rounds to 2^24), returned as float64."""
    u1 = ((h1 >> np.uint32(8)).astype(np.float32) + np.float32(1)) * (np.float32(1) / np.float32(16777217.0))
    u2 = (h2 >> np.uint32(8)).astype(np.float32) * (np.float32(1) / np.float32(16777216.0))
    return u1.astype(np.float64), u2.astype(np.float64)


def sensor_ref(canvas, seed, H, W):
    """canvas uint8 [N,H,W] -> (dropout mask bool [N,H,W], noisy uint8 [N,H,W] BEFORE dropout, n float64 [N,H,W])."""
    canvas = np.asarray(canvas).reshape(-1, H, W)
    h1, h2, h3 = sensor_hashes(seed, canvas.shape[0], H, W)
    u1, u2 = uniforms(h1, h2)
    n = 40.0 + 40.0 * np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    noisy = np.minimum(canvas.astype(np.float64) + np.clip(np.rint(n), 0, 255), 255).astype(np.uint8)
    return (h3 & np.uint32(0x10000)) != 0, noisy, n


# ----------------------------------------------------------------------------------------------------- crafted launches
# One entry per launch: (H, W, [frame, frame, frame]), frame = (waves, [node, ...]); a node of eight values carries its own
# `valid`; "nnode" overrides the count the kernel is told (slots past it hold VALID nodes that must not be drawn).
# Shapes: two x-blocks with a partial second one, odd sizes, three x-blocks with the last one 8 wide, a single row.
# Centres, axes, angles and wave parameters are non-integers wherever the case does not need integers, so that no threshold
# is met exactly by a whole row or column of pixels; the bands are 23 px or more apart unless the case needs them closer and
# the 22-outline antinodes are small (a pixel's chance of lying within NEAR_TIE of a band edge is ~6e-3 / spacing, and every
# outline edge adds its length times 2 NEAR_TIE): tests/test_fake_espi_cpu.py holds each launch to NEAR_TIE_SHARE.
_GHOST = (150.2, 12.4, 30, 12, 25.5, 2, 1)          # a valid node parked in slots that nnode excludes
CASES = {
    "two_blocks_40x300": (40, 300, [
        # nnode = 0 with valid nodes in every slot; negative slope
        dict(waves=(12.3, 37, 5.2, -0.31, 45.3), nodes=[_GHOST] * 7, nnode=0),
        # nnode = 7: rings 0 / 1 / 5 / 11 with both starts, angles 0 / 90 / 180 / non-integer, a valid = 0 slot between two
        # valid ones (drawn, it would cover its neighbours); slope 0.  The first centre is a pixel and its single outline
        # reaches it (bj = 7.8 <= t/2 = 8): the gn == 0 branch paints that pixel
        dict(waves=(8.3, 51, 4.4, 0.0, 23.3), nodes=[
            (20, 19, 17.2, 15.6, 0, 0, 0), (60.7, 20.2, 18.3, 16.1, 90, 0, 1), (100.4, 18.9, 19.1, 14.3, 180, 1, 0),
            (121.0, 20.0, 24.0, 15.0, 33, 1, 1, 0.0), (141.2, 21.3, 19.4, 15.2, 37.5, 1, 1),
            (185.6, 19.4, 19.5, 17.6, 12.25, 5, 0), (240.1, 20.7, 14.3, 12.2, 101.7, 11, 1)]),
        # rint(2.5) = 2 and rint(3.5) = 4 (half to even) in the thickness; nnode = 2 of 4; positive slope
        # (rings 5 with start 1 and rings 11 with start 0 are in the launches below)
        dict(waves=(15.2, 29, 6.3, 0.42, 35.1), nodes=[
            (30.4, 20.3, 22.3, 15, 15.5, 3, 0), (80.6, 19.2, 12.7, 7, 60.25, 1, 1), _GHOST, (260.0, 20.0, 25, 14, 80, 2, 0)],
            nnode=2),
    ]),
    "odd_37x331": (37, 331, [
        # spacing < thick: bands cover everything a line index exists for; a circle
        dict(waves=(5.1, 40, 20.3, 0.0, 9.2), nodes=[(165.5, 18.5, 16.3, 16.3, 45, 2, 0)]),
        # spacing > H; centres outside the frame with the rim inside (left, and past the bottom-right corner); a pixel
        # exactly at a centre (gn == 0)
        dict(waves=(10.4, 60, 7.1, -0.15, 50.3), nodes=[
            (-6.5, 15.2, 30.2, 20.1, 20, 3, 1), (340.2, 40.3, 28.4, 18.2, 160, 2, 0), (200, 18, 25.3, 17.1, 63.3, 2, 1)]),
        # two overlapping antinodes (the later one wins wherever it paints); min(A,B)/nwb = 0.36: thickness clamped to 1
        dict(waves=(20.3, 45, 5.3, 0.9, 34.2), nodes=[
            (100.3, 18.1, 30.2, 16.3, 15, 3, 0), (120.8, 20.4, 28.1, 15.2, 140, 2, 1), (250.6, 18.3, 20.4, 8, 75, 11, 0)]),
    ]),
    "three_blocks_24x520": (24, 520, [
        # antinodes across both block seams (x = 256, x = 512) and in the 8-wide last block; 5 / 2 = 2.5 again; a steep
        # positive slope over close lines: left of x ~ 150 the nearest line's index is past 60 + int(H/spacing), no band
        dict(waves=(9.2, 33, 12.3, 1.4, 8.4), nodes=[
            (256.4, 12.2, 20.3, 10.4, 30, 1, 0), (505.7, 11.6, 14.2, 9.3, 0, 2, 1), (516.2, 5.5, 6.4, 5, 120.5, 1, 1)]),
        dict(waves=(6.37, 70, 3.3, 0.0, 28.3), nodes=[_GHOST], nnode=0),
        dict(waves=(14.1, 25, 8.2, -1.2, 30.4), nodes=[(507.5, 12.5, 22.2, 11.3, 90, 5, 1), (130.2, 10.9, 40.3, 11.2, 3.7, 0, 0)]),
    ]),
    "one_row_1x64": (1, 64, [
        dict(waves=(3.2, 10, 2.3, 0.1, 5.2), nodes=[(31.6, 0.3, 12.2, 7.4, 10, 1, 0)]),
        dict(waves=(4.1, 12, 3.2, -0.2, 6.3), nodes=[_GHOST], nnode=0),
        dict(waves=(2.7, 9, 2.2, 0.0, 4.3), nodes=[(10.2, -3.4, 14.3, 9.1, 77, 2, 1)]),
    ]),
}
SENSOR_CASE = "three_blocks_24x520"


def case_launch(name):
    """(H, W, waves [3,5], nodes [3,7,8], nnode [3]) of a crafted launch."""
    H, W, frames = CASES[name]
    waves, nodes, nn = pack([(fr["waves"], fr["nodes"]) for fr in frames])
    for k, fr in enumerate(frames):
        if "nnode" in fr:
            nn[k] = fr["nnode"]
    return H, W, waves, nodes, nn
