"""csrc/overlay.hip through spnet_amd.overlay.draw_overlays_device against the numpy restatement
(tests/helpers/overlay_ref.py, itself held against Pillow in tests/test_overlay_cpu.py): byte for byte.

Frames are the smallest on which the kernel can still go wrong: 37 x 53 (odd, a partial 64 x 16 tile in both directions,
byte accesses), 64 x 64 (exactly one tile wide, four high, the 16-byte paths), 24 x 80 (16-byte paths with a partial tile),
grey and RGB, three frames a launch.  The scene holds an outline that crosses every frame edge, one wholly outside, the
three degenerate ellipses, two crossing outlines of different colour, a label under an outline and one over it, a frame
with no commands, equal strings sharing a mask and a file name that runs past the right edge.  One case has 257
commands in one tile, one more than the kernel's LDS list holds.  End to end: show_pred_ellipses(draw="device",
png="device") on four written fake-ESPI files."""
import os

import numpy as np
import pytest
import torch
from PIL import Image, ImageDraw

from spnet_amd import overlay as O
from spnet_amd import utils as U
from tests.helpers import overlay_ref as R

pytestmark = pytest.mark.gpu

LIST_CAPACITY = 256          # OV_CAP of csrc/overlay.hip

YELLOW, CYAN, RED, WHITE = (255, 255, 0), (0, 255, 255), (255, 0, 0), (255, 255, 255)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _ell(cx, cy, a, b, angle):
    return U.ellipse_polygon([cx, cy], [a, b], angle)


def scene(H, W):
    """Three frames of commands for an H x W frame."""
    mx, my = W // 2, H // 2
    first = [("outline", YELLOW, _ell(mx, my, W // 2 + 3, H // 2 + 3, 180.0)),        # crosses all four edges
             ("outline", RED, _ell(W + 50, H + 50, 10, 5, 30.0)),                      # wholly outside
             ("outline", CYAN, _ell(mx - 4, my, 14, 6, 25.0)),                         # two colours crossing: order shows
             ("outline", RED, _ell(mx + 3, my - 2, 6, 13, 110.0)),
             ("text", WHITE, (mx - 12, my - 4), "12.5"),                               # a label over the outlines ...
             ("outline", YELLOW, _ell(mx, my, 9, 3, 170.0)),                           # ... and an outline over the label
             ("text", CYAN, (W - 20, 1), " 3.0")]
    third = [("outline", CYAN, _ell(7, 9, 0, 5, 40.0)),                                # a == 0
             ("outline", YELLOW, _ell(W - 8, 6, 5, 0, 75.0)),                          # b == 0
             ("outline", RED, _ell(mx, H - 3, 0, 0, 180.0)),                           # both: a disc, cut by the edge
             ("text", YELLOW, (3, my), " 3.0"),                                        # equal strings: one mask
             ("text", RED, (mx, my + 6), " 3.0"),
             ("text", WHITE, (5, H - 14), "steelpan_0000042.png")]                     # runs past the right edge
    return [first, [], third]


CASES = [(37, 53, 1), (37, 53, 3), (64, 64, 1), (64, 64, 3), (24, 80, 1), (24, 80, 3)]


@pytest.fixture(scope="module")
def cases():
    """(H, W, channels) -> (frames, plan, the restatement's output); computed once, never changed."""
    _need_gpu()
    out = {}
    for H, W, ch in CASES:
        rng = np.random.RandomState(H * 100 + W + ch)
        frames = rng.randint(0, 256, (3, H, W) if ch == 1 else (3, H, W, 3)).astype(np.uint8)
        plan = O.pack_commands(scene(H, W), [(H, W)] * 3)
        want = R.draw_plan(frames, plan)
        want.setflags(write=False)
        out[(H, W, ch)] = (frames, plan, want)
    return out


@pytest.mark.parametrize("H,W,ch", CASES)
def test_device_equals_the_restatement(cases, H, W, ch):
    frames, plan, want = cases[(H, W, ch)]
    assert plan.cmd[10, 6] == plan.cmd[11, 6] == plan.cmd[6, 6]                       # the three " 3.0" share one mask
    assert plan.cmd[1, 4] <= plan.cmd[1, 2] and plan.frame_start.tolist() == [0, 7, 7, 13]
    rgb0 = np.repeat(frames[..., None], 3, -1) if ch == 1 else frames
    assert (want[0] != rgb0[0]).any() and (want[2] != rgb0[2]).any() and np.array_equal(want[1], rgb0[1])
    got = O.draw_overlays_device(torch.from_numpy(frames).cuda(), plan)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3, H, W, 3) and got.is_cuda
    got = got.cpu().numpy()
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())
    if ch == 1:                                                                     # [N,H,W,1] is the same input
        again = O.draw_overlays_device(torch.from_numpy(frames).cuda().unsqueeze(-1), plan).cpu().numpy()
        assert np.array_equal(again, want)


def test_unaligned_frames_and_a_chunk_of_a_plan(cases):
    """The same frames one byte into a buffer (no 16-byte path although W % 16 == 0), and frames 1 .. 2 alone."""
    frames, plan, want = cases[(64, 64, 1)]
    buf = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(frames).reshape(-1)
    got = O.draw_overlays_device(buf[1:].view(3, 64, 64), plan).cpu().numpy()
    assert np.array_equal(got, want)
    got = O.draw_overlays_device(torch.from_numpy(frames[1:]).cuda(), plan.chunk(1, 3)).cpu().numpy()
    assert np.array_equal(got, want[1:])


def test_one_command_more_than_the_list_holds():
    """257 commands in the first tile of a 64 x 64 frame: the last one, painted in a second round, must land on top."""
    _need_gpu()
    H = W = 64
    rng = np.random.RandomState(9)
    commands = []
    for k in range(LIST_CAPACITY + 1):
        rgb = tuple(int(v) for v in rng.randint(0, 256, 3))
        x, y = int(rng.randint(2, 60)), int(rng.randint(2, 14))
        if k % 3 == 2:
            commands.append(("text", rgb, (x - 2, y - 6), "%d" % (k % 10)))
        else:
            commands.append(("outline", rgb, _ell(x, y, int(rng.randint(0, 9)), int(rng.randint(0, 4)), float(rng.uniform(1, 180)))))
    commands[-1] = ("outline", WHITE, _ell(30, 8, 25, 5, 180.0))
    plan = O.pack_commands([commands, commands[:3]], [(H, W)] * 2)
    assert plan.frame_start.tolist() == [0, LIST_CAPACITY + 1, LIST_CAPACITY + 4]
    assert (plan.cmd[:LIST_CAPACITY + 1, 3] < 16).all() and (plan.cmd[:LIST_CAPACITY + 1, 2] < 64).all()    # all in tile (0, 0)
    frames = rng.randint(0, 256, (2, H, W)).astype(np.uint8)
    want = R.draw_plan(frames, plan)
    short = O.pack_commands([commands[:-1], commands[:3]], [(H, W)] * 2)
    assert (R.draw_plan(frames, short) != want).any()                               # the 257th command shows
    got = O.draw_overlays_device(torch.from_numpy(frames).cuda(), plan).cpu().numpy()
    assert np.array_equal(got, want), "%d bytes differ" % int((got != want).sum())


def test_bad_arguments_are_refused():
    _need_gpu()
    plan = O.pack_commands([[]], [(8, 8)])
    with pytest.raises(TypeError):
        O.draw_overlays_device(torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda"), plan)
    with pytest.raises(ValueError):
        O.draw_overlays_device(torch.zeros((1, 8, 8, 2), dtype=torch.uint8, device="cuda"), plan)
    with pytest.raises(ValueError):
        O.draw_overlays_device(torch.zeros((2, 8, 8), dtype=torch.uint8, device="cuda"), plan)
    with pytest.raises(ValueError):
        O.draw_overlays_device(torch.zeros((1, 8, 9), dtype=torch.uint8, device="cuda"), plan)
    from spnet_amd import _lib as L
    z = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(L.HipError):
        L.spnet_draw_overlays(z.data_ptr(), 1, 8, 5000, 1, z.data_ptr(), z.data_ptr(), 0, z.data_ptr(), 0, z.data_ptr(), 0,
                              z.data_ptr(), L.current_stream())
    with pytest.raises(L.HipError):
        L.spnet_draw_overlays(z.data_ptr(), 1, 4, 4, 2, z.data_ptr(), z.data_ptr(), 0, z.data_ptr(), 0, z.data_ptr(), 0,
                              z.data_ptr(), L.current_stream())
    out = O.draw_overlays_device(torch.zeros((0, 8, 8), dtype=torch.uint8, device="cuda"), O.pack_commands([], []))
    assert tuple(out.shape) == (0, 8, 8, 3)


def _decoded(directory):
    return {f: np.asarray(Image.open(os.path.join(directory, f))) for f in sorted(os.listdir(directory)) if f.endswith(".png")}


def test_show_pred_ellipses_draws_on_the_device(tmp_path):
    """Four written fake-ESPI files: the PNG files decode to the restatement's pixels, the CSV is the host path's."""
    _need_gpu()
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    _, labels, frames = F.generate_device(4, seed=11, want_u8=True)
    frames = frames.cpu().numpy()
    src = tmp_path / "src"
    src.mkdir()
    files = []
    for j in range(4):
        files.append(str(src / ("steelpan_%07d.png" % j)))
        Image.fromarray(frames[j]).save(files[-1])
    v = cf.vars_per_pred
    n_pred = max(max(len(rows) for rows in labels), 1) + 1
    Yp = np.zeros((4, n_pred * v), np.float64)
    Yp[:, 6::v] = 1.0
    Yt = Yp.copy()
    for j, rows in enumerate(labels):
        for k, (cx, cy, a, b, angle, rings) in enumerate(rows):
            t = 2 * np.deg2rad(float(angle))
            Yt[j, k * v:(k + 1) * v] = (cx, cy, a, b, np.cos(t), np.sin(t), 0, rings)
            Yp[j, k * v:(k + 1) * v] = (cx + 3.4, cy - 2.2, a * 0.9, b * 1.1, np.cos(t + 0.1), np.sin(t + 0.1), 0.2, rings + 0.3)
    Yp[3, :] = Yt[3, :] = 0.0
    Yp[3, 6::v] = Yt[3, 6::v] = 1.0                                                  # a frame with nothing to draw
    assert sum(len(rows) for rows in labels[:3]) > 0
    plan = O.plan_overlays(Yt, Yp, files, show_true=True, size=(384, 512))
    want = R.draw_plan(frames, plan)
    outs = {}
    for name, kw in (("host", dict(draw="host", png="host")),
                     ("device", dict(draw="device", png="device", png_chunk=3)),
                     ("device_pillow", dict(draw="device", png="host", png_chunk=3)),
                     ("device_decode", dict(draw="device", png="device", device_decode=True, png_chunk=3))):
        d = tmp_path / name
        d.mkdir()
        U.show_pred_ellipses(Yt, Yp, files, num_draw=4, log_dir=str(d), out_csv=str(d / "pred.csv"), **kw)
        outs[name] = (_decoded(str(d)), (d / "pred.csv").read_text())
    names = ["steelpan_pred_%05d.png" % j for j in range(4)]
    for name in ("device", "device_pillow", "device_decode"):
        pix, text = outs[name]
        assert sorted(pix) == names
        assert text == outs["host"][1] == "".join(plan.csv)
        for j, f in enumerate(names):
            assert pix[f].shape == (384, 512, 3) and np.array_equal(pix[f], want[j]), (name, f)
    # against the host path's pixels: only near outlines may a pixel differ (the documented rule), never far from them
    for j, f in enumerate(names):
        host = outs["host"][0][f]
        differs = (host != want[j]).any(axis=2)
        outline = np.zeros((384, 512), bool)
        for c in plan.frames[j]:
            if c[0] == "outline":
                pts = [tuple(p) for p in c[2]]
                img = Image.new("L", (512, 384), 0)
                ImageDraw.Draw(img).line(pts + [pts[0]], fill=255, width=3, joint="curve")
                outline |= R.outline_cover(O.quantise_vertices(c[2]), 384, 512) | (np.asarray(img) != 0)
        assert not (differs & ~R.near(outline, 2)).any(), f
    assert (want[0] != np.repeat(frames[0][..., None], 3, 2)).any()
