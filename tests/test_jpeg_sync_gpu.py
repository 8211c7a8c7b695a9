"""spnet_jpeg_entropy_sync (spnet_amd/csrc/jpeg_decode_sync.hip: a workgroup per restart interval, a lane per segment,
speculative decoding chained until it is the serial decode) against the serial kernel spnet_jpeg_entropy -- workspace and
status, torch.equal -- and against Pillow through spnet_jpeg_pixels and the public entropy= argument."""
import numpy as np
import pytest
import torch

from tests.helpers import jpeg_decode_corpus as C

pytestmark = pytest.mark.gpu

SEGS = (4, 8, 32, 256)
LANES = 256              # of the kernel's workgroup (csrc/jpeg_decode_sync.hip)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


class Launch:
    """One plan in device memory, and both entropy kernels on it."""

    def __init__(self, datas):
        from spnet_amd import jpeg as J
        self.infos = [J.parse_jpeg(d) for d in datas]
        assert all(i.device for i in self.infos), [i.host_reason for i in self.infos]
        self.plan = J.plan_decode(self.infos)
        self.dev = {k: torch.from_numpy(self.plan[k].view(np.uint8).reshape(-1).copy()).cuda()
                    for k in ("intervals", "files", "tables", "quant", "blob")}
        self.n = len(datas)

    def _args(self, coef, status, seg_bytes=None):
        from spnet_amd import _lib as L
        p, d = self.plan, self.dev
        head = (d["blob"].data_ptr(), int(p["blob"].size), d["intervals"].data_ptr(), int(p["intervals"].shape[0]),
                d["files"].data_ptr(), self.n, d["tables"].data_ptr(), int(p["tables"].shape[0]))
        tail = (coef.data_ptr(), int(p["blocks"]), status.data_ptr(), L.current_stream())
        return head + (() if seg_bytes is None else (seg_bytes,)) + tail

    def serial(self):
        from spnet_amd import _lib as L
        coef = torch.zeros((self.plan["blocks"], 64), dtype=torch.int16, device="cuda")
        status = torch.full((self.n,), 77, dtype=torch.int32, device="cuda")
        L.spnet_jpeg_entropy(*self._args(coef, status))
        return coef, status

    def sync(self, seg_bytes):
        from spnet_amd import _lib as L
        coef = torch.zeros((self.plan["blocks"], 64), dtype=torch.int16, device="cuda")
        status = torch.zeros((self.n,), dtype=torch.int32, device="cuda")             # the kernel merges, it does not clear
        L.spnet_jpeg_entropy_sync(*self._args(coef, status, seg_bytes))
        return coef, status

    def pixels(self, coef, status, k=0):
        """uint8 [H][W][C] of file k (all files of the plan have its size)."""
        from spnet_amd import _lib as L
        i = self.infos[k]
        out = torch.zeros((self.n, i.height, i.width, i.components), dtype=torch.uint8, device="cuda")
        L.spnet_jpeg_pixels(coef.data_ptr(), int(self.plan["blocks"]), self.dev["files"].data_ptr(), self.n,
                            self.dev["quant"].data_ptr(), int(self.plan["quant"].shape[0]), i.height, i.width, i.components,
                            0, out.data_ptr(), status.data_ptr(), L.current_stream())
        return out[k].cpu().numpy()


@pytest.fixture(scope="module")
def corpus_launch():
    """The whole corpus (every size, encoder, option, table set and sampling) as ONE plan, and the serial kernel's result
    on it: computed once, never changed."""
    _need_gpu()
    launch = Launch([c.data for c in C.corpus()])
    coef, status = launch.serial()
    assert not status.any()
    return launch, coef, status


@pytest.mark.parametrize("seg_bytes", SEGS)
def test_corpus_equals_the_serial_kernel(corpus_launch, seg_bytes):
    launch, want, want_status = corpus_launch
    coef, status = launch.sync(seg_bytes)
    assert torch.equal(status, want_status)
    assert torch.equal(coef, want), int((coef != want).sum())


def test_two_runs_give_identical_workspaces(corpus_launch):
    launch, want, _ = corpus_launch
    a, sa = launch.sync(8)
    b, sb = launch.sync(8)
    assert torch.equal(a, b) and torch.equal(sa, sb) and torch.equal(a, want)


@pytest.mark.parametrize("sub", [None, 2], ids=["grey", "420"])
def test_more_segments_than_lanes(sub):
    """96 x 128 noise at quality 100, no restart markers, 4-byte segments: thousands of segments for 256 lanes, so the
    interval is worked off in batches that hand their exit state on."""
    _need_gpu()
    from spnet_amd import jpeg as J
    shape = (96, 128) if sub is None else (96, 128, 3)
    kw = dict(quality=100) if sub is None else dict(quality=100, subsampling=sub)
    data = C.pillow_jpeg(C.content("noise", shape, 1), **kw)
    info = J.parse_jpeg(data)
    assert info.bounds.shape[0] == 1 and int(info.bounds[0][1] - info.bounds[0][0]) // 4 > LANES
    launch = Launch([data])
    want, want_status = launch.serial()
    coef, status = launch.sync(4)
    assert torch.equal(status, want_status) and not status.any()
    assert torch.equal(coef, want), int((coef != want).sum())
    assert np.array_equal(launch.pixels(coef, status), C.pillow_pixels(data))


def test_short_intervals():
    """An interval of exactly one segment, and intervals shorter than seg_bytes."""
    _need_gpu()
    from spnet_amd import jpeg as J
    data = C.pillow_jpeg(C.content("noise", (8, 8), 2), quality=50)
    lo, hi = (int(v) for v in J.parse_jpeg(data).bounds[0])
    one = (hi - lo + 3) // 4 * 4
    assert 4 <= one <= 4096
    launch = Launch([data])
    want, want_status = launch.serial()
    for seg_bytes in (one, one + 4, 4096):
        assert (hi - lo + seg_bytes - 1) // seg_bytes == 1 and (seg_bytes == one or hi - lo < seg_bytes)
        coef, status = launch.sync(seg_bytes)
        assert torch.equal(status, want_status) and not status.any() and torch.equal(coef, want), seg_bytes
    assert np.array_equal(launch.pixels(coef, status), C.pillow_pixels(data))
    for seg_bytes in (0, 2, 6, 4100):
        with pytest.raises(Exception, match="spnet_jpeg_entropy_sync"):
            launch.sync(seg_bytes)


def _damaged_sets():
    from tests.helpers.jpeg_sync_cases import pillow_damaged
    bad, sound = C.damaged()
    out = [("ours-" + n, bad[n], sound) for n in sorted(bad)]
    bad, sound = pillow_damaged()
    return out + [("pillow-" + n, bad[n], sound) for n in sorted(bad)]


@pytest.mark.parametrize("which", range(6), ids=["ours-cut", "ours-flipped", "ours-unassigned", "pillow-cut",
                                                 "pillow-flipped", "pillow-garbage"])
def test_damaged_file_between_sound_ones(which):
    _need_gpu()
    from spnet_amd import jpeg as J
    name, bad, sound = _damaged_sets()[which]
    datas = [sound, bad, sound]
    launch = Launch(datas)
    want, want_status = launch.serial()
    assert want_status[0] == 0 and want_status[2] == 0 and want_status[1] != 0
    blocks = launch.infos[0].blocks
    for seg_bytes in (4, 32):
        coef, status = launch.sync(seg_bytes)
        assert torch.equal(status, want_status), (name, status.tolist(), want_status.tolist())
        assert torch.equal(coef[:blocks], want[:blocks]) and torch.equal(coef[2 * blocks:], want[2 * blocks:])
    assert np.array_equal(launch.pixels(coef, status, 0), C.pillow_pixels(sound))
    assert np.array_equal(launch.pixels(coef, status, 2), C.pillow_pixels(sound))
    # the public call: the host decodes what the device rejected
    try:
        pil = C.pillow_pixels(bad)[:, :, 0]
    except Exception as e:                                   # noqa: BLE001 -- whatever the default path raises
        with pytest.raises(type(e)):
            J.decode_jpeg_device(datas, entropy="sync")
        return
    got, status, info = J.decode_jpeg_device(datas, return_info=True, entropy="sync", seg_bytes=32)
    assert info == [1] and status[1] == int(want_status[1]) and status[0] == 0 and status[2] == 0
    got = got.cpu().numpy()
    sound_px = C.pillow_pixels(sound)[:, :, 0]
    assert np.array_equal(got[0], sound_px) and np.array_equal(got[2], sound_px) and np.array_equal(got[1], pil)


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_public_sync_path_equals_pillow(shape):
    _need_gpu()
    from spnet_amd import jpeg as J
    cases = [c for c in C.corpus() if c.shape == shape]
    wants = C.expected(cases)
    intervals = sum(int(J.parse_jpeg(c.data).bounds.shape[0]) for c in cases)
    for channels in ("first", "all"):
        got, status, info = J.decode_jpeg_device([c.data for c in cases], channels=channels, return_info=True,
                                                 entropy="sync", seg_bytes=8)
        assert info == [] and not status.any() and (info.lane_intervals, info.sync_intervals) == (0, intervals)
        got = got.cpu().numpy()
        for k, c in enumerate(cases):
            want = wants[c.name] if channels == "all" else wants[c.name][:, :, 0]
            assert np.array_equal(got[k], want.reshape(got[k].shape)), c.name
    same = J.decode_jpeg_device([c.data for c in cases], channels="all", entropy="interval")
    assert np.array_equal(same.cpu().numpy(), got)


def test_auto_sends_each_interval_to_its_kernel():
    """One 384 x 512 frame as this project's encoder writes it (48 short intervals) and as Pillow writes it without
    restart markers (one long interval), in one call: both kernels run on one workspace."""
    _need_gpu()
    from spnet_amd import jpeg as J
    yy, xx = np.mgrid[0:384, 0:512]
    frame = 110 + 70 * np.cos(np.hypot(xx - 200, yy - 150) ** 2 / 900) + np.random.default_rng(2).normal(0, 12, (384, 512))
    frame = np.clip(frame, 0, 255).astype(np.uint8)
    ours = J.encode_jpeg_device(torch.from_numpy(frame[None]).cuda(), 90)[0]
    plain = C.pillow_jpeg(frame, quality=90)
    assert J.parse_jpeg(ours).bounds.shape[0] == 48 and J.parse_jpeg(plain).bounds.shape[0] == 1
    assert int(np.diff(J.parse_jpeg(plain).bounds[0])[0]) >= J.SYNC_MIN_BYTES
    assert int(np.diff(J.parse_jpeg(ours).bounds, axis=1).max()) < J.SYNC_MIN_BYTES
    want = np.stack([C.pillow_pixels(ours)[:, :, 0], C.pillow_pixels(plain)[:, :, 0]])
    got, status, info = J.decode_jpeg_device([ours, plain], return_info=True, entropy="auto")
    assert info == [] and not status.any() and (info.lane_intervals, info.sync_intervals) == (48, 1)
    assert np.array_equal(got.cpu().numpy(), want)
    got, status, info = J.decode_jpeg_device([ours, plain], return_info=True, entropy="interval")
    assert (info.lane_intervals, info.sync_intervals) == (49, 0) and np.array_equal(got.cpu().numpy(), want)
    got, status, info = J.decode_jpeg_device([ours, plain], return_info=True)            # the default
    assert info.lane_intervals + info.sync_intervals == 49 and np.array_equal(got.cpu().numpy(), want)


def test_movie_of_pillow_frames(tmp_path):
    _need_gpu()
    from spnet_amd import jpeg as J
    files = [C.pillow_jpeg(C.content("noise", (40, 72), s), quality=90) for s in range(3)]
    it = iter(files)
    path = str(tmp_path / "camera.avi")
    with J.MjpegWriter(path, 72, 40, fps=25.0, channels=1, encoder=lambda frames: [next(it) for _ in frames]) as w:
        for _ in files:
            w.add(np.zeros((1, 40, 72), np.uint8))
    reader = J.MjpegReader(path)
    assert len(reader) == 3 and all(J.parse_jpeg(reader.frame_bytes(k)).restart == 0 for k in range(3))
    want = np.stack([C.pillow_pixels(f)[:, :, 0] for f in files])
    got, status, info = reader.read_device(entropy="sync", return_info=True)
    assert info == [] and not status.any() and (info.lane_intervals, info.sync_intervals) == (0, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(reader.read_device([2, 0], entropy="sync", seg_bytes=4).cpu().numpy(), want[[2, 0]])
