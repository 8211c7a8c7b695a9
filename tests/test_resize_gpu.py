"""Device resize on the GPU: spnet_resize_u8 (csrc/resize.hip) against PIL.Image.resize itself, bit for bit, and the
opt-in surface built on it -- Model.predict(resize=True), fake_espi.generate_device(size=...), predict_spnet's
device_resize -- against the host path each replaces."""
import numpy as np
import pytest
from PIL import Image

pytestmark = pytest.mark.gpu

# the CPU test's cases (tests/test_resize_cpu.py): (H, W) -> (OH, OW)
CASES = [((384, 512), (331, 331)), ((384, 512), (224, 224)), ((384, 512), (384, 512)), ((384, 512), (331, 512)),
         ((96, 128), (131, 150)), ((47, 61), (29, 17)), ((47, 61), (1, 47))]


def frames(N, H, W, seed=0):
    """uniform noise, 0/255 binary, smooth fringes in turn: uint8 [N, H, W]"""
    rs = np.random.RandomState(seed + 31 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((N, H, W), np.uint8)
    for i in range(N):
        if i % 3 == 0:
            out[i] = rs.randint(0, 256, (H, W))
        elif i % 3 == 1:
            out[i] = rs.randint(0, 2, (H, W)) * 255
        else:
            out[i] = 127.5 + 127.5 * np.sin(xx / (5.0 + i) + yy / 23.0) * np.cos(yy / 7.0)
    return out


def pil_resize(a, OH, OW):
    """The input codec's own call (utils._load_one): RGB, resize, channel 0."""
    return np.asarray(Image.fromarray(a).convert("RGB").resize((OW, OH), Image.LANCZOS), dtype=np.uint8)[:, :, 0]


@pytest.mark.parametrize("src,dst", CASES)
def test_kernel_equals_pillow_bit_for_bit(src, dst):
    """N = 1, 5 and 37 frames; out_u8 alone, out_f alone, both; out_f == to_network_input(out_u8) bit for bit; a frame's
    bits do not depend on N (37 frames of 331 x 331 bytes also put every output alignment in play)."""
    import torch
    from spnet_amd import fake_espi as F
    from spnet_amd import resize as RZ
    (H, W), (OH, OW) = src, dst
    X = frames(37, H, W)
    ref = np.stack([pil_resize(a, OH, OW) for a in X])
    Xd = torch.from_numpy(X).cuda()
    for N in (1, 5, 37):
        u_only, none_f = RZ.resize_u8_device(Xd[:N], (OH, OW))
        assert none_f is None and u_only.shape == (N, OH, OW)
        f_buf = torch.full((N, OH, OW, 1), float("nan"), device="cuda")
        _, f_only = RZ.resize_u8_device(Xd[:N], (OH, OW), out_f=f_buf)
        u_buf = torch.full((N, OH, OW), 77, dtype=torch.uint8, device="cuda")
        f_buf2 = torch.full((N, OH, OW, 1), float("nan"), device="cuda")
        RZ.resize_u8_device(Xd[:N, :, :, None], (OH, OW), out_f=f_buf2, out_u8=u_buf)
        got = u_only.cpu().numpy()
        assert np.array_equal(got, ref[:N]), "%d pixels differ (N = %d, %s -> %s)" % (int((got != ref[:N]).sum()), N, src, dst)
        assert np.array_equal(u_buf.cpu().numpy(), ref[:N])
        want_f = F.to_network_input(ref[:N])
        assert np.array_equal(f_only.cpu().numpy(), want_f)
        assert np.array_equal(f_buf2.cpu().numpy(), want_f)


def test_kernel_takes_slices_at_any_alignment():
    """Frames 3..8 of a resident batch into frames 1..6 of larger outputs: neither the source slice (61 x 47 bytes per
    frame) nor the output slices start on a 16-byte boundary, and the frames around them stay untouched."""
    import torch
    from spnet_amd import fake_espi as F
    from spnet_amd import resize as RZ
    X = frames(9, 47, 61, seed=4)
    ref = np.stack([pil_resize(a, 29, 17) for a in X[3:8]])
    Xd = torch.from_numpy(X).cuda()
    u = torch.full((7, 29, 17), 201, dtype=torch.uint8, device="cuda")
    f = torch.full((7, 29, 17), 5.0, device="cuda")
    RZ.resize_u8_device(Xd[3:8], (29, 17), out_f=f[1:6], out_u8=u[1:6])
    assert np.array_equal(u[1:6].cpu().numpy(), ref)
    assert np.array_equal(f[1:6].cpu().numpy(), F.to_network_input(ref)[..., 0])
    for k in (0, 6):
        assert bool((u[k] == 201).all()) and bool((f[k] == 5.0).all())


def test_bad_shapes_return_an_error_and_write_nothing():
    import torch
    from spnet_amd import _lib as L
    from spnet_amd import resize as RZ
    H, W, OH, OW = 47, 61, 29, 17
    Xd = torch.from_numpy(frames(2, H, W)).cuda()
    xt = torch.from_numpy(np.array(RZ.lanczos_taps(W, OW))).cuda()
    yt = torch.from_numpy(np.array(RZ.lanczos_taps(H, OH))).cuda()
    xtaps, ytaps = xt.shape[1] - 2, yt.shape[1] - 2
    out = torch.full((2, OH, OW), 99, dtype=torch.uint8, device="cuda")
    outf = torch.full((2, OH, OW), 3.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = dict(src=Xd.data_ptr(), N=2, H=H, W=W, xtab=xt.data_ptr(), xtaps=xtaps, ytab=yt.data_ptr(), ytaps=ytaps, OH=OH,
                OW=OW, out_u8=out.data_ptr(), out_f=outf.data_ptr())
    order = ("src", "N", "H", "W", "xtab", "xtaps", "ytab", "ytaps", "OH", "OW", "out_u8", "out_f")
    bad = [dict(H=0), dict(W=0), dict(OH=0), dict(OW=-3), dict(H=2049), dict(OW=2049), dict(N=-1), dict(src=None),
           dict(out_u8=None, out_f=None), dict(xtab=None), dict(ytab=None), dict(xtaps=0), dict(ytaps=H + 1),
           dict(out_f=outf.data_ptr() + 2)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(L.HipError):
            L.spnet_resize_u8(*[a[k] for k in order], st)
    torch.cuda.synchronize()
    assert bool((out == 99).all()) and bool((outf == 3.0).all())
    L.spnet_resize_u8(*[good[k] for k in order], st)              # ... and the unchanged arguments are accepted
    assert np.array_equal(out.cpu().numpy(), np.stack([pil_resize(a, OH, OW) for a in Xd.cpu().numpy()]))
    # the Python entry: wrong dtype / output size
    with pytest.raises(TypeError):
        RZ.resize_u8_device(Xd.float(), (OH, OW))
    with pytest.raises(ValueError):
        RZ.resize_u8_device(Xd, (OH, OW), out_u8=torch.empty((2, OH, OW + 1), dtype=torch.uint8, device="cuda"))


def test_predict_resizes_native_frames_on_the_device():
    """Model((331, 331, 1)).predict(native uint8 frames, resize=True) == predict of the frames PIL resized on the host:
    host array (streamed at 384 x 512) and device tensor, ragged last batch; a size mismatch without the flag still
    raises ValueError."""
    import torch
    from spnet_amd import models as M
    U = frames(11, 384, 512, seed=2)
    U331 = np.stack([pil_resize(a, 331, 331) for a in U])
    model = M.Model((331, 331, 1), Y0size=576, seed=5)
    want = model.predict(U331[..., None], batch_size=4)
    assert np.abs(want).max() > 0
    y_host = model.predict(U, batch_size=4, resize=True)
    y_host4 = model.predict_u8(U[..., None], batch_size=4, resize=True)
    y_dev = model.predict(torch.from_numpy(U).cuda(), batch_size=4, resize=True)
    assert np.array_equal(y_host, want) and np.array_equal(y_host4, want) and np.array_equal(y_dev, want)
    # frames that already have the model's size pass through unchanged
    assert np.array_equal(model.predict(U331, batch_size=4, resize=True), want)
    with pytest.raises(ValueError):
        model.predict(U, batch_size=4)
    with pytest.raises(TypeError):
        model.predict(U.astype(np.float32), batch_size=4, resize=True)


def test_generate_device_at_the_network_size():
    """generate_device(n, size=331, want_u8=True): the uint8 frames are Pillow's resize of the 384 x 512 uint8 frames the
    same call returns with size=None, X is their network input, the labels are unchanged (two chunks, the second
    ragged)."""
    from spnet_amd import fake_espi as F
    n = 7
    X0, lab0, U0 = F.generate_device(n, seed=3, want_u8=True, chunk=4)
    X1, lab1, U1 = F.generate_device(n, seed=3, want_u8=True, chunk=4, size=331)
    assert lab1 == lab0 and U0.shape == (n, 384, 512)
    assert X1.shape == (n, 331, 331, 1) and U1.shape == (n, 331, 331)
    ref = np.stack([pil_resize(a, 331, 331) for a in U0.cpu().numpy()])
    assert np.array_equal(U1.cpu().numpy(), ref)
    assert np.array_equal(X1.cpu().numpy(), F.to_network_input(ref))
    X2, lab2 = F.generate_device(n, seed=3, chunk=4, size=(331, 331))
    assert lab2 == lab0 and np.array_equal(X2.cpu().numpy(), X1.cpu().numpy())


def test_predict_network_csv_is_identical_with_device_resize(tmp_path):
    """predict_spnet.predict_network over a small written dataset: hawley_spnet.csv byte for byte the same whether the
    host (PIL, float frames) or the device (uint8 frames at the files' size) resizes."""
    import predict_spnet
    from spnet_amd import config as cf
    from spnet_amd import fake_espi as F
    from spnet_amd import models as M
    from spnet_amd import utils as U
    assert cf.model_type == "monolithic"
    data = tmp_path / "frames"
    F.write_dataset(str(data) + "/", 16, seed=6)
    files = sorted(str(p) for p in data.glob("*.png"))
    X_native, dims = U.build_X(16, files, force_dim=331, grayscale=True, as_uint8=True, device_resize=True)
    assert X_native.shape == (16, 384, 512, 1) and X_native.dtype == np.uint8 and dims == (384, 512, 1)
    with pytest.raises(ValueError):
        U.build_X(16, files, force_dim=331, grayscale=True, device_resize=True)
    model = M.Model((331, 331, 1), Y0size=576, seed=8)
    csv = {}
    for flag in (False, True):
        log = str(tmp_path / ("log_%d" % flag)) + "/"
        predict_spnet.predict_network(datapath=str(data), log_dir=log, batch_size=8, model=model, device_resize=flag)
        csv[flag] = open(log + "hawley_spnet.csv", "rb").read()
    assert len(csv[False]) > 0 and csv[True] == csv[False]


# beyond the issue's cases: more than one column tile (OW > 512: clipped store groups at the tile seam), sizes up to the
# ABI's 2048, strong reductions whose bands need more source rows / columns than one LDS chunk holds, one-pixel axes
WIDE_CASES = [((40, 1100), (23, 700)), ((2048, 37), (3, 37)), ((5, 2048), (5, 3)), ((9, 700), (11, 2048)),
              ((1, 1), (7, 5)), ((300, 300), (1, 1))]


@pytest.mark.parametrize("src,dst", WIDE_CASES)
def test_kernel_equals_pillow_on_wide_and_extreme_sizes(src, dst):
    import torch
    from spnet_amd import fake_espi as F
    from spnet_amd import resize as RZ
    (H, W), (OH, OW) = src, dst
    X = frames(3, H, W, seed=7)
    ref = np.stack([pil_resize(a, OH, OW) for a in X])
    u = torch.full((3, OH, OW), 77, dtype=torch.uint8, device="cuda")
    f = torch.full((3, OH, OW, 1), float("nan"), device="cuda")
    RZ.resize_u8_device(torch.from_numpy(X).cuda(), (OH, OW), out_f=f, out_u8=u)
    got = u.cpu().numpy()
    assert np.array_equal(got, ref), "%d pixels differ (%s -> %s)" % (int((got != ref).sum()), src, dst)
    assert np.array_equal(f.cpu().numpy(), F.to_network_input(ref))


def test_generate_device_resizes_the_band_pass_mixed_frames(tmp_path):
    """generate_device(size=331, bandpass_real=...): the resized frames are Pillow's resize of the MIXED uint8 frames the
    same call returns at the native size."""
    import os
    from spnet_amd import fake_espi as F
    rng = np.random.RandomState(4)
    d = str(tmp_path / "real")
    os.makedirs(d)
    r, c = np.mgrid[0:F.IM_H, 0:F.IM_W]
    for i in range(3):
        a = 110 + 60 * np.cos(2 * np.pi * (rng.uniform(1, 4) * r / F.IM_H + rng.uniform(1, 4) * c / F.IM_W)) \
            + rng.normal(0, 20, r.shape)
        Image.fromarray(np.clip(np.rint(a), 0, 255).astype(np.uint8)).save(os.path.join(d, "real_%02d.png" % i))
    _, lab0, U0 = F.generate_device(5, seed=3, want_u8=True, bandpass_real=d, chunk=4)
    X1, lab1, U1 = F.generate_device(5, seed=3, want_u8=True, bandpass_real=d, chunk=4, size=331)
    ref = np.stack([pil_resize(a, 331, 331) for a in U0.cpu().numpy()])
    assert lab1 == lab0 and np.array_equal(U1.cpu().numpy(), ref)
    assert np.array_equal(X1.cpu().numpy(), F.to_network_input(ref))
    X2, _ = F.generate_device(5, seed=3, bandpass_real=d, chunk=4, size=331)
    assert np.array_equal(X2.cpu().numpy(), X1.cpu().numpy())


def test_acceptance_inputs_are_the_host_resize_of_the_generated_frames():
    """tools/acceptance_run.make_set (device resize) gives the frames its former host path gave: PIL's resize of the
    one-channel 'L' image of each generated uint8 frame -- the same bytes as channel 0 of the codec's RGB call."""
    import importlib.util
    import os
    import torch
    from spnet_amd import fake_espi as F
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("acceptance_run", os.path.join(root, "tools", "acceptance_run.py"))
    AR = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(AR)
    X, Y = AR.make_set(6, 17, torch.device("cuda:0"), 331)
    _, _, U = F.generate_device(6, seed=17, device="cuda:0", want_u8=True)
    want = np.stack([np.asarray(Image.fromarray(a).resize((331, 331), Image.LANCZOS), dtype=np.uint8) for a in U.cpu().numpy()])
    assert X.shape == (6, 331, 331, 1) and Y.shape[0] == 6
    assert np.array_equal(X, F.to_network_input(want))
