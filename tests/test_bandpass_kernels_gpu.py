"""The band-pass mix-up kernels (csrc/bandpass.hip) through the C ABI, stage by stage and at every tile edge:
spnet_bandpass_ws, spnet_bandpass_project and spnet_bandpass_apply at the smallest shapes that reach each branch of the
column tiling (256 columns), the row blocking (64 rows) and the documented limits 16 and 2048.

Every comparison is either an equality of bits (the device's sums run in a fixed order) or a comparison with a float64
reference to an a-priori rounding bound derived in tests/helpers/bandpass_ref.py (project_bound, mix_bound, recon_bound),
which tests/test_bandpass_cpu.py shows to hold for a float32 emulation of the kernel's order and to fail for three
one-line bugs.  No constant here was fitted to device output.  Each bounded test prints its largest error / bound.

Window tables of the apply tests are built on the host, so that no projection error can cancel a reconstruction error.
Every workspace is exactly spnet_bandpass_ws floats followed by canaries, checked after every call."""
import numpy as np
import pytest
import torch

from tests.helpers import bandpass_ref as R

pytestmark = pytest.mark.gpu

CANARY, CANARIES = np.float32(-7.25), 64
PATTERN = np.float32(-3.5)
BIG = [(130, 513), (2048, 16)]                       # more than one row block: where in place can go wrong
DTYPE = {0: np.uint8, 1: np.float32, 2: np.float32}


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from spnet_amd import _lib
    return _lib


def st():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def i32(a):
    return None if a is None else dev(np.asarray(a, np.int32))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


class Work:
    """exactly spnet_bandpass_ws(N, H, W) floats, then canaries"""

    def __init__(self, L, N, H, W):
        self.n = int(L.spnet_bandpass_ws(N, H, W))
        nb = -(-H // R.BP_RB)
        assert self.n == N * (nb * 512 + 512 + nb * 2 + 1)
        self.t = torch.full((self.n + CANARIES,), float(CANARY), device="cuda")
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.t[self.n:] == float(CANARY)).all().item())


def as_kind(pix, kind):
    """integer pixel values [N,H,W] as the frames of x_kind 0 / 1; x_kind 2 takes network values, see network()"""
    return np.ascontiguousarray(pix, DTYPE[kind])


def network(rs, shape):
    """x_kind 2 frames and the float32 pixel values the kernel makes of them"""
    v = rs.uniform(-1, 1, shape).astype(np.float32)
    return v, R.to_pixel32(v)


def project(L, x, kind, flip=None):
    """x: host frames [N,H,W] of the kind's dtype -> win [N,16,16,2] (numpy)"""
    N, H, W = x.shape
    xd, fd, ws = dev(x), i32(flip), Work(L, N, H, W)
    win = torch.full((N, 16, 16, 2), float(PATTERN), device="cuda")
    L.spnet_bandpass_project(xd.data_ptr(), kind, N, H, W, L.ptr(fd), win.data_ptr(), ws.ptr, st())
    torch.cuda.synchronize()
    assert ws.intact()
    return win.cpu().numpy()


def apply(L, x, kind, table, row, s, f_kind=0, want_u8=False, sel=None, N=None):
    """out of place: x host frames [n_src,H,W] -> out_f [n_src,H,W] (NaN where nothing was written) and, with want_u8,
    out_u8 (0xAB where nothing was written)"""
    n_src, H, W = x.shape
    N = n_src if N is None else N
    xd, td, rd, sd, seld, ws = dev(x), dev(table), i32(row), dev(np.asarray(s, np.float32)), i32(sel), Work(L, N, H, W)
    of = torch.full((n_src, H, W), float("nan"), device="cuda")
    ou = torch.full((n_src, H, W), 0xAB, dtype=torch.uint8, device="cuda") if want_u8 else None
    L.spnet_bandpass_apply(xd.data_ptr(), kind, L.ptr(seld), n_src, N, H, W, td.data_ptr(), len(table), rd.data_ptr(),
                           sd.data_ptr(), of.data_ptr(), f_kind, L.ptr(ou), ws.ptr, st())
    torch.cuda.synchronize()
    assert ws.intact() and same(xd.cpu().numpy(), x)            # the input is read only
    return (of.cpu().numpy(), ou.cpu().numpy()) if want_u8 else of.cpu().numpy()


def apply_in_place(L, x, kind, table, row, s, f_kind=0, sel=None, N=None):
    """out_f == x (fp32 kinds) or out_u8 == x (uint8) -> the frames afterwards"""
    n_src, H, W = x.shape
    N = n_src if N is None else N
    xd, td, rd, sd, seld, ws = dev(x), dev(table), i32(row), dev(np.asarray(s, np.float32)), i32(sel), Work(L, N, H, W)
    of, ou = (None, xd.data_ptr()) if kind == 0 else (xd.data_ptr(), None)
    L.spnet_bandpass_apply(xd.data_ptr(), kind, L.ptr(seld), n_src, N, H, W, td.data_ptr(), len(table), rd.data_ptr(),
                           sd.data_ptr(), of, f_kind, ou, ws.ptr, st())
    torch.cuda.synchronize()
    assert ws.intact()
    return xd.cpu().numpy()


def complex2(F):
    return np.stack([F.real, F.imag], -1)


def threes(items):
    """the items three at a time, the last group filled up from the front: every launch has N = 3"""
    items = list(items)
    return [[items[(i + j) % len(items)] for j in range(3)] for i in range(0, len(items), 3)]


# ---- spnet_bandpass_project --------------------------------------------------------------------------------------------
def impulse_value(kind):
    """(the value written into the frame, the pixel value it stands for)"""
    if kind != 2:
        return R.IMPULSE, R.IMPULSE
    v = R.network_value_of(R.IMPULSE)
    return (float(v), R.IMPULSE) if v is not None else (1.0, 255.0)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_project_impulses_at_every_edge(L, H, W, kind):
    """one pixel of value A: F[k][l] is ONE product of two twiddles times A, so a wrong phase anywhere in the walk shows at
    full scale; the bound is a few ulp of A.  Every flip behaviour (-1, 0, 1, and 2 and 7 = not flipped) at every position."""
    value, A = impulse_value(kind)
    zero = -1.0 if kind == 2 else 0.0
    codes = [-1, 0, 1, 2, 7]
    worst, ref = 0.0, {}
    for g, group in enumerate(threes(R.edge_positions(H, W))):
        x = np.full((3, H, W), zero, DTYPE[kind])
        for n, (r, c) in enumerate(group):
            x[n, r, c] = value
        for turn in range(5):
            flip = [codes[(g + n + turn) % 5] for n in range(3)]
            got = project(L, x, kind, flip).astype(np.float64)
            for n, (r, c) in enumerate(group):
                rr = H - 1 - r if flip[n] in (0, -1) else r
                cc = W - 1 - c if flip[n] in (1, -1) else c
                if (rr, cc) not in ref:
                    t = R.impulse_frame(H, W, rr, cc, A, np.float64)
                    ref[rr, cc] = (complex2(R.window(t)), R.project_bound(t))
                want, bound = ref[rr, cc]
                assert bound.max() <= 5 * np.spacing(np.float32(A))
                worst = max(worst, R.ratio(np.abs(got[n] - want), bound))
    print("bandpass project impulses %dx%d x_kind %d: largest error / bound %.3f" % (H, W, kind, worst))
    assert worst <= 1.0


def dense_case(H, W, kind, seed):
    rs = np.random.RandomState(seed)
    if kind == 2:
        return network(rs, (3, H, W))
    pix = rs.randint(0, 256, (3, H, W)).astype(np.float32)
    return as_kind(pix, kind), pix


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_project_dense_frames(L, H, W, kind):
    x, pix = dense_case(H, W, kind, 100 * H + W + kind)
    worst = 0.0
    for flip in ([1, -1, 0], [2, 7, -1], None):
        got = project(L, x, kind, flip).astype(np.float64)
        for n in range(3):
            t = R.cv2_flip(pix[n].astype(np.float64), 2 if flip is None else flip[n])
            worst = max(worst, R.ratio(np.abs(got[n] - complex2(R.window(t))), R.project_bound(t)))
    print("bandpass project dense %dx%d x_kind %d: largest error / bound %.4f" % (H, W, kind, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_project_exact_identities(L, H, W):
    rs = np.random.RandomState(H + 3 * W)
    pix = rs.randint(0, 256, (3, H, W)).astype(np.float32)
    base = project(L, pix, 1)
    # the flip is an index mapping: the same terms in the same order as the host-flipped frame unflipped
    for flip in ([-1, 0, 1], [1, -1, 0], [0, 1, -1], [2, 7, -5]):
        flipped = np.stack([R.cv2_flip(pix[n], flip[n]) for n in range(3)])
        assert same(project(L, pix, 1, flip), project(L, flipped, 1)), flip
    assert same(project(L, pix, 1, [2, 7, -5]), base)
    assert same(project(L, pix.astype(np.uint8), 0), base)                          # uint8 = fp32 on the same integers
    v, conv = network(rs, (3, H, W))
    assert same(project(L, v, 2, [0, 2, -1]), project(L, conv, 1, [0, 2, -1]))      # network units = the converted pixels
    # a frame's window does not depend on the batch around it
    assert same(project(L, pix[1:2], 1)[0], base[1])
    moved = project(L, np.stack([pix[2], pix[0], pix[1]]), 1, [1, 0, -1])
    assert same(moved[2], project(L, pix[1:2], 1, [-1])[0])


# ---- spnet_bandpass_apply ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("H,W", R.SHAPES)
def test_apply_reconstruction_alone(L, H, W, kind):
    """a constant frame: d = 0 and F = 0 exactly, so G = fl(fl(s T) * fl(1 / (H W))) is known on the host bit for bit and
    out_f is the reconstruction of two to four coefficients at the window's corners and edges, nothing else"""
    table = R.recon_table(H, W)
    s = np.array([1.0, 0.75, 1.5], np.float32)
    row = [2, 0, 1]
    x = as_kind(np.full((3, H, W), 77.0), kind)
    got = apply(L, x, kind, table, row, s).astype(np.float64)
    G = R.mix_g32(table[row], s, np.zeros((3, 16, 16, 2), np.float32), H, W)
    worst = 0.0
    for n in range(3):
        b = R.recon_bound(G[n], np.zeros((H, W)), centred=False)
        assert b["range"] >= 0.25 * b["ymax"] and b["bound"].max() < 1e-2
        worst = max(worst, R.ratio(np.abs(got[n] - b["ref"]), b["bound"]))
    print("bandpass reconstruction alone %dx%d x_kind %d: largest error / bound %.3f" % (H, W, kind, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_apply_impulses_with_a_zero_table(L, H, W):
    """y = d minus its own low-pass, the impulse at every edge position, (0, 0) -- the centring pixel -- among them.  At
    16 x 16 the window is the whole spectrum, y = 0 in exact arithmetic and the bound is infinite: only the launch is tested."""
    zero = np.zeros((2, 16, 16, 2), np.float32)
    worst, finite = 0.0, 0
    for group in threes(R.edge_positions(H, W)):
        x = np.stack([R.impulse_frame(H, W, r, c, dtype=np.uint8) for r, c in group])
        got = apply(L, x, 0, zero, [0, 1, 0], [1.0, 2.0, 0.0]).astype(np.float64)
        assert np.isfinite(got).all()
        for n in range(3):
            b = R.apply_bound(x[n], zero[0], 1.0)
            finite += bool(np.isfinite(b["bound"]).all())
            worst = max(worst, R.ratio(np.abs(got[n] - b["ref"]), b["bound"]))
    assert (finite == 0) == ((H, W) == (16, 16))
    print("bandpass apply impulses %dx%d: largest error / bound %.4f" % (H, W, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_apply_dense_frames_with_a_dense_host_table(L, H, W):
    table = R.dense_table(4, H, W, 5)
    pix = R.dense_frames(3, H, W, 9)
    row = [3, 0, 2]
    worst = 0.0
    for turn in range(3):
        s = np.array([R.S_VALUES[(n + turn) % 3] for n in range(3)], np.float32)
        assert float(s.max()) < 3.0
        got = apply(L, pix, 1, table, row, s).astype(np.float64)
        for n in range(3):
            b = R.apply_bound(pix[n], table[row[n]], s[n])
            worst = max(worst, R.ratio(np.abs(got[n] - b["ref"]), b["bound"]))
    print("bandpass apply dense %dx%d: largest error / bound %.5f" % (H, W, worst))
    assert worst <= 1.0


def to_network32(o):
    """f_kind 1 of the f_kind 0 value: fl(fl(fl(o / 255) - 0.5) * 2)"""
    return (np.asarray(o, np.float32) / np.float32(255.0) - np.float32(0.5)) * np.float32(2.0)


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_apply_exact_identities(L, H, W):
    rs = np.random.RandomState(7 * H + W)
    table = R.dense_table(4, H, W, 6)
    pix = rs.randint(0, 249, (3, H, W)).astype(np.float32)          # + 7 stays below 256
    row, s = [1, 3, 0], np.array([0.5, 2.25, 1.0], np.float32)
    base, u8 = apply(L, pix, 1, table, row, s, want_u8=True)
    assert not np.isnan(base).any() and base.min() == 0.0 and base.max() > 254.0
    assert np.array_equal(u8, R.to_u8(base))                        # out_u8 = rint(out_f) of the same launch
    net = apply(L, pix, 1, table, row, s, f_kind=1)
    assert same(net, to_network32(base))
    b0, u0 = apply(L, pix.astype(np.uint8), 0, table, row, s, want_u8=True)
    assert same(b0, base) and np.array_equal(u0, u8)                # uint8 = fp32 on the same integers
    # network units = the converted pixels.  Regression: the kernel's * 255 once fused with the centring `- f[0][0]` into
    # one FMA, so x_kind 2 centred the unrounded pixel and differed from x_kind 1 in the last bits (at every shape)
    v, conv = network(rs, (3, H, W))
    assert same(apply(L, v, 2, table, row, s), apply(L, conv, 1, table, row, s))
    assert same(apply(L, v, 2, table, row, s, f_kind=1), to_network32(apply(L, conv, 1, table, row, s)))
    # the centring: f and f + 7 project the same d = f - f[0][0]
    assert same(apply(L, (pix + 7).astype(np.uint8), 0, table, row, s), base)
    # a frame's bits: alone, at another batch position, through sel
    assert same(apply(L, pix[1:2], 1, table, row[1:2], s[1:2])[0], base[1])
    order = [2, 0, 1]
    moved = apply(L, pix[order], 1, table, [row[i] for i in order], s[order])
    assert same(moved[order.index(1)], base[1])
    picked = apply(L, pix, 1, table, [row[1]], [s[1]], sel=[1], N=1)
    assert same(picked[1], base[1]) and np.isnan(picked[[0, 2]]).all()


@pytest.mark.parametrize("H,W", BIG)
def test_apply_in_place_equals_out_of_place(L, H, W):
    """another row block of the frame may have overwritten pixel 0 before this block reads it (the p0buf of the kernel): a
    small shift a tolerance would hide, so bits are compared.  Pixel 0 is far from the frame's mean here."""
    rs = np.random.RandomState(H)
    table = R.dense_table(3, H, W, 8)
    row, s = [2, 0, 1], np.array([1.5, 0.0, 2.5], np.float32)
    pix = rs.randint(0, 256, (3, H, W)).astype(np.float32)
    pix[:, 0, 0] = [255, 0, 131]
    assert same(apply_in_place(L, pix, 1, table, row, s), apply(L, pix, 1, table, row, s))
    v, _ = network(rs, (3, H, W))
    v[:, 0, 0] = [1.0, -1.0, 0.03]
    assert same(apply_in_place(L, v, 2, table, row, s, f_kind=1), apply(L, v, 2, table, row, s, f_kind=1))
    u = pix.astype(np.uint8)
    assert np.array_equal(apply_in_place(L, u, 0, table, row, s), apply(L, u, 0, table, row, s, want_u8=True)[1])


@pytest.mark.parametrize("H,W", BIG + [(47, 331)])
def test_apply_sel_scatters_and_leaves_the_other_frames(L, H, W):
    rs = np.random.RandomState(W)
    table = R.dense_table(3, H, W, 4)
    pix = rs.randint(0, 256, (5, H, W)).astype(np.float32)
    sel, row, s = [3, 1], [2, 0], np.array([0.5, 2.0], np.float32)
    packed = apply(L, pix[sel], 1, table, row, s)                   # the compacted run
    out = apply(L, pix, 1, table, row, s, sel=sel, N=2)             # NaN pre-filled
    assert same(out[3], packed[0]) and same(out[1], packed[1])
    assert (bits(out[[0, 2, 4]]) == bits(np.float32(np.nan))).all()
    inpl = apply_in_place(L, pix, 1, table, row, s, sel=sel, N=2)
    assert same(inpl[3], packed[0]) and same(inpl[1], packed[1]) and same(inpl[[0, 2, 4]], pix[[0, 2, 4]])
    u = pix.astype(np.uint8)
    pu = apply(L, u[sel], 0, table, row, s, want_u8=True)[1]
    ou = apply(L, u, 0, table, row, s, want_u8=True, sel=sel, N=2)[1]
    assert np.array_equal(ou[3], pu[0]) and np.array_equal(ou[1], pu[1]) and (ou[[0, 2, 4]] == 0xAB).all()
    iu = apply_in_place(L, u, 0, table, row, s, sel=sel, N=2)
    assert np.array_equal(iu[3], pu[0]) and np.array_equal(iu[1], pu[1]) and np.array_equal(iu[[0, 2, 4]], u[[0, 2, 4]])


def test_apply_clamps_sel_and_row(L):
    H, W, n_src, n_table = 65, 257, 5, 4
    rs = np.random.RandomState(1)
    table = R.dense_table(n_table, H, W, 2)
    pix = rs.randint(0, 256, (n_src, H, W)).astype(np.float32)
    one = np.array([1.25], np.float32)
    # one index per launch: duplicates in sel are not supported
    for given, means in ((-3, 0), (n_src + 5, n_src - 1)):
        want = apply(L, pix, 1, table, [1], one, sel=[means], N=1)
        got = apply(L, pix, 1, table, [1], one, sel=[given], N=1)
        assert same(got, want) and not np.isnan(got[means]).any() and np.isnan(np.delete(got, means, 0)).all()
    for given, means in ((-1, 0), (n_table + 9, n_table - 1)):
        want = apply(L, pix[:3], 1, table, [means, 2, means], np.repeat(one, 3))
        got = apply(L, pix[:3], 1, table, [given, 2, given], np.repeat(one, 3))
        assert same(got, want)
    assert not same(apply(L, pix[:1], 1, table, [0], one), apply(L, pix[:1], 1, table, [n_table - 1], one))


@pytest.mark.parametrize("H,W", R.SHAPES)
def test_constant_frame_with_s_zero_is_all_zeros(L, H, W):
    table = R.dense_table(2, H, W, 3)
    zeros = np.zeros(3, np.float32)
    of, ou = apply(L, np.stack([np.full((H, W), v, np.uint8) for v in (100, 0, 255)]), 0, table, [1, 0, 1], zeros, want_u8=True)
    assert not of.any() and not ou.any() and not np.signbit(of).any()
    of = apply(L, np.stack([np.full((H, W), v, np.float32) for v in (37.5, 0.0, 254.9)]), 1, table, [0, 1, 1], zeros)
    assert not of.any()
    of = apply(L, np.stack([np.full((H, W), v, np.float32) for v in (0.3, -1.0, 1.0)]), 2, table, [0, 1, 1], zeros, f_kind=1)
    assert (of == -1.0).all()                                       # pixel 0 in network units


# ---- the workspace and the rejections ----------------------------------------------------------------------------------
def test_workspace_size(L):
    for N in (0, 1, 3, 64):
        for H, W in R.SHAPES + [(2048, 2048), (63, 16), (129, 700)]:
            nb = -(-H // 64)
            assert L.spnet_bandpass_ws(N, H, W) == N * (nb * 512 + 512 + nb * 2 + 1)
    for bad in (15, 2049):
        assert L.spnet_bandpass_ws(3, bad, 64) == -1 and L.spnet_bandpass_ws(3, 64, bad) == -1
    assert L.spnet_bandpass_ws(-1, 64, 64) == -1


@pytest.mark.parametrize("H,W", [(65, 257), (2048, 16)])
def test_workspace_of_exactly_the_returned_size(L, H, W):
    """project() and apply() put 64 canaries behind exactly spnet_bandpass_ws floats and check them after the call"""
    pix = R.dense_frames(3, H, W, 11)
    project(L, pix, 1, [0, 1, -1])
    apply(L, pix, 1, R.dense_table(2, H, W, 1), [0, 1, 1], [1.0, 2.0, 0.5], want_u8=True)
    apply(L, pix.astype(np.uint8), 0, R.dense_table(2, H, W, 1), [0], [1.0], want_u8=True, sel=[2], N=1)


class Args:
    """valid arguments of both entry points at 3 x 32 x 48, every output and the workspace patterned"""
    N, H, W, n_table = 3, 32, 48, 2

    def __init__(self, L):
        N, H, W = self.N, self.H, self.W
        self.x = dev(R.dense_frames(N, H, W, 0))
        self.x8 = dev(R.dense_frames(N, H, W, 0).astype(np.uint8))
        self.flip, self.sel, self.row = i32([0, 1, -1]), i32([2, 0, 1]), i32([0, 1, 0])
        self.table, self.s = dev(R.dense_table(self.n_table, H, W, 0)), dev(np.ones(N, np.float32))
        self.ws_n = int(L.spnet_bandpass_ws(N, H, W))
        self.outs = dict(win=torch.full((N, 16, 16, 2), float(PATTERN), device="cuda"),
                         out_f=torch.full((N, H, W), float(PATTERN), device="cuda"),
                         out_u8=torch.full((N, H, W), 0xAB, dtype=torch.uint8, device="cuda"),
                         ws=torch.full((self.ws_n,), float(PATTERN), device="cuda"))
        self.before = {k: v.clone() for k, v in self.outs.items()}
        self.frames = {"x": self.x.clone(), "x8": self.x8.clone()}

    def untouched(self):
        torch.cuda.synchronize()
        return (all(torch.equal(self.outs[k], self.before[k]) for k in self.outs)
                and torch.equal(self.x, self.frames["x"]) and torch.equal(self.x8, self.frames["x8"]))

    def project(self, L, **kw):
        a = dict(x=self.x.data_ptr(), x_kind=1, N=self.N, H=self.H, W=self.W, flip=self.flip.data_ptr(),
                 win=self.outs["win"].data_ptr(), ws=self.outs["ws"].data_ptr())
        a.update(kw)
        L.spnet_bandpass_project(a["x"], a["x_kind"], a["N"], a["H"], a["W"], a["flip"], a["win"], a["ws"], st())

    def apply(self, L, **kw):
        a = dict(x=self.x.data_ptr(), x_kind=1, sel=None, n_src=self.N, N=self.N, H=self.H, W=self.W,
                 table=self.table.data_ptr(), n_table=self.n_table, row=self.row.data_ptr(), s=self.s.data_ptr(),
                 out_f=self.outs["out_f"].data_ptr(), f_kind=0, out_u8=self.outs["out_u8"].data_ptr(),
                 ws=self.outs["ws"].data_ptr())
        a.update(kw)
        L.spnet_bandpass_apply(a["x"], a["x_kind"], a["sel"], a["n_src"], a["N"], a["H"], a["W"], a["table"], a["n_table"],
                               a["row"], a["s"], a["out_f"], a["f_kind"], a["out_u8"], a["ws"], st())


def test_rejections_write_nothing(L):
    """every call here is refused by the entry point before anything is launched: no invalid pointer reaches the device"""
    a = Args(L)
    sel = a.sel.data_ptr()
    dims = [dict(H=15), dict(H=2049), dict(W=15), dict(W=2049), dict(H=0), dict(W=-16), dict(N=-1)]
    project = dims + [dict(x_kind=-1), dict(x_kind=3), dict(x=None), dict(win=None), dict(ws=None)]
    applies = dims + [dict(x_kind=-1), dict(x_kind=3), dict(f_kind=-1), dict(f_kind=2), dict(x=None), dict(ws=None),
                      dict(table=None), dict(row=None), dict(s=None), dict(out_f=None, out_u8=None), dict(n_table=0),
                      dict(n_table=-2), dict(sel=sel, n_src=0), dict(sel=sel, n_src=-4)]
    wrong = []
    for name, call, cases in (("project", a.project, project), ("apply", a.apply, applies)):
        for kw in cases:
            try:
                call(L, **kw)
                wrong.append("%s %r: no HipError" % (name, kw))
            except L.HipError as e:
                if not str(e).endswith("hipError_t 1"):
                    wrong.append("%s %r: %s" % (name, kw, e))
            if not a.untouched():
                wrong.append("%s %r: something was written" % (name, kw))
                break
    assert wrong == []
    # the same arguments, valid: both run (the table above refuses for the reason it names, not for another)
    a.project(L)
    a.apply(L, sel=sel)
    torch.cuda.synchronize()
    assert not any(torch.equal(a.outs[k], a.before[k]) for k in a.outs)


def test_nothing_to_do_is_success_and_writes_nothing(L):
    a = Args(L)
    a.project(L, N=0)
    a.apply(L, N=0)
    a.apply(L, N=0, sel=a.sel.data_ptr(), x=a.x8.data_ptr(), x_kind=0)
    assert a.untouched()
