"""The float64 references of tests/helpers/small_kernels_ref.py against what the oracle already has (no GPU needed): the
convolution / stem-head restatements against oracle/torch_ref.py and its autograd, the painters against
numpy_ref.augment_image on seeded frames, and the dropout restatement against its own documented properties."""
import numpy as np
import pytest
import torch

from oracle import numpy_ref as R
from oracle import torch_ref as T
from tests.helpers import small_kernels_ref as S


def _eq64(got, want, scale):
    """two float64 evaluations that sum in different orders: equal to 1e-12 of the size of the terms"""
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * scale


@pytest.mark.parametrize("B,H,W", [(2, 8, 12), (1, 9, 11), (2, 2, 2), (1, 3, 5), (1, 33, 47)])
def test_stem_head_reference_equals_the_unfused_oracle(B, H, W):
    rs = np.random.RandomState(H * 31 + W)
    x = torch.tensor(rs.randn(B, H, W, 1), dtype=torch.float64)
    w = torch.tensor(rs.randn(3, 3, 1, 3), dtype=torch.float64, requires_grad=True)
    p1 = T.avgpool2(T.conv2d(x, w, 1, "same"))
    px = T.avgpool2(x)
    dp = torch.tensor(rs.randn(*p1.shape), dtype=torch.float64)
    p1.backward(dp)
    got1, gotx = S.stem_head_fwd(x[..., 0], w.detach())
    _eq64(got1, p1.detach(), 10.0)
    _eq64(gotx, px[..., 0], 10.0)
    _eq64(S.stem_head_wgrad(x[..., 0], dp), w.grad, 10.0 * B * H * W)


@pytest.mark.parametrize("cin,cout", [(1, 3), (3, 3)])
@pytest.mark.parametrize("H,W", [(7, 9), (1, 4), (12, 5)])
def test_conv3x3_same_reference_and_its_data_gradient(cin, cout, H, W):
    rs = np.random.RandomState(cin + H)
    x = torch.tensor(rs.randn(2, H, W, cin), dtype=torch.float64, requires_grad=True)
    w = torch.tensor(rs.randn(3, 3, cin, cout), dtype=torch.float64)
    y = T.conv2d(x, w, 1, "same")
    dy = torch.tensor(rs.randn(*y.shape), dtype=torch.float64)
    y.backward(dy)
    _eq64(S.conv3x3_same(x.detach(), w), y.detach(), 100.0)
    _eq64(S.conv3x3_same_dgrad(dy, w), x.grad, 100.0)


def test_avgpool2_reference_drops_the_odd_row_and_column():
    x = torch.arange(2 * 5 * 7 * 3, dtype=torch.float64).reshape(2, 5, 7, 3)
    assert torch.equal(S.avgpool2(x), T.avgpool2(x))


@pytest.mark.parametrize("H,W", [(96, 128), (120, 90)])
def test_painters_equal_augment_image(H, W):
    """cutout -> salt & pepper of numpy_ref.augment_image, redone with the painters from the same RNG draws.  The seeds
    are required to cover a frame with no rectangle, one with several, a salted and an unsalted one."""
    seen = set()
    for seed in range(24):
        img0 = np.random.RandomState(1000 + seed).uniform(-1, 1, (H, W, 1)).astype(np.float32)
        want = R.augment_image(img0.copy(), rng=np.random.RandomState(seed))
        rng = np.random.RandomState(seed)
        img = img0[..., 0].copy()
        rects = R.draw_cutout_params(img0.shape, lambda: (np.min(img), np.max(img)), rng)
        S.paint_rects(img, rects)
        sp = R.draw_saltpepper_params(img0.shape, img0.size, rng)
        if sp is not None:
            S.paint_saltpepper(img, sp[0], sp[1], sp[2], sp[3], np.max(img), np.min(img))
        assert np.array_equal(img, want[..., 0]), seed
        seen.add(("rects", min(len(rects), 2)))
        seen.add(("salt", sp is not None))
    assert seen == {("rects", 0), ("rects", 1), ("rects", 2), ("salt", False), ("salt", True)}


def test_painters_order():
    img = np.zeros((4, 5), np.float32)
    S.paint_rects(img, [(0, 3, 0, 3, 1.0), (1, 4, 2, 5, 2.0), (2, 2, 0, 5, 9.0)])      # (the third is empty)
    assert img[0, 0] == 1.0 and img[1, 2] == 2.0 and img[3, 4] == 2.0 and img[3, 0] == 0.0 and not (img == 9.0).any()
    S.paint_saltpepper(img, [0, 0, 1], [0, 0, 1], [1, 3], [1, 0], 7.0, -7.0)
    assert img[0, 0] == 7.0 and img[1, 1] == -7.0 and img[3, 0] == -7.0


def test_selective_sigmoid_reference():
    rs = np.random.RandomState(0)
    y = rs.randn(3, 20)
    s = S.selective_sigmoid_fwd(y, 3, 7)
    cols = np.zeros(20, bool)
    cols[3::7] = True
    assert np.array_equal(s[:, ~cols], y[:, ~cols])
    yt = torch.tensor(y, requires_grad=True)
    st = torch.where(torch.tensor(cols), torch.sigmoid(yt), yt)
    g = rs.randn(3, 20)
    st.backward(torch.tensor(g))
    np.testing.assert_allclose(s, st.detach().numpy(), rtol=1e-14, atol=0)
    np.testing.assert_allclose(S.selective_sigmoid_bwd(s, g, 3, 7), yt.grad.numpy(), rtol=1e-13, atol=0)


def test_dropout_restatement():
    """The documented rule, hash(i * 0x9e3779b9 + seed) >= rate * 2^32 in uint32 arithmetic, on values worked out by
    hand, and the properties that follow from it."""
    def h32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    n, seed = 70000, 0xFFFFFF00                        # (i * golden + seed wraps)
    h = S.dropout_hash(n, seed)
    for i in (0, 1, 2, 255, 256, 69999):
        assert int(h[i]) == h32(i * 0x9E3779B9 + seed)
    assert S.dropout_threshold(0.0) == 0 and S.dropout_keep(n, seed, 0.0).all()
    assert S.dropout_threshold(0.5) == 2 ** 31
    assert S.dropout_threshold(0.1) == 13421773 * 32           # float32(0.1) = 13421773 / 2^27
    assert abs(S.dropout_keep(n, seed, 0.1).mean() - 0.9) < 0.01
    assert (S.dropout_keep(n, seed, 0.1) != S.dropout_keep(n, seed + 1, 0.1)).any()
    for rate in (0.0, 0.1, 0.5):
        assert S.dropout_scale(rate) == np.float32(1.0 / (1.0 - rate))
