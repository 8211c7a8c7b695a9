"""DenseNet121 backbone: structure, parameter layout and layer table (no GPU needed)."""
import numpy as np

from tests.helpers import densenet_ref as R


def _n(shape):
    return int(np.prod(shape))


def test_densenet_parameter_counts():
    from spnet_amd.densenet import densenet_param_specs
    specs = densenet_param_specs()
    assert sum(_n(s) for _, s, _, _ in specs) == 7037504                    # keras DenseNet121(include_top=False)
    assert sum(_n(s) for _, s, t, _ in specs if not t) == 83648
    assert sum(_n(s) for _, s, t, _ in specs if t) == 6953856


def test_densenet_totals_and_output_planes():
    from spnet_amd.densenet import densenet_out_hw
    from spnet_amd.engine import param_specs
    assert densenet_out_hw(331, 331) == (5, 5)
    assert densenet_out_hw(384, 512) == (6, 8)
    assert sum(_n(s) for _, s, _, _ in param_specs(331, 331, backbone="DenseNet121")) == 21783905
    assert sum(_n(s) for _, s, _, _ in param_specs(384, 512, backbone="DenseNet121")) == 35349857


def test_densenet_conv_and_bn_names_in_keras_order():
    from spnet_amd.densenet import densenet_param_specs
    specs = densenet_param_specs()
    convs = [n[:-len("/kernel")] for n, _, _, _ in specs if n.endswith("/kernel")]
    bns = [n[:-len("/gamma")] for n, _, _, _ in specs if n.endswith("/gamma")]
    assert len(convs) == 120 and len(bns) == 121
    ref = R.layer_list()
    assert convs == [n for n, k in ref if k == "conv"]
    assert bns == [n for n, k in ref if k == "bn"]
    names = {n for n, _, _, _ in specs}
    for n in ("conv1/conv/kernel", "conv1/bn/gamma", "conv2_block1_0_bn/moving_mean", "conv4_block24_2_conv/kernel",
              "pool3_conv/kernel", "bn/beta"):
        assert n in names
    shapes = dict((n, s) for n, s, _, _ in specs)
    assert shapes["conv4_block24_1_conv/kernel"] == (1, 1, 256 + 23 * 32, 128)
    assert shapes["pool4_conv/kernel"] == (1, 1, 1024, 512)


def test_densenet_l2_prefix_head_first():
    from spnet_amd.engine import param_layout, param_specs
    specs = param_specs(384, 512, backbone="DenseNet121")
    lay = param_layout(384, 512, backbone="DenseNet121")
    l2 = [n for n, _, _, r in specs if r]
    assert len(l2) == 3 + 120 + 1
    assert all(n.endswith("/kernel") for n in l2)
    p = lay["p_off"]
    assert p["FinalOutput/kernel"][0] == 0
    assert max(p[n][0] + p[n][1] for n in l2) <= lay["l2_n"]
    assert min(off for n, (off, _, _) in p.items() if n not in l2) >= lay["l2_n"]


def test_densenet_layer_table_and_freeze_mapping():
    from spnet_amd.densenet import densenet_layers
    from spnet_amd.models import keras_layer_table
    t = keras_layer_table("DenseNet121")
    # 13 stem entries + 425 Keras 2.1.3 layers (the closing ReLU of later releases is not there)
    assert len(t) == 13 + 425
    assert [n for n, _ in t[13:]] == [n for n, _ in R.layer_list()]
    assert [k for _, k, _ in densenet_layers()] == [k for _, k in R.layer_list()]
    # freezing the first 15 entries = the stem + ZeroPadding2D + conv1/conv: conv1/bn stays trainable
    frozen = [p for _, ps in t[:15] for p in ps]
    assert "conv1/conv" in frozen and "conv1/bn" not in frozen
    from spnet_amd.engine import param_layout
    lay = param_layout(331, 331, backbone="DenseNet121")
    hit = [n for n in lay["p_off"] if n.split("/")[0] in frozen or n.rsplit("/", 1)[0] in frozen]
    assert "conv1/conv/kernel" in hit and "conv1/bn/gamma" not in hit and "conv2d_1/kernel" in hit


def test_densenet_grad_buckets_cover_layout():
    from spnet_amd.densenet import densenet_pnames
    from spnet_amd.engine import param_layout, plan_grad_buckets
    lay = param_layout(384, 512, backbone="DenseNet121")
    stem = [("conv2d_%d" % k, ["conv2d_%d" % k, "batch_normalization_%d" % k], False) for k in (1, 2, 3)]
    nodes = stem + [("densenet", [p.split("/")[0] for p in densenet_pnames()], False), ("FinalOutput", ["FinalOutput"], False)]
    buckets, tail = plan_grad_buckets(lay["p_off"], lay["rest_lo"], lay["n_theta"], nodes)
    cover = np.zeros(lay["n_theta"], dtype=np.int32)
    for lo, hi, _ in buckets:
        cover[lo:hi] += 1
    for lo, hi in tail:
        cover[lo:hi] += 1
    assert (cover == 1).all()
