"""MobileNetV1 on the CPU: the architecture of Howard et al.'s Table 1, the registry, and the reference path."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from cs744_distributed_data_parallel_amd.models import INPUT_SHAPES, get_model, mobilenet_v1, mobilenet_v1_025
from cs744_distributed_data_parallel_amd.ops import functional as CF

WIDTHS = [64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 512, 1024, 1024]
STRIDES = [1, 2, 1, 2, 1, 2, 1, 1, 1, 1, 1, 2, 1]


def test_parameter_count_and_state_dict_keys():
    net = mobilenet_v1()
    assert sum(p.numel() for p in net.parameters()) == 4231976
    assert sum(p.numel() for n, p in net.named_parameters() if not n.startswith("fc.")) == 3206976
    bn = ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    want = ["stem.0.weight"] + [f"stem.1.{k}" for k in bn]
    for i in range(13):
        want += [f"blocks.{i}.dw.weight"] + [f"blocks.{i}.bn1.{k}" for k in bn]
        want += [f"blocks.{i}.pw.weight"] + [f"blocks.{i}.bn2.{k}" for k in bn]
    assert list(net.state_dict()) == want + ["fc.weight", "fc.bias"]


@pytest.mark.parametrize("make,mult", [(mobilenet_v1, 1.0), (mobilenet_v1_025, 0.25)])
def test_block_widths_and_strides(make, mult):
    net = make()
    assert net.stem[0].out_channels == int(32 * mult) and net.stem[0].stride == (2, 2)
    assert [b.pw.out_channels for b in net.blocks] == [int(c * mult) for c in WIDTHS]
    assert [b.dw.stride[0] for b in net.blocks] == STRIDES
    assert all(b.dw.groups == b.dw.in_channels == b.dw.out_channels and b.dw.bias is None for b in net.blocks)
    assert net.fc.in_features == int(1024 * mult)


def test_registry_spellings():
    assert type(get_model("mobilenet_v1")) is type(get_model("mobilenetv1_050"))
    assert get_model("mobilenetv1_050").fc.in_features == 512
    assert INPUT_SHAPES["mobilenetv1"] == INPUT_SHAPES["mobilenetv1050"] == ((3, 224, 224), 1000)


def test_small_forward_is_finite():
    torch.manual_seed(0)
    net = mobilenet_v1_025(num_classes=10, small_input=True)
    assert net.stem[0].stride == (1, 1)
    out = net(torch.randn(2, 3, 32, 32))
    assert out.shape == (2, 10) and torch.isfinite(out).all()


def test_out_of_domain_depthwise_is_torch_conv():
    torch.manual_seed(0)
    x = torch.randn(2, 6, 9, 7)
    for conv in (nn.Conv2d(6, 6, 5, 1, 2, groups=6), nn.Conv2d(6, 12, 3, 2, 1, groups=6, dilation=1),
                 nn.Conv2d(6, 6, 3, 1, 2, groups=6, dilation=2)):
        assert not CF._dwconv_native(x, conv)
        want = F.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding, conv.dilation, conv.groups)
        assert torch.equal(CF.conv2d(x, conv), want)
