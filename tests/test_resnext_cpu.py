"""ResNeXt / Wide ResNet on the CPU: the factories, torchvision's parameter counts, keys and shapes, and the
reference composition of a grouped conv block."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from cs744_distributed_data_parallel_amd.models import get_model
from cs744_distributed_data_parallel_amd.models.resnet import BasicBlock, Bottleneck, ResNet
from cs744_distributed_data_parallel_amd.ops import functional as CF

NAMES = ["resnext50_32x4d", "resnext101_32x8d", "resnext101_64x4d", "wide_resnet50_2", "wide_resnet101_2"]


@pytest.mark.parametrize("name,params", [("resnext50_32x4d", 25028904), ("wide_resnet50_2", 68883240),
                                         ("seresnext50_32x4d", None)])
def test_factories_build(name, params):
    net = get_model(name)
    assert params is None or sum(p.numel() for p in net.parameters()) == params
    groups = 32 if "resnext" in name else 1
    assert net.layer1[0].conv2.groups == groups and net.layer1[0].conv2.weight.shape == (128, 128 // groups, 3, 3)
    assert ("se" in name) == hasattr(net.layer1[0], "se")


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_is_torchvisions(name):
    tvm = pytest.importorskip("torchvision.models")
    ours, theirs = get_model(name).state_dict(), getattr(tvm, name)().state_dict()
    assert {k: tuple(v.shape) for k, v in ours.items()} == {k: tuple(v.shape) for k, v in theirs.items()}


def test_basic_block_refuses_groups():
    with pytest.raises(ValueError):
        ResNet(BasicBlock, [1, 1, 1, 1], groups=2)
    with pytest.raises(ValueError):
        ResNet(BasicBlock, [1, 1, 1, 1], width_per_group=128)


def test_cpu_forward_is_the_torch_composition():
    torch.manual_seed(3)
    net = ResNet(Bottleneck, [1, 1, 1, 1], groups=4, width_per_group=8, num_classes=10).eval()
    x = torch.randn(2, 3, 32, 32)
    blk = net.layer2[0]
    assert blk.conv2.groups == 4 and blk.conv2.weight.shape == (64, 16, 3, 3)
    h = torch.randn(2, 64, 6, 6)
    want = F.relu(F.batch_norm(F.conv2d(h, blk.conv2.weight, None, 2, 1, 1, 4), blk.bn2.running_mean,
                               blk.bn2.running_var, blk.bn2.weight, blk.bn2.bias, False, 0.0, blk.bn2.eps))
    assert torch.equal(CF.conv_bn_act(h, blk.conv2, blk.bn2, relu=True), want)
    # the whole model against the same modules chained by hand
    y = net.maxpool(F.relu(net.bn1(net.conv1(x))))
    for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
        b = layer[0]
        out = F.relu(b.bn1(b.conv1(y)))
        out = b.bn3(b.conv3(F.relu(b.bn2(F.conv2d(out, b.conv2.weight, None, b.conv2.stride, 1, 1, 4)))))
        y = F.relu(out + b.downsample(y))
    assert torch.allclose(net(x), net.fc(y.mean((2, 3))), rtol=1e-5, atol=1e-6)
