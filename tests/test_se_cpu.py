"""The SE-ResNet models on the CPU: timm's `seresnetNN` state-dict layout, the registry names, and the reference
path against a hand-written torch Squeeze-and-Excitation block chain."""
import torch
import torch.nn.functional as F

from cs744_distributed_data_parallel_amd.models import get_model, resnet50, seresnet18, seresnet50


def test_seresnet50_layout_and_registry():
    plain, se = resnet50().state_dict(), seresnet50().state_dict()
    extra = {k: tuple(v.shape) for k, v in se.items() if k not in plain}
    assert set(plain) <= set(se) and all(se[k].shape == plain[k].shape for k in plain)
    want = {}
    for layer, (blocks, planes) in enumerate(zip([3, 4, 6, 3], [64, 128, 256, 512]), 1):
        C = 4 * planes
        for b in range(blocks):
            pre = f"layer{layer}.{b}.se."
            want.update({pre + "fc1.weight": (C // 16, C, 1, 1), pre + "fc1.bias": (C // 16,),
                         pre + "fc2.weight": (C, C // 16, 1, 1), pre + "fc2.bias": (C,)})
    assert extra == want and len(want) == 4 * 16
    assert sum(p.numel() for p in seresnet50().parameters()) == 28_088_024 == 25_557_032 + 2_530_992
    a, b = get_model("seresnet50"), get_model("resnet50_se")
    assert type(a) is type(b) and a.state_dict().keys() == b.state_dict().keys() == se.keys()


def _se_basic_block(blk, x):
    """A BasicBlock with Squeeze-and-Excitation written out in torch ops from its parameters."""
    bn = lambda m, t: F.batch_norm(t, None, None, m.weight, m.bias, True, 0.0, m.eps)
    out = F.relu(bn(blk.bn1, F.conv2d(x, blk.conv1.weight, None, blk.stride, 1)))
    u = bn(blk.bn2, F.conv2d(out, blk.conv2.weight, None, 1, 1))
    z = u.mean((2, 3))
    h = F.relu(z @ blk.se.fc1.weight.flatten(1).t() + blk.se.fc1.bias)
    g = torch.sigmoid(h @ blk.se.fc2.weight.flatten(1).t() + blk.se.fc2.bias)
    idt = x
    if blk.downsample is not None:
        idt = bn(blk.downsample[1], F.conv2d(x, blk.downsample[0].weight, None, blk.stride))
    return F.relu(u * g[:, :, None, None] + idt)


def test_seresnet18_reference_path_matches_hand_written_chain():
    torch.manual_seed(0)
    m = seresnet18(num_classes=10).double().train()
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)
    t = F.max_pool2d(F.relu(F.batch_norm(F.conv2d(x, m.conv1.weight, None, 2, 3), None, None, m.bn1.weight,
                                         m.bn1.bias, True, 0.0, m.bn1.eps)), 3, 2, 1)
    for layer in (m.layer1, m.layer2, m.layer3, m.layer4):
        for blk in layer:
            t = _se_basic_block(blk, t)
    want = F.linear(t.mean((2, 3)), m.fc.weight, m.fc.bias)
    torch.testing.assert_close(m(x), want, rtol=1e-10, atol=1e-12)
