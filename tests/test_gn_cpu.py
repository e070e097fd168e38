"""The GroupNorm ResNets on the CPU: torchvision's `norm_layer=GroupNorm` state-dict layout, the registry names,
the constructor's checks, and `CF.group_norm_act` off the native path."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from cs744_distributed_data_parallel_amd.models import get_model, resnet18_gn, resnet50, resnet50_gn
from cs744_distributed_data_parallel_amd.ops import functional as CF


def test_resnet50_gn_layout_and_registry():
    gn, plain = get_model("resnet50_gn"), resnet50().state_dict()
    stat = ("running_mean", "running_var", "num_batches_tracked")
    want = {k: v.shape for k, v in plain.items() if not k.endswith(stat)}
    assert {k: v.shape for k, v in gn.state_dict().items()} == want
    assert not list(gn.buffers())
    norms = [m for m in gn.modules() if isinstance(m, (nn.GroupNorm, nn.BatchNorm2d))]
    assert len(norms) == 53 and all(isinstance(m, nn.GroupNorm) and m.num_groups == 32 for m in norms)
    assert get_model("resnet50gn").state_dict().keys() == gn.state_dict().keys()
    assert get_model("resnet18_gn", gn_groups=16).layer1[0].bn1.num_groups == 16


def test_zero_init_residual_zeroes_each_blocks_last_norm():
    for net, last in ((resnet50_gn(zero_init_residual=True), "bn3"), (resnet18_gn(zero_init_residual=True), "bn2")):
        for name, m in net.named_modules():
            if isinstance(m, nn.GroupNorm):
                assert bool((m.weight == 0).all()) == name.endswith("." + last), name


@pytest.mark.parametrize("kw", [dict(gn_groups=48), dict(gn_groups=0), dict(se=True)])
def test_bad_arguments_raise(kw):
    with pytest.raises(ValueError):
        resnet18_gn(**kw)


@pytest.mark.parametrize("C,G", [(12, 4), (64, 32)])  # Cg = 3 (straddles a channel quad) and the plain path
def test_group_norm_act_off_the_native_path(C, G):
    torch.manual_seed(C)
    y, r = torch.randn(3, C, 5, 4, dtype=torch.float64), torch.randn(3, C, 5, 4, dtype=torch.float64)
    w, b = torch.randn(C, dtype=torch.float64), torch.randn(C, dtype=torch.float64)
    s = torch.tensor([1.25, 0.0, 1.25], dtype=torch.float64)
    gn = F.group_norm(y, G, w, b, 1e-5)
    torch.testing.assert_close(CF.group_norm_act(y, w, b, G), F.relu(gn), rtol=0, atol=0)
    torch.testing.assert_close(CF.group_norm_act(y, w, b, G, relu=False, residual=r), gn + r, rtol=0, atol=0)
    torch.testing.assert_close(CF.group_norm_act(y, w, b, G, residual=r, drop_scale=s),
                               F.relu(gn * s.view(-1, 1, 1, 1) + r), rtol=0, atol=0)
    with pytest.raises(ValueError):
        CF.group_norm_act(y, w, b, G, drop_scale=s)
