"""Depthwise 3x3 convolution on the GPU (csrc/kernels/dwconv.hip): the three ops against float64
`F.conv2d(..., groups=C)` under the project's fp32 dot-product bound, the fused conv -> BN -> ReLU block and
`conv_gn_act` with a depthwise conv, and one training step of a small MobileNetV1 against the float64 reference path.

The ops are held to `_gemm_util.fp32_bound` (K = 9 for y and dx, N P Q for dw); the block and the step to 4 x what the
same composition in float32 torch on the CPU misses float64 by, a block tensor plus 1e-6 of its scale
(test_gconv_gpu.py's criterion)."""
import copy
import functools
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _gemm_util import check_bound, cl, lib, make_data

pytestmark = pytest.mark.gpu

# (N, C, H, W, stride); below 64 channels a workgroup is 32 channels x 128 rows, from 64 on 64 channels x 64 rows
CASES = [
    (2, 8, 7, 5, 1),     # channel block not filled, odd map, row-tile tail
    (2, 8, 7, 5, 2),     # stride 2 on an odd map (P, Q = 4, 3), parity at the border
    (3, 68, 9, 9, 2),    # a full 64-channel block plus one quad; M = 75: two 64-row tiles
    (2, 16, 12, 20, 1),  # M = 480: four 128-row tiles and several weight-gradient chunks
    (1, 64, 1, 1, 1),    # a 1x1 map: eight of nine taps are padding
    (2, 4, 2, 3, 2),     # one quad, a map smaller than the filter
    (2, 32, 9, 9, 1),    # a full 32-channel block; M = 162: a 128-row tile and its tail
]


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """fp32 CPU inputs and the float64 y, dx, dw of one depthwise conv with the sum_i |a_i||b_i| of each element.
    Computed once per (case, kind); read only."""
    N, C, H, W, s = case
    gen = torch.Generator().manual_seed(11)
    x = make_data(kind, (N, C, H, W), gen)
    w = (torch.randn(C, 1, 3, 3, generator=gen) / 3.0).float()
    conv = lambda a, b: F.conv2d(a, b, None, s, 1, 1, C)
    xd, wd = x.double().requires_grad_(), w.double().requires_grad_()
    y = conv(xd, wd)
    gy = make_data(kind, tuple(y.shape), gen)
    y.backward(gy.double())
    xa, wa = xd.detach().abs().requires_grad_(), wd.detach().abs().requires_grad_()
    abs_y = conv(xa, wa)
    abs_y.backward(gy.double().abs())
    return types.SimpleNamespace(x=x, w=w, gy=gy, y=y.detach(), dx=xd.grad, dw=wd.grad, abs_y=abs_y.detach(),
                                 abs_dx=xa.grad, abs_dw=wa.grad, K=(9, 9, y.numel() // C))


def run_ops(case, kind, out=None, accumulate=False):
    N, C, H, W, s = case
    r, L = reference(case, kind), lib()
    x, w, gy = cl(r.x.cuda()), cl(r.w.cuda()), cl(r.gy.cuda())
    y = L.dwconv2d_fwd(x, w, None, s, 1, False)[0]
    dx = L.dwconv2d_dgrad(gy, w, [N, C, H, W], s, 1, None)
    dw = L.dwconv2d_wgrad(gy, x, list(w.shape), s, 1, out, accumulate)
    return y, dx, dw


@pytest.mark.parametrize("kind", ["gauss", "heavy"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_ops_match_fp64(case, kind):
    r = reference(case, kind)
    y, dx, dw = run_ops(case, kind)
    ratios = [check_bound("y", y, r.y, r.abs_y, r.K[0]), check_bound("dx", dx, r.dx, r.abs_dx, r.K[1]),
              check_bound("dw", dw, r.dw, r.abs_dw, r.K[2])]
    print("dwconv ops {} {}: |err|/bound y {:.3f} dx {:.3f} dw {:.3f}".format(case, kind, *ratios))


def test_wgrad_accumulates_and_calls_repeat_bitwise():
    case, kind = CASES[2], "heavy"
    r = reference(case, kind)
    first, again = run_ops(case, kind), run_ops(case, kind)
    for name, a, b in zip(("y", "dx", "dw"), first, again):
        assert torch.equal(a, b), f"{name}: a second call differs bitwise"
    base = make_data("gauss", tuple(r.w.shape), torch.Generator().manual_seed(3))
    slot = cl(base.cuda())
    dw = run_ops(case, kind, out=slot, accumulate=True)[2]
    assert dw.data_ptr() == slot.data_ptr()
    # the slot's own add rounds once more: 2^-24 |base + dw| <= 2^-24 (|base| + sum |a||b|), with a factor 2
    check_bound("dw += ", dw, r.dw + base.double(), r.abs_dw, r.K[2], extra=2.0 ** -23 * (base.double().abs() + r.abs_dw))


# ------------------------------------------------------------------------------ the fused block
def block_tensors(case, norm, device, dtype):
    """(out, dx, dW, dgamma, dbeta[, running mean, running var]) of conv -> norm -> ReLU in training mode."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    N, C, H, W, s = case
    r = reference(case, "gauss")
    conv = nn.Conv2d(C, C, 3, s, 1, groups=C, bias=False)
    nm = nn.BatchNorm2d(C) if norm == "bn" else nn.GroupNorm(C // 4, C)
    with torch.no_grad():
        conv.weight.copy_(r.w)
        gen = torch.Generator().manual_seed(5)
        nm.weight.copy_(1.0 + 0.5 * torch.randn(C, generator=gen))
        nm.bias.copy_(torch.randn(C, generator=gen))
    conv, nm = conv.to(device=device, dtype=dtype), nm.to(device=device, dtype=dtype)
    x = r.x.to(device=device, dtype=dtype, copy=True)  # (a copy: the reference stays as it is)
    if device == "cuda":
        x = cl(x)
    x.requires_grad_()
    fn = CF.conv_bn_act if norm == "bn" else CF.conv_gn_act
    out = fn(x, conv, nm, relu=True)
    out.backward(r.gy.to(device=device, dtype=dtype))
    ts = [out, x.grad, conv.weight.grad, nm.weight.grad, nm.bias.grad]
    ts += [nm.running_mean, nm.running_var] if norm == "bn" else []
    return [t.detach().double().cpu().reshape(-1) for t in ts]


@pytest.mark.parametrize("case,norm", [(CASES[1], "bn"), (CASES[2], "bn"), (CASES[3], "gn")],
                         ids=["bn_s2_odd", "bn_c68_s2", "gn_c16"])
def test_block_matches_fp64(case, norm):
    ref = block_tensors(case, norm, "cpu", torch.float64)
    f32 = block_tensors(case, norm, "cpu", torch.float32)
    got = block_tensors(case, norm, "cuda", torch.float32)
    bad = []
    for name, a, b, c in zip(("out", "dx", "dW", "dgamma", "dbeta", "running_mean", "running_var"), got, ref, f32):
        err, yard, scale = (a - b).abs().max().item(), (c - b).abs().max().item(), b.abs().max().item()
        print(f"dwconv block {norm} {name}: kernel err {err:.3e}  fp32 torch err {yard:.3e}")
        if not err <= 4.0 * yard + 1e-6 * scale:
            bad.append((name, err, yard))
    assert not bad, bad


# ------------------------------------------------------------------------------ one training step
def step(ref, x, y, device, dtype):
    net = copy.deepcopy(ref).to(device=device, dtype=dtype)
    xin = x.to(device=device, dtype=dtype)
    if device == "cuda":
        xin = cl(xin)
    loss = F.cross_entropy(net(xin), y.to(device))
    loss.backward()
    return loss.item(), [p.grad.double().cpu() for p in net.parameters()]


def step_error(got, want):
    worst = abs(got[0] - want[0]) / abs(want[0])
    return max([worst] + [((g - g64).norm() / g64.norm()).item() for g, g64 in zip(got[1], want[1])])


def test_mobilenet_step_matches_reference():
    """mobilenet_v1_025(num_classes=10, small_input=True): 13 depthwise convs of 8 .. 256 channels, four of them
    stride 2; max(relative loss error, worst parameter gradient's |g - g64|_2 / |g64|_2) held to 4 x the float32
    CPU reference path's. At 2 x 3 x 32 x 32 with the stride-1 stem the deepest maps are 2 x 2, so every BatchNorm
    sees at least 8 values per channel and the float64 reference is well conditioned."""
    from cs744_distributed_data_parallel_amd.models import mobilenet_v1_025

    torch.manual_seed(7)
    ref = mobilenet_v1_025(num_classes=10, small_input=True)
    x, y = torch.randn(2, 3, 32, 32), torch.tensor([3, 8])
    want = step(ref, x, y, "cpu", torch.float64)
    yard = step_error(step(ref, x, y, "cpu", torch.float32), want)
    err = step_error(step(ref, x, y, "cuda", torch.float32), want)
    print(f"dwconv step: native {err:.3e}  fp32 cpu {yard:.3e}  ratio {err / yard:.2f}")
    assert err <= 4.0 * yard
