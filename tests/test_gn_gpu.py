"""GroupNorm on the GPU (csrc/kernels/gn.hip): `CF.group_norm_act` against the formula

    out = act(s[n] * group_norm(y, G, gamma, beta) + r)

in float64 torch on the CPU, its published act maxima, and one training step of the GroupNorm ResNets against
their float64 reference path.

Tolerances come from references, not from the kernels: a tensor (or a step) may miss fp64 by 4 x what the same
composition in float32 torch on the CPU misses it by (the margin for a different summation order), an op tensor
plus 1e-6 of its scale."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAMES = ("out", "dy", "dgamma", "dbeta", "dr")
# (N, C, G, H, W, relu, residual, drop, offset)
CASES = {
    "cg2_one_chunk": (2, 64, 32, 7, 7, True, True, False, 0.0),
    "cg4_odd_c": (3, 20, 5, 5, 5, True, False, False, 0.0),  # C not a multiple of a wave's quads, odd HW
    "cg1_ragged_chunks": (2, 8, 8, 33, 33, False, False, False, 0.0),  # several chunks, the last one shorter
    "g1_many_images_drop": (17, 32, 1, 3, 3, True, True, True, 0.0),  # more images than the act-max window of 16
    "widest_drop": (2, 2048, 32, 2, 2, True, True, True, 0.0),
    # y = 1000 + randn: float32 torch misses out by 2.0e-4 here (bound 8.1e-4), a plain fp32 sum of squares by
    # 0.76. Without the ReLU: at that error a sign of `out` near 0 would decide the gradients, not the statistics.
    "cancellation": (2, 64, 32, 9, 9, False, False, False, 1000.0),
}


def _CF():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    return CF


def _lib():
    from cs744_distributed_data_parallel_amd import _native

    return _native.lib()


def _inputs(N, C, G, H, W, relu, residual, drop, offset):
    """Seeded fp32 CPU inputs ([y, gamma, beta, r or None], s or None, upstream gradient)."""
    gen = torch.Generator().manual_seed(C + H)
    rn = lambda *s: torch.randn(*s, generator=gen)
    y, gamma, beta, gout = rn(N, C, H, W) + offset, 1.0 + 0.5 * rn(C), rn(C), rn(N, C, H, W)
    r = rn(N, C, H, W) if residual else None
    # stochastic depth at p = 0.2: dropped images (0) and kept ones (1 / (1 - p))
    s = torch.tensor([0.0 if n % 3 == 1 else 1.25 for n in range(N)]) if drop else None
    return [y, gamma, beta, r], s, gout


def _formula(y, weight, bias, num_groups, relu, residual, drop_scale):
    out = F.group_norm(y, num_groups, weight, bias, 1e-5)
    if drop_scale is not None:
        out = drop_scale.view(-1, 1, 1, 1) * out
    if residual is not None:
        out = out + residual
    return torch.relu(out) if relu else out


def _five(fn, case, tensors, s, gout, device, dtype):
    """(out, dy, dgamma, dbeta[, dr]) of `fn` at the given inputs, as float64 CPU tensors."""
    G, relu = CASES[case][2], CASES[case][5]
    leaves = [None if t is None else t.to(device=device, dtype=dtype, copy=True) for t in tensors]
    for i in (0, 3):  # (the CPU compositions stay NCHW: torch's plain GroupNorm path is the yardstick)
        if leaves[i] is not None and device == "cuda":
            leaves[i] = leaves[i].contiguous(memory_format=torch.channels_last)
    leaves = [None if t is None else t.requires_grad_() for t in leaves]
    y, gamma, beta, r = leaves
    out = fn(y, gamma, beta, G, relu=relu, residual=r, drop_scale=None if s is None else s.to(device=device, dtype=dtype))
    out.backward(gout.to(device=device, dtype=dtype))
    return [t.detach().double().cpu().reshape(-1) for t in [out] + [l.grad for l in leaves if l is not None]]


@pytest.mark.parametrize("case", list(CASES))
def test_group_norm_act_matches_fp64(case):
    tensors, s, gout = _inputs(*CASES[case])
    formula = lambda y, w, b, G, **kw: _formula(y, w, b, G, kw["relu"], kw["residual"], kw["drop_scale"])
    ref = _five(formula, case, tensors, s, gout, "cpu", torch.float64)
    f32 = _five(formula, case, tensors, s, gout, "cpu", torch.float32)
    got = _five(_CF().group_norm_act, case, tensors, s, gout, "cuda", torch.float32)
    again = _five(_CF().group_norm_act, case, tensors, s, gout, "cuda", torch.float32)
    assert len(got) == len(ref) == (5 if CASES[case][6] else 4)
    bad = []
    for name, a, b, c, d in zip(NAMES, got, ref, f32, again):
        err, yard, scale = (a - b).abs().max().item(), (c - b).abs().max().item(), b.abs().max().item()
        print(f"gn {case} {name}: kernel err {err:.3e}  fp32 torch err {yard:.3e}  ratio {err / max(yard, 1e-300):.2f}")
        if not err <= 4.0 * yard + 1e-6 * scale:
            bad.append((name, err, yard))
        assert torch.equal(a, d), f"{name}: a second call differs bitwise"
    assert not bad, bad


@pytest.mark.parametrize("case", ["cg2_one_chunk", "g1_many_images_drop"])
def test_gn_publishes_act_max(case):
    L = _lib()
    orig = L.get_conv_gemm()
    L.set_conv_gemm("f16x2")
    try:
        (y, gamma, beta, r), s, _ = _inputs(*CASES[case])
        N, C, G = CASES[case][:3]
        cl = lambda t: t.cuda().contiguous(memory_format=torch.channels_last)
        out = _CF().group_norm_act(cl(y), gamma.cuda(), beta.cuda(), G, relu=True, residual=cl(r),
                                   drop_scale=None if s is None else s.cuda())
        slots, want = _CF()._get_amax(out), L.act_max(out)  # (the stand-alone pass, act_max_of)
        assert slots is not None
        # per image, then kActCopies copies per channel of which the consumers take the maximum (float bits)
        fold = lambda t: torch.cat([t[:N], t[N:N + L.act_max_copies() * C].view(-1, C).max(0).values])
        assert torch.equal(fold(slots), fold(want))
    finally:
        L.set_conv_gemm(orig)


def _step(ref, x, y, device, dtype):
    """(loss, parameter gradients) of one training step of a copy of `ref`, as float64 CPU values."""
    net = copy.deepcopy(ref).to(device=device, dtype=dtype)
    xin = x.to(device=device, dtype=dtype)
    if device == "cuda":
        xin = xin.contiguous(memory_format=torch.channels_last)
    loss = F.cross_entropy(net(xin), y.to(device))
    loss.backward()
    return loss.item(), [p.grad.double().cpu() for p in net.parameters()]


def _step_error(got, want):
    worst = abs(got[0] - want[0]) / abs(want[0])
    return max([worst] + [((g - g64).norm() / g64.norm()).item() for g, g64 in zip(got[1], want[1])])


@pytest.mark.parametrize("depth", ["18", "50"])
def test_resnet_gn_step_matches_reference(depth):
    """max(relative loss error, worst parameter gradient's |g - g64|_2 / |g64|_2) of the native step against the
    float64 reference path, held to 4 x the float32 CPU reference path's."""
    from cs744_distributed_data_parallel_amd.models import get_model

    torch.manual_seed(7)
    ref = get_model(f"resnet{depth}_gn", num_classes=10)
    x, y = torch.randn(2, 3, 64, 64), torch.tensor([3, 8])
    want = _step(ref, x, y, "cpu", torch.float64)
    yard = _step_error(_step(ref, x, y, "cpu", torch.float32), want)
    err = _step_error(_step(ref, x, y, "cuda", torch.float32), want)
    print(f"gn step: resnet{depth}_gn native {err:.3e}  fp32 cpu {yard:.3e}  ratio {err / yard:.2f}")
    assert err <= 4.0 * yard
