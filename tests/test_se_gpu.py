"""Squeeze-and-Excitation on the GPU (csrc/kernels/se.hip): `CF.se_scale_act` against the formula

    out = relu(s[n] * sigmoid(W2 relu(W1 mean_hw(u) + b1) + b2)[n, c] * u + r)

in float64 torch on the CPU, its published act maxima, and one training step of the SE-ResNets against their
float64 reference path.

Tolerances come from references, not from the kernels: an op tensor may miss fp64 by 4 x what the same
composition in float32 torch misses it by (the margin for a different summation order) plus 1e-6 of the tensor's
scale; an SE model may miss its fp64 step by 2 x what the plain ResNet of the same depth misses its own by."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAMES = ("out", "du", "dr", "dW1", "db1", "dW2", "db2")
# (N, C, Cr, H, W, drop)
CASES = {
    "one_chunk": (2, 64, 4, 7, 7, False),
    "odd_c_cr1": (3, 20, 1, 5, 5, False),  # C not a multiple of a wave's quads, Cr = 1, odd HW
    "ragged_chunks": (2, 8, 2, 33, 33, False),  # several chunks, the last one shorter
    "many_images_drop": (17, 32, 2, 3, 3, True),  # more images than the act-max LDS window of 16
    "widest_drop": (2, 2048, 128, 2, 2, True),
}


def _CF():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    return CF


def _lib():
    from cs744_distributed_data_parallel_amd import _native

    return _native.lib()


def _inputs(N, C, Cr, H, W, drop):
    """Seeded fp32 CPU inputs (u, r, w1, b1, w2, b2, s, upstream gradient); the weights at 1 / sqrt(fan_in) so the
    gate is not saturated, 4-D like the 1x1 convs' in the drop cases."""
    gen = torch.Generator().manual_seed(C + H)  # (seeds at which every case has hidden units that are alive)
    rn = lambda *s: torch.randn(*s, generator=gen)
    w1, w2 = rn(Cr, C) / C ** 0.5, rn(C, Cr) / Cr ** 0.5
    s = None
    if drop:  # stochastic depth at p = 0.2: dropped images (0) and kept ones (1 / (1 - p))
        s = torch.tensor([0.0 if n % 3 == 1 else 1.25 for n in range(N)])
        w1, w2 = w1.view(Cr, C, 1, 1), w2.view(C, Cr, 1, 1)
    return [rn(N, C, H, W), rn(N, C, H, W), w1, rn(Cr), w2, rn(C)], s, rn(N, C, H, W)


def _formula(u, r, w1, b1, w2, b2, drop_scale=None):
    C = u.shape[1]
    h = torch.relu(u.mean((2, 3)) @ w1.reshape(-1, C).t() + b1)
    y = torch.sigmoid(h @ w2.reshape(C, -1).t() + b2)[:, :, None, None] * u
    if drop_scale is not None:
        y = drop_scale.view(-1, 1, 1, 1) * y
    return torch.relu(y + r)


def _seven(fn, tensors, s, gout, device, dtype):
    """(out, du, dr, dW1, db1, dW2, db2) of `fn` at the given inputs, as float64 CPU tensors."""
    leaves = [t.to(device=device, dtype=dtype, copy=True) for t in tensors]
    for i in (0, 1):
        leaves[i] = leaves[i].contiguous(memory_format=torch.channels_last)
    leaves = [t.requires_grad_() for t in leaves]
    out = fn(*leaves, drop_scale=None if s is None else s.to(device=device, dtype=dtype))
    out.backward(gout.to(device=device, dtype=dtype))
    return [t.detach().double().cpu().reshape(-1) for t in [out] + [l.grad for l in leaves]]


@pytest.mark.parametrize("case", list(CASES))
def test_se_scale_act_matches_fp64(case):
    tensors, s, gout = _inputs(*CASES[case])
    ref = _seven(_formula, tensors, s, gout, "cpu", torch.float64)
    f32 = _seven(_formula, tensors, s, gout, "cpu", torch.float32)
    got = _seven(_CF().se_scale_act, tensors, s, gout, "cuda", torch.float32)
    again = _seven(_CF().se_scale_act, tensors, s, gout, "cuda", torch.float32)
    bad = []
    for name, a, b, c, d in zip(NAMES, got, ref, f32, again):
        err, yard, scale = (a - b).abs().max().item(), (c - b).abs().max().item(), b.abs().max().item()
        print(f"se {case} {name}: kernel err {err:.3e}  fp32 torch err {yard:.3e}  ratio {err / max(yard, 1e-300):.2f}")
        if not err <= 4.0 * yard + 1e-6 * scale:
            bad.append((name, err, yard))
        assert torch.equal(a, d), f"{name}: a second call differs bitwise"
    assert not bad, bad


@pytest.mark.parametrize("case", ["one_chunk", "many_images_drop"])
def test_se_publishes_act_max(case):
    L = _lib()
    orig = L.get_conv_gemm()
    L.set_conv_gemm("f16x2")
    try:
        tensors, s, _ = _inputs(*CASES[case])
        N, C = tensors[0].shape[:2]
        args = [t.cuda() for t in tensors]
        args[0], args[1] = (a.contiguous(memory_format=torch.channels_last) for a in args[:2])
        out = _CF().se_scale_act(*args, drop_scale=None if s is None else s.cuda())
        slots, want = _CF()._get_amax(out), L.act_max(out)  # (the stand-alone pass, act_max_of)
        assert slots is not None
        # per image, then kActCopies copies per channel of which the consumers take the maximum (float bits)
        fold = lambda t: torch.cat([t[:N], t[N:N + L.act_max_copies() * C].view(-1, C).max(0).values])
        assert torch.equal(fold(slots), fold(want))
    finally:
        L.set_conv_gemm(orig)


def _step_error(name):
    """max(relative loss error, worst parameter gradient's |g - g64|_2 / |g64|_2) of one training step of the
    model on the GPU against the same model and batch in float64 on the reference path."""
    from cs744_distributed_data_parallel_amd.models import get_model

    torch.manual_seed(7)
    ref = get_model(name, num_classes=10)
    net = copy.deepcopy(ref).cuda()
    ref = ref.double()
    x, y = torch.randn(2, 3, 64, 64), torch.tensor([3, 8])
    loss = F.cross_entropy(net(x.cuda().contiguous(memory_format=torch.channels_last)), y.cuda())
    loss.backward()
    loss64 = F.cross_entropy(ref(x.double()), y)
    loss64.backward()
    worst = abs(loss.item() - loss64.item()) / abs(loss64.item())
    for (n, p), q in zip(net.named_parameters(), ref.parameters()):
        g, g64 = p.grad.double().cpu(), q.grad
        worst = max(worst, ((g - g64).norm() / g64.norm()).item())
    return worst


@pytest.mark.parametrize("depth", ["18", "50"])
def test_seresnet_step_matches_reference(depth):
    yard, err = _step_error("resnet" + depth), _step_error("seresnet" + depth)
    print(f"se step: resnet{depth} {yard:.3e}  seresnet{depth} {err:.3e}  ratio {err / yard:.2f}")
    assert err <= 2.0 * yard
