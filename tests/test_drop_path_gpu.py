"""Stochastic depth on the GPU: the per-image scale inside the fused residual apply kernels (forward,
statistics reduction, backward apply) against an fp64 composition of

    out[b] = relu(s[b] * bn(conv(x))[b] + shortcut[b]),

the exact properties of dropped images, the device draw against its Python twin, and the model with
`drop_path_rate` / `zero_init_residual` against its fp64 reference path, captured in a hipGraph included.

Tolerances are those of tests/test_kernels_gpu.py::test_residual_block_no_pool and its neighbours
(`rel_err`: max |a - b| / max |b|): out 5e-5, dres 1e-5, dx / dW / dgamma / dbeta 5e-4."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _cdp():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp


def _CF():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    return CF


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _pair(ci, co, k):
    """A conv / BatchNorm pair on the GPU (non-trivial affine) and its fp64 twin on the CPU."""
    conv = torch.nn.Conv2d(ci, co, k, 1, k // 2, bias=False).cuda()
    bn = torch.nn.BatchNorm2d(co).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    conv_r = torch.nn.Conv2d(ci, co, k, 1, k // 2, bias=False).double()
    bn_r = torch.nn.BatchNorm2d(co).double()
    conv_r.load_state_dict(conv.state_dict())
    bn_r.load_state_dict(bn.state_dict())
    conv.weight.data = cl(conv.weight.data)
    return conv, bn, conv_r, bn_r


BLOCK_CASES = {
    # name: (k, Cin, Cout, x shape, scales, relu, downsample shortcut)
    "a_drop_1x1": (1, 64, 64, (4, 64, 8, 8), [0.0, 1.25, 0.0, 1.25], True, False),
    "b_arbitrary_scales": (1, 64, 64, (4, 64, 8, 8), [0.5, 2.0, 0.0, 1.0], True, False),
    "c_3x3_odd_batch": (3, 128, 128, (5, 128, 6, 6), [1.25, 0.0, 1.25, 1.25, 0.0], True, False),
    "d_two_quads_per_thread": (1, 512, 2048, (4, 512, 2, 2), [2.0, 2.0, 0.0, 2.0], True, False),
    "e_no_relu_zout": (1, 64, 64, (4, 64, 8, 8), [0.0, 1.25, 0.0, 1.25], False, False),
    "f_downsample_shortcut": (1, 64, 64, (4, 64, 8, 8), [0.0, 1.25, 0.0, 1.25], True, True),
}


@pytest.mark.parametrize("case", list(BLOCK_CASES))
def test_block_matches_fp64(case):
    CF = _CF()
    k, ci, co, shape, scales, relu, down = BLOCK_CASES[case]
    torch.manual_seed(3)
    conv, bn, conv_r, bn_r = _pair(ci, co, k)
    s = torch.tensor(scales, device="cuda")
    x = torch.randn(*shape, device="cuda")
    xn = cl(x).requires_grad_()
    xr = x.double().cpu().requires_grad_()
    sr = s.double().cpu().view(-1, 1, 1, 1)
    if down:  # the shortcut is a deferred 1x1 downsample conv + BatchNorm of the same input
        dconv, dbn, dconv_r, dbn_r = _pair(ci, co, 1)
        idt = CF.conv_bn_act(xn, dconv, dbn, relu=False, defer_apply=True)
        out = CF.conv_bn_act(xn, conv, bn, relu=relu, residual=idt, drop_scale=s)
        ref = sr * bn_r(conv_r(xr)) + dbn_r(dconv_r(xr))
    else:
        r = torch.randn(shape[0], co, shape[2], shape[3], device="cuda")
        rn = cl(r).requires_grad_()
        rr = r.double().cpu().requires_grad_()
        out = CF.conv_bn_act(xn, conv, bn, relu=relu, residual=rn, drop_scale=s)
        ref = sr * bn_r(conv_r(xr)) + rr
    if relu:
        ref = F.relu(ref)
    errs = {"out": rel_err(out, ref)}
    g = torch.randn_like(out)
    out.backward(g)
    ref.backward(g.double().cpu())
    if not down:
        errs["dres"] = rel_err(rn.grad, rr.grad)
    errs["dx"] = rel_err(xn.grad, xr.grad)
    errs["dW"] = rel_err(conv.weight.grad, conv_r.weight.grad)
    errs["dgamma"] = rel_err(bn.weight.grad, bn_r.weight.grad)
    errs["dbeta"] = rel_err(bn.bias.grad, bn_r.bias.grad)
    if down:
        errs["ds_dW"] = rel_err(dconv.weight.grad, dconv_r.weight.grad)
        errs["ds_dgamma"] = rel_err(dbn.weight.grad, dbn_r.weight.grad)
        errs["ds_dbeta"] = rel_err(dbn.bias.grad, dbn_r.bias.grad)
    print(case, errs)
    assert errs.pop("out") < 5e-5
    assert errs.pop("dres", 0.0) < 1e-5
    for name, e in errs.items():
        assert e < 5e-4, (name, e)
    # the statistics are those of the unscaled BatchNorm
    assert rel_err(bn.running_mean, bn_r.running_mean) < 1e-5
    assert rel_err(bn.running_var, bn_r.running_var) < 1e-5
    assert int(bn.num_batches_tracked) == 1


def _plain_block(s, seed=4, drop=True, relu=True):
    CF = _CF()
    torch.manual_seed(seed)
    conv, bn, _, _ = _pair(64, 64, 1)
    x = torch.randn(4, 64, 8, 8, device="cuda")
    r = torch.randn(4, 64, 8, 8, device="cuda")
    xn, rn = cl(x).requires_grad_(), cl(r).requires_grad_()
    kw = {"drop_scale": s} if drop else {}
    out = CF.conv_bn_act(xn, conv, bn, relu=relu, residual=rn, **kw)
    g = torch.randn_like(out)
    out.backward(g)
    return out.detach(), g, xn, rn, conv, bn


def test_dropped_images_are_the_shortcut_bitwise():
    s = torch.tensor([0.0, 1.25, 0.0, 1.25], device="cuda")
    out, g, xn, rn, conv, bn = _plain_block(s)
    for b in (0, 2):
        assert torch.equal(out[b], F.relu(rn.detach()[b]))
    # the shortcut's gradient is dz itself, for every image, dropped or kept
    assert torch.equal(rn.grad, g * (out > 0))
    assert not torch.equal(out[1], F.relu(rn.detach()[1]))


def test_all_dropped_block_has_zero_branch_gradients():
    s = torch.zeros(4, device="cuda")
    out, g, xn, rn, conv, bn = _plain_block(s)
    assert torch.equal(out, F.relu(rn.detach()))
    zero = lambda t: torch.equal(t, torch.zeros_like(t))  # noqa: E731
    assert zero(conv.weight.grad) and zero(bn.weight.grad) and zero(bn.bias.grad)
    for t in (out, xn.grad, rn.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad, bn.running_mean,
              bn.running_var):
        assert torch.isfinite(t).all()


def test_no_scale_is_the_call_without_the_argument_and_a_scale_needs_a_residual():
    CF = _CF()
    a = _plain_block(None)
    b = _plain_block(None, drop=False)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[2].grad, b[2].grad) and torch.equal(a[3].grad, b[3].grad)
    assert torch.equal(a[4].weight.grad, b[4].weight.grad)
    assert torch.equal(a[5].weight.grad, b[5].weight.grad) and torch.equal(a[5].bias.grad, b[5].bias.grad)
    conv, bn, _, _ = _pair(64, 64, 1)
    x = cl(torch.randn(4, 64, 8, 8, device="cuda"))
    s = torch.ones(4, device="cuda")
    with pytest.raises((ValueError, RuntimeError)):
        CF.conv_bn_act(x, conv, bn, relu=True, drop_scale=s)
    lib = _cdp()._native.lib()
    args = (x, conv.weight, None, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
            0.1, 1e-5, True, 1, 0)
    with pytest.raises(RuntimeError):  # the op itself: no residual
        lib.conv_bn_act_fwd(*args, False, True, None, drop_scale=s)
    with pytest.raises(RuntimeError):  # a residual, but pooled
        lib.conv_bn_act_fwd(*args, True, True, x, drop_scale=s)
    with pytest.raises(RuntimeError):  # defer_apply
        lib.conv_bn_act_fwd(*args, False, False, None, defer_apply=True, drop_scale=s)


@pytest.mark.parametrize("B", [1, 5, 64])
def test_draw_kernel_is_the_python_twin(B):
    from cs744_distributed_data_parallel_amd.ops.functional import drop_path_scales

    lib = _cdp()._native.lib()
    rates = [0.1, 0.25, 0.5]
    rd = torch.tensor(rates, device="cuda")
    seed, c0 = 1234567, 41
    counter = torch.tensor([c0], dtype=torch.int64, device="cuda")
    table = lib.drop_path_table(seed, c0, 8, rd, B)
    assert table.shape == (8, 3, B) and table.dtype == torch.float32
    assert int(counter) == c0  # the schedule moves no counter
    for t in range(8):
        want = drop_path_scales(seed, c0 + t, rates, B)
        got = lib.drop_path_draw(counter, seed, rd, B)
        assert int(counter) == c0 + t + 1
        assert torch.equal(got.cpu(), want), t
        assert torch.equal(table[t].cpu(), want), t
    assert int(counter) == c0 + 8


def _load(model, ref):
    model.load_state_dict({k: v.float().cuda() for k, v in ref.state_dict().items()})


def _mixed(table):
    """at least one dropped and one kept branch"""
    return bool((table == 0).any()) and bool((table != 0).any())


def test_resnet18_drop_path_gradients_match_fp64():
    cdp = _cdp()
    torch.manual_seed(1)
    kw = dict(num_classes=10, drop_path_rate=0.5, drop_path_seed=3)
    ref = cdp.resnet18(channels_last=False, **kw).double()
    model = cdp.resnet18(**kw).cuda()
    _load(model, ref)
    x = torch.randn(2, 3, 64, 64)
    y = torch.randint(0, 10, (2,))
    cdp.CrossEntropyLoss()(model(x.cuda()), y.cuda()).backward()
    F.cross_entropy(ref(x.double()), y).backward()
    assert model.last_drop_scales.is_cuda and torch.equal(model.last_drop_scales.cpu(), ref.last_drop_scales)
    assert _mixed(ref.last_drop_scales), ref.last_drop_scales
    assert int(model.drop_path_step) == int(ref.drop_path_step) == 1
    for (n, p), pr in zip(model.named_parameters(), ref.parameters()):
        err = ((p.grad.double().cpu() - pr.grad).norm() / pr.grad.norm().clamp_min(1e-30)).item()
        assert err < 1e-4, (n, err)


def test_resnet50_drop_path_forward_backward_small(monkeypatch):
    cdp = _cdp()
    torch.manual_seed(0)
    kw = dict(num_classes=100, drop_path_rate=0.5, drop_path_seed=7)
    ref = cdp.resnet50(channels_last=False, **kw).double()
    model = cdp.resnet50(**kw).cuda()
    _load(model, ref)
    x = torch.randn(4, 3, 64, 64)
    y = torch.randint(0, 100, (4,))
    loss = cdp.CrossEntropyLoss()(model(x.cuda()), y.cuda())
    loss.backward()
    loss_r = F.cross_entropy(ref(x.double()), y)
    loss_r.backward()
    assert torch.equal(model.last_drop_scales.cpu(), ref.last_drop_scales) and _mixed(ref.last_drop_scales)
    assert abs(loss.item() - loss_r.item()) < 1e-3 * max(1.0, abs(loss_r.item()))
    g = torch.cat([p.grad.double().cpu().reshape(-1) for p in model.parameters()])
    gr = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
    monkeypatch.setenv("CDP_FORCE_REFERENCE", "1")
    t32 = cdp.resnet50(channels_last=False, **kw).cuda()
    _load(t32, ref)
    F.cross_entropy(t32(x.cuda()), y.cuda()).backward()
    assert torch.equal(t32.last_drop_scales.cpu(), ref.last_drop_scales)  # the same scales
    gt = torch.cat([p.grad.double().cpu().reshape(-1) for p in t32.parameters()])
    e_nat = ((g - gr).norm() / gr.norm()).item()
    e_t32 = ((gt - gr).norm() / gr.norm()).item()
    print("e_nat", e_nat, "e_t32", e_t32)
    assert e_nat < max(3 * e_t32, 1e-4), (e_nat, e_t32)


def test_resnet18_zero_init_residual_matches_fp64():
    cdp = _cdp()
    torch.manual_seed(1)
    kw = dict(num_classes=10, drop_path_rate=0.5, drop_path_seed=3, zero_init_residual=True)
    ref = cdp.resnet18(channels_last=False, **kw).double()
    model = cdp.resnet18(**kw).cuda()
    _load(model, ref)
    x = torch.randn(2, 3, 64, 64)
    y = torch.randint(0, 10, (2,))
    loss = cdp.CrossEntropyLoss()(model(x.cuda()), y.cuda())
    loss.backward()
    loss_r = F.cross_entropy(ref(x.double()), y)
    loss_r.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-3 * abs(loss_r.item())
    nzero = 0
    for (n, p), pr in zip(model.named_parameters(), ref.parameters()):
        if not pr.grad.any():  # nothing reaches the convolutions behind a zero BatchNorm weight
            nzero += 1
            assert not p.grad.any(), n
            continue
        err = ((p.grad.double().cpu() - pr.grad).norm() / pr.grad.norm()).item()
        assert err < 1e-4, (n, err)
    assert nzero >= 8  # at least every block's first conv


def test_captured_step_drops_different_images_at_every_replay():
    cdp = _cdp()
    torch.manual_seed(0)
    model = cdp.resnet18(num_classes=10, drop_path_rate=0.5, drop_path_seed=11).cuda()
    opt = cdp.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    crit = cdp.CrossEntropyLoss()
    x = cl(torch.randn(8, 3, 64, 64, device="cuda"))
    y = torch.randint(0, 10, (8,), device="cuda")

    def body():
        opt.zero_grad()
        loss = crit(model(x), y)
        loss.backward()
        opt.step()
        return loss

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
        with pytest.raises(RuntimeError):
            model.set_drop_path_step(0)  # not while capturing
    c0 = int(model.drop_path_step)
    assert c0 == 3  # the capture itself ran nothing
    tables = []
    for i in range(4):
        g.replay()
        want = model.drop_path_schedule(c0 + i, 1, 8)[0]
        assert torch.equal(model.last_drop_scales, want), i
        tables.append(model.last_drop_scales.clone())
    assert any(not torch.equal(tables[0], t) for t in tables[1:])
    assert int(model.drop_path_step) == c0 + 4
    assert all(torch.isfinite(p).all() for p in model.parameters())


def test_rate_zero_and_eval_are_the_plain_model():
    cdp = _cdp()
    torch.manual_seed(2)
    plain = cdp.resnet18(num_classes=10).cuda()
    zero = cdp.resnet18(num_classes=10, drop_path_rate=0.0).cuda()
    zero.load_state_dict(plain.state_dict())
    assert zero.drop_path_step is None and zero.last_drop_scales is None
    x = cl(torch.randn(2, 3, 64, 64, device="cuda"))
    y = torch.randint(0, 10, (2,), device="cuda")
    crit = cdp.CrossEntropyLoss()
    crit(plain(x), y).backward()
    crit(zero(x), y).backward()
    for (n, p), q in zip(plain.named_parameters(), zero.parameters()):
        assert torch.equal(p.grad, q.grad), n
    half = cdp.resnet18(num_classes=10, drop_path_rate=0.5).cuda()
    half.load_state_dict(plain.state_dict())
    plain.eval()
    half.eval()
    with torch.no_grad():
        assert torch.equal(half(x), plain(x))
    assert int(half.drop_path_step) == 0 and half.last_drop_scales is None
