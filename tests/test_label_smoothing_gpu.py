"""Label smoothing and top-k accuracy on the fused cross-entropy kernels: every row layout of
xent_fwd / xent_bwd against torch in fp64, the rank rule of the top-k count, the one-launch
classifier backward with a smoothed gradient, and a captured VGG-11 step."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, C): the smallest shapes at which each code path of the kernels can go wrong
SHAPES = [
    (5, 10), (3, 64),                      # thread per row; its upper bound; B no multiple of the backward's 4 rows
    (1030, 10),                            # a thread's second row (r += 1024)
    (3, 65), (37, 1000), (70, 1024),       # four rows per wave: first width; partial group, lanes past C; rb += 64
    (3, 1025), (19, 2000),                 # row per wave; a wave's second row
]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _case(B, K):
    torch.manual_seed(5)
    logits = 3 * torch.randn(B, K, device="cuda")
    t = torch.randint(0, K, (B,), device="cuda")
    return logits, t


def _rank_hits(z, t, k):
    """The rank rule with torch ops on the host: rank = #{c : z_c > z_t, or z_c == z_t and c < t}."""
    z, t = z.cpu(), t.cpu()
    K = z.shape[1]
    tok = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1).unsqueeze(1)
    zt = z.gather(1, tc)
    rank = ((z > zt) | ((z == zt) & (torch.arange(K).unsqueeze(0) < tc))).sum(1)
    return int((tok & ~torch.isnan(zt.squeeze(1)) & (rank < k)).sum())


@pytest.mark.parametrize("eps", [0.1, 1.0])
@pytest.mark.parametrize("B,K", SHAPES)
def test_smoothed_cross_entropy_matches_fp64(B, K, eps):
    """loss = logsumexp(z) - (1 - eps) z_t - (eps / C) sum z, dlogits = (softmax - (1 - eps) onehot - eps / C) / B
    in all three row layouts, with the bounds of test_cross_entropy_and_accuracy."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    logits, t = _case(B, K)
    logits.requires_grad_()
    loss = CF.cross_entropy(logits, t, label_smoothing=eps)
    lr = logits.detach().double().cpu().requires_grad_()
    ref = F.cross_entropy(lr, t.cpu(), label_smoothing=eps)
    print(f"loss err {abs(loss.item() - ref.item()):.3e}")
    assert abs(loss.item() - ref.item()) < 1e-5
    loss.backward()
    ref.backward()
    print(f"grad err {rel_err(logits.grad, lr.grad):.3e}")
    assert rel_err(logits.grad, lr.grad) < 1e-5


@pytest.mark.parametrize("B,K", SHAPES)
def test_topk_count_follows_the_rank_rule(B, K):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    logits, t = _case(B, K)
    for k in (1, 2, 5, K):
        if k > K:
            continue
        assert int(CF.count_correct(logits, t, topk=k).item()) == _rank_hits(logits, t, k), k
    # quantised logits: many exact ties in every row
    q = logits.round()
    for k in (1, 2, 5):
        assert int(CF.count_correct(q, t, topk=k).item()) == _rank_hits(q, t, k), k


def test_topk_ties_go_to_the_lower_index():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    t = torch.tensor([0, 1, 4, 9], device="cuda")
    for K, tail in ((10, 0.0), (100, -1.0), (1100, -1.0)):  # the same ten tied classes in each row layout
        z = torch.full((4, K), tail, device="cuda")
        z[:, :10] = 0.0
        assert [int(CF.count_correct(z, t, topk=k).item()) for k in (1, 2, 5)] == [1, 2, 3], K


@pytest.mark.parametrize("K", [10, 100, 1100])
def test_bad_rows_are_not_counted_and_only_a_bad_target_poisons_the_loss(K):
    """A target of -1 and a NaN target logit: neither row is a top-k hit; the loss and the top-k count of
    one launch; NaN loss from the out-of-range row only."""
    import cs744_distributed_data_parallel_amd as cdp

    lib = cdp._native.lib()
    torch.manual_seed(2)
    z = torch.randn(6, K, device="cuda")
    t = torch.randint(0, K, (6,), device="cuda")
    t[4] = 3  # (the NaN row's target; not class 0, where the top-1 argmax scan starts)
    z[torch.arange(6, device="cuda"), t] = 50.0  # every row a top-1 hit ...
    bad_t = t.clone()
    bad_t[1] = -1  # ... but this one
    out = torch.zeros(1, dtype=torch.long, device="cuda")
    loss = lib.xent_fwd(z, bad_t, out, 0.1, 3)
    assert int(out.item()) == 5 and torch.isnan(loss).item()
    out.zero_()
    loss = lib.xent_fwd(z, t, out, 0.1, 3)
    ref = F.cross_entropy(z.double().cpu(), t.cpu(), label_smoothing=0.1)
    assert int(out.item()) == 6 and abs(loss.item() - ref.item()) < 1e-5
    # a NaN target logit: its row is not counted, for any k (k = K: every other row is)
    zn = z.clone()
    zn[4, t[4]] = float("nan")
    for k in (1, 3, K):
        out.zero_()
        lib.xent_fwd(zn, t, out, 0.0, k)
        assert int(out.item()) == 5, k
        out.zero_()
        lib.xent_fwd(zn, bad_t, out, 0.0, k)
        assert int(out.item()) == 4, k


def test_native_argument_checks():
    import cs744_distributed_data_parallel_amd as cdp

    lib = cdp._native.lib()
    z = torch.randn(4, 10, device="cuda")
    t = torch.randint(0, 10, (4,), device="cuda")
    g = torch.ones(1, device="cuda")
    for bad in (-0.1, 1.5):
        with pytest.raises(RuntimeError):
            lib.xent_fwd(z, t, None, bad, 1)
        with pytest.raises(RuntimeError):
            lib.xent_bwd(g, z, t, bad)
    with pytest.raises(RuntimeError):
        lib.xent_fwd(z, t, None, 0.0, 0)
    ref = F.cross_entropy(z.double().cpu(), t.cpu(), label_smoothing=0.1).item()
    assert abs(torch.ops.cdp.cross_entropy(z, t, 0.1).item() - ref) < 1e-5
    assert torch.equal(torch.ops.cdp.cross_entropy(z, t), lib.xent_fwd(z, t))


def test_zero_smoothing_and_top1_are_the_plain_kernels_bits():
    """label_smoothing=0.0 and topk=1 passed explicitly give the bits of a call without them."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    for B, K in ((37, 10), (37, 1000), (19, 2000)):
        logits, t = _case(B, K)
        a = logits.clone().requires_grad_()
        b = logits.clone().requires_grad_()
        la, lb = CF.cross_entropy(a, t), CF.cross_entropy(b, t, label_smoothing=0.0)
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
        assert torch.equal(CF.count_correct(logits, t), CF.count_correct(logits, t, topk=1))


# ------------------------------------------------------------------------------- fused classifier
@pytest.mark.parametrize("B,I,O", [(7, 512, 10), (32, 512, 10), (5, 24, 16)])
def test_fused_classifier_backward_with_smoothing_matches_fp64(B, I, O, monkeypatch):
    """CrossEntropyLoss(label_smoothing=0.1)(Linear(x)) backward as one launch: the smoothed dlogits and
    the dx, dW, db formed from it, with test_fused_classifier_backward_matches_fp64's tolerances
    ((5, 24, 16): the kernel's widest classifier, I no multiple of the 16-column tile)."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    eps = 0.1
    g = torch.Generator(device="cuda").manual_seed(B)
    x0 = torch.randn(B, I, device="cuda", generator=g)
    w0 = torch.randn(O, I, device="cuda", generator=g) * 0.05
    b0 = torch.randn(O, device="cuda", generator=g)
    t = torch.randint(0, O, (B,), device="cuda", generator=g)

    def run(fused):
        monkeypatch.setenv("CDP_FUSED_CLASSIFIER", "1" if fused else "0")
        x = x0.clone().requires_grad_()
        w = w0.clone().requires_grad_()
        b = b0.clone().requires_grad_()
        logits = CF.linear(x, w, b)
        logits.retain_grad()
        loss = CF.cross_entropy(logits, t, label_smoothing=eps)
        (loss * 0.5).backward()  # a non-unit incoming gradient
        torch.cuda.synchronize()
        return [logits.grad, x.grad, w.grad, b.grad]

    fz, un = run(True), run(False)
    xd = x0.double().requires_grad_()
    wd = w0.double().requires_grad_()
    bd = b0.double().requires_grad_()
    ld = F.linear(xd, wd, bd)
    ld.retain_grad()
    (F.cross_entropy(ld, t, label_smoothing=eps) * 0.5).backward()
    ref = [ld.grad, xd.grad, wd.grad, bd.grad]
    for name, a, u, r in zip(["dlogits", "dx", "dw", "db"], fz, un, ref):
        torch.testing.assert_close(a.double(), r, rtol=1e-5, atol=1e-7, msg=name)
        torch.testing.assert_close(a, u, rtol=1e-6, atol=1e-8, msg=name)
    # the smoothing reached the kernel: the unsmoothed gradient is another one
    plain = F.linear(x0.double(), w0.double(), b0.double()).requires_grad_()
    (F.cross_entropy(plain, t) * 0.5).backward()
    assert (fz[0].double() - plain.grad).abs().max().item() > 1e-4


def test_vgg11_smoothed_fused_classifier_takes_the_last_blocks_bn_reduction(monkeypatch):
    """VGG-11 at B = 32 with label_smoothing=0.1: the fused classifier backward still takes the last
    block's BN statistics hand-off, and every gradient matches the unfused path's (bounds of
    test_vgg11_fused_classifier_takes_the_last_blocks_bn_reduction)."""
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    B = 32
    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (B,), device="cuda", generator=g)
    crit = cdp.CrossEntropyLoss(label_smoothing=0.1)

    def grads(fused):
        monkeypatch.setenv("CDP_FUSED_CLASSIFIER", "1" if fused else "0")
        model.zero_grad(set_to_none=True)
        n0 = CF.LINK_HANDOFFS[0]
        crit(model(x), t).backward()
        torch.cuda.synchronize()
        return [p.grad.detach().clone() for p in model.parameters()], CF.LINK_HANDOFFS[0] - n0

    g_f, h_f = grads(True)
    g_u, h_u = grads(False)
    assert h_f == h_u + 1, (h_f, h_u)
    names = [n for n, _ in model.named_parameters()]
    for name, a, b in zip(names, g_f, g_u):
        if name.startswith("layers.") and name.endswith(".bias") and isinstance(
                model.layers[int(name.split(".")[1])], torch.nn.Conv2d):
            continue  # conv bias before training-mode BN: analytically zero, rounding noise
        err = ((a - b).norm() / b.norm().clamp_min(1e-30)).item()
        assert err < 1e-5, (name, err)


# ------------------------------------------------------------------------------- whole step
def test_captured_smoothed_step_replays_bitwise_like_eager():
    """A VGG-11 step with CrossEntropyLoss(label_smoothing=0.1), captured as test_graph_capture_training_step
    does, replays bitwise like a twin's eager steps (the comparison of
    test_replayed_step_matches_eager_with_other_work_between): eps is a host kernel argument, so the
    capture needs nothing new. The first loss differs from the eps = 0 loss on the same weights."""
    import cs744_distributed_data_parallel_amd as cdp

    crit = cdp.CrossEntropyLoss(label_smoothing=0.1)
    g = torch.Generator(device="cuda").manual_seed(1)
    xb = torch.randn(32, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    yb = torch.randint(0, 10, (32,), device="cuda", generator=g)

    def make():
        torch.manual_seed(0)
        m = cdp.VGG11().cuda()
        return m, cdp.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

    def body(m, o):
        o.zero_grad()
        loss = crit(m(xb), yb)
        loss.backward()
        o.step()
        return loss

    E, G, P = make(), make(), make()
    plain = cdp.CrossEntropyLoss()(P[0](xb), yb).item()  # a third twin: the same weights, eps = 0
    first = body(*E).item()
    body(*G)
    assert first != plain, (first, plain)
    for _ in range(2):
        body(*E); body(*G)
    body(*E)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body(*G)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        lo = body(*G)
    torch.cuda.synchronize()
    losses = []
    for i in range(5):
        le = body(*E).item()
        gr.replay()
        torch.cuda.synchronize()
        assert lo.item() == le, (i, lo.item(), le)
        for (n, a), b in zip(E[0].named_parameters(), G[0].parameters()):
            assert torch.equal(a, b), (i, n)
        losses.append(le)
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
