"""Binary cross-entropy in the loss kernels: every row layout of bce_fwd / bce_bwd against a dense-target
F.binary_cross_entropy_with_logits in fp64, extreme logits, the bitwise identities of the mixed target, bad
targets, determinism, the BCE mode of the one-launch classifier backward, and a captured VGG-11 step whose lam
changes between replays."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (B, C): the smallest shapes at which each code path of the kernels can go wrong (test_label_smoothing_gpu.py)
SHAPES = [
    (5, 10), (3, 64),                      # thread per row; its upper bound; B no multiple of the backward's 4 rows
    (1030, 10),                            # a thread's second row (r += 1024)
    (3, 65), (37, 1000), (70, 1024),       # rows in registers: first width; partial group, lanes past C; next group
    (3, 1025), (19, 2000),                 # row per wave; a wave's second row
]
# (eps, threshold, lam; None: unmixed). No dense target value lies within 0.09 of the 0.2 threshold.
CONFIGS = [(0.0, None, None), (0.1, None, 0.3), (0.1, 0.2, 0.5), (0.1, 0.2, 0.9)]


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def close(loss, ref):
    return abs(loss - ref) <= 1e-5 * max(1.0, abs(ref))


def _case(B, K):
    torch.manual_seed(5)
    logits = 3 * torch.randn(B, K, device="cuda")
    t = torch.randint(0, K, (B,), device="cuda")
    return logits, t


def dense_target(t, C, eps=0.0, thr=None, tb=None, lam=None):
    """y = ((c == t_a ? wa : 0) + (c == t_b ? wb : 0)) + off in fp32 on the host, each step rounded on its own,
    then y > thr; an index out of [0, C) matches no class."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    lam = f(1.0) if lam is None else f(float(lam))
    on = f(1.0) - f(eps)
    off = f(eps) / C
    wa, wb = on * lam, on * (f(1.0) - lam)
    cls = torch.arange(C).unsqueeze(0)
    ya = torch.where(cls == t.cpu().unsqueeze(1), wa, f(0.0))
    yb = torch.where(cls == tb.cpu().unsqueeze(1), wb, f(0.0)) if tb is not None else torch.zeros_like(ya)
    y = (ya + yb) + off
    if thr is not None:
        y = (y > thr).float()
    return y


def ref_loss(z64, y, sum_classes):
    l = F.binary_cross_entropy_with_logits(z64, y.double(), reduction="none")
    return l.sum(1).mean() if sum_classes else l.mean()


def _lam(v):
    return torch.full((1,), v, device="cuda")


def _check_against_fp64(logits, t, eps, thr, lam, sum_classes, tag):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    tb = t.flip(0) if lam is not None else None
    a = logits.clone().requires_grad_()
    loss = CF.binary_cross_entropy(a, t, eps, thr, sum_classes, target_b=tb, lam=None if lam is None else _lam(lam))
    loss.backward()
    zr = logits.double().cpu().requires_grad_()
    ref = ref_loss(zr, dense_target(t, logits.shape[1], eps, thr, tb, lam), sum_classes)
    ref.backward()
    lerr = abs(loss.item() - ref.item()) / max(1.0, abs(ref.item()))
    gerr = rel_err(a.grad, zr.grad)
    print(f"{tag} eps {eps} thr {thr} lam {lam} sum_classes {sum_classes}: loss err {lerr:.3e} grad err {gerr:.3e}")
    assert torch.isfinite(a.grad).all() and torch.isfinite(loss)
    assert close(loss.item(), ref.item()), (tag, eps, thr, lam, sum_classes, loss.item(), ref.item())
    assert gerr < 1e-5, (tag, eps, thr, lam, sum_classes, gerr)
    return a.grad


@pytest.mark.parametrize("B,K", SHAPES)
def test_bce_matches_fp64_in_every_row_layout(B, K):
    """loss = sum(max(z, 0) - z y + log1p(exp(-|z|))) / (B C) or / B, dz = (sigmoid(z) - y) g / (B C) or / B, with
    the project's cross-entropy bounds (the loss bound relative: sum_classes losses reach about 2800)."""
    logits, t = _case(B, K)
    for eps, thr, lam in CONFIGS:
        for sum_classes in (False, True):
            _check_against_fp64(logits, t, eps, thr, lam, sum_classes, (B, K))


@pytest.mark.parametrize("K", [12, 100, 1100])
def test_extreme_logits_stay_finite(K):
    """+-100 and +-30 among ordinary logits, the targets on a -100 and on a +100 class: exp(-|z|) keeps the loss
    and the sigmoid finite; no inf or NaN anywhere in dlogits."""
    torch.manual_seed(3)
    z = 3 * torch.randn(6, K, device="cuda")
    z[:, 0], z[:, 1], z[:, 2], z[:, 3] = -100.0, 100.0, -30.0, 30.0
    z[1, 7], z[1, 8] = 100.0, -100.0
    t = torch.tensor([0, 1, 0, 1, 5, 2], device="cuda")  # rows 0, 2 on a -100 class, rows 1, 3 on a +100 class
    for eps, thr, lam in CONFIGS:
        for sum_classes in (False, True):
            g = _check_against_fp64(z, t, eps, thr, lam, sum_classes, ("extreme", K))
            assert g.abs().max().item() <= 1.0


@pytest.mark.parametrize("B,K", [(37, 10), (37, 1000), (19, 2000)])
def test_identities_are_bitwise(B, K):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    logits, t = _case(B, K)
    tb = t.flip(0)

    def run(*args, **kw):
        a = logits.clone().requires_grad_()
        loss = CF.binary_cross_entropy(a, t, *args, **kw)
        loss.backward()
        return loss.detach(), a.grad

    def same(p, q):
        return torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])

    for eps, thr, sc in ((0.0, None, False), (0.1, None, True), (0.1, 0.2, False)):
        assert same(run(eps, thr, sc, target_b=tb, lam=_lam(1.0)), run(eps, thr, sc)), (eps, thr, sc)
    assert same(run(target_b=t, lam=_lam(0.37)), run(0.0))
    assert same(run(0.1, target_threshold=None, sum_classes=False), run(0.1))
    thr = run(0.1, 0.2)
    assert same(run(0.1, 0.2, target_b=tb, lam=_lam(0.9)), thr)       # the partner's 0.09 + off is not above 0.2
    both = run(0.1, 0.2, target_b=tb, lam=_lam(0.5))                   # both classes are positives
    assert not torch.equal(both[0], thr[0]) and not torch.equal(both[1], thr[1])


@pytest.mark.parametrize("K", [10, 100, 1100])
def test_bad_targets_poison_the_loss_and_match_no_class(K):
    import cs744_distributed_data_parallel_amd as cdp

    lib = cdp._native.lib()
    torch.manual_seed(2)
    B, eps, lam = 6, 0.1, 0.3
    z = torch.randn(B, K, device="cuda")
    t = torch.randint(0, K, (B,), device="cuda")
    tb = t.flip(0).contiguous()
    g = torch.full((1,), 0.5, device="cuda")
    lam_t = _lam(lam)
    assert torch.isfinite(lib.bce_fwd(z, t, eps, None, False, tb, lam_t)).item()
    bad_a, bad_b = t.clone(), tb.clone()
    bad_a[1] = -1
    bad_b[4] = K
    sg = torch.sigmoid(z.double().cpu())
    for ta, tbb, row in ((bad_a, tb, 1), (t, bad_b, 4)):
        assert torch.isnan(lib.bce_fwd(z, ta, eps, None, False, tbb, lam_t)).item()
        assert torch.isnan(lib.bce_fwd(z, ta, eps, None, True, tbb, lam_t)).item()
        d = lib.bce_bwd(g, z, ta, eps, None, False, tbb, lam_t)
        assert torch.isfinite(d).all()
        # the bad row: sigmoid(z) * k minus the valid slot's weight only (the bad index matches no class)
        want = (sg - dense_target(ta, K, eps, None, tbb, lam).double()) * (0.5 / (B * K))
        assert rel_err(d, want) < 1e-5 and rel_err(d[row], want[row]) < 1e-5
    # the unmixed kernel
    assert torch.isnan(lib.bce_fwd(z, bad_a, eps)).item()
    d = lib.bce_bwd(g, z, bad_a, eps)
    want = (sg - dense_target(bad_a, K, eps).double()) * (0.5 / (B * K))
    assert torch.isfinite(d).all() and rel_err(d, want) < 1e-5 and rel_err(d[1], want[1]) < 1e-5


def test_native_argument_checks():
    import cs744_distributed_data_parallel_amd as cdp

    lib = cdp._native.lib()
    z = torch.randn(4, 10, device="cuda")
    t = torch.randint(0, 10, (4,), device="cuda")
    g = torch.ones(1, device="cuda")
    for bad in (-0.1, 1.5):
        with pytest.raises(RuntimeError):
            lib.bce_fwd(z, t, bad)
        with pytest.raises(RuntimeError):
            lib.bce_bwd(g, z, t, bad)
    for bad in (-0.1, 1.0):
        with pytest.raises(RuntimeError):
            lib.bce_fwd(z, t, 0.1, bad)
        with pytest.raises(RuntimeError):
            lib.bce_bwd(g, z, t, 0.1, bad)
    with pytest.raises(RuntimeError):
        lib.bce_fwd(z, t, 0.1, None, False, t)
    with pytest.raises(RuntimeError):
        lib.bce_bwd(g, z, t, 0.1, None, False, None, _lam(0.5))
    # the BCE knobs of the fused classifier backward belong to bce=True
    x = torch.randn(4, 24, device="cuda")
    w = torch.randn(10, 24, device="cuda")
    with pytest.raises(RuntimeError):
        lib.xent_linear_bwd(g, z, t, x, w, True, False, target_threshold=0.2)
    with pytest.raises(RuntimeError):
        lib.xent_linear_bwd(g, z, t, x, w, True, False, bce=True, target_threshold=1.0)


def test_forward_is_deterministic():
    import cs744_distributed_data_parallel_amd as cdp

    lib = cdp._native.lib()
    logits, t = _case(70, 1024)
    a = lib.bce_fwd(logits, t, 0.1, None, False, t.flip(0).contiguous(), _lam(0.3))
    b = lib.bce_fwd(logits, t, 0.1, None, False, t.flip(0).contiguous(), _lam(0.3))
    assert torch.equal(a, b) and torch.isfinite(a).item()


# ------------------------------------------------------------------------------- fused classifier
@pytest.mark.parametrize("eps,thr,lam", [(0.1, 0.2, None), (0.1, None, 0.3)])
@pytest.mark.parametrize("B,I,O", [(7, 512, 10), (32, 512, 10), (5, 24, 16)])
def test_fused_classifier_backward_in_bce_mode_matches_fp64(B, I, O, eps, thr, lam, monkeypatch):
    """BinaryCrossEntropy(Linear(x)) backward as one launch: dlogits bitwise bce_bwd's, and the dx, dW, db formed
    from it, with test_fused_classifier_backward_with_smoothing_matches_fp64's shapes and tolerances."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    g = torch.Generator(device="cuda").manual_seed(B)
    x0 = torch.randn(B, I, device="cuda", generator=g)
    w0 = torch.randn(O, I, device="cuda", generator=g) * 0.05
    b0 = torch.randn(O, device="cuda", generator=g)
    t = torch.randint(0, O, (B,), device="cuda", generator=g)
    tb = t.flip(0) if lam is not None else None
    lam_t = None if lam is None else _lam(lam)

    def run(fused):
        monkeypatch.setenv("CDP_FUSED_CLASSIFIER", "1" if fused else "0")
        x = x0.clone().requires_grad_()
        w = w0.clone().requires_grad_()
        b = b0.clone().requires_grad_()
        logits = CF.linear(x, w, b)
        logits.retain_grad()
        loss = CF.binary_cross_entropy(logits, t, eps, thr, target_b=tb, lam=lam_t)
        (loss * 0.5).backward()  # a non-unit incoming gradient
        torch.cuda.synchronize()
        return [logits.grad, x.grad, w.grad, b.grad]

    fz, un = run(True), run(False)
    xd = x0.double().cpu().requires_grad_()
    wd = w0.double().cpu().requires_grad_()
    bd = b0.double().cpu().requires_grad_()
    ld = F.linear(xd, wd, bd)
    ld.retain_grad()
    (ref_loss(ld, dense_target(t, O, eps, thr, tb, lam), False) * 0.5).backward()
    ref = [ld.grad, xd.grad, wd.grad, bd.grad]
    assert torch.equal(fz[0], un[0])
    for name, a, u, r in zip(["dlogits", "dx", "dw", "db"], fz, un, ref):
        torch.testing.assert_close(a.double().cpu(), r, rtol=1e-5, atol=1e-7, msg=name)
        torch.testing.assert_close(a, u, rtol=1e-6, atol=1e-8, msg=name)
    # the mode reached the kernel: the cross-entropy gradient on the same inputs is another one
    plain = F.linear(x0.double(), w0.double(), b0.double()).requires_grad_()
    ce = F.cross_entropy(plain, t, label_smoothing=eps)
    if lam is not None:
        ce = lam * ce + (1 - lam) * F.cross_entropy(plain, tb, label_smoothing=eps)
    (ce * 0.5).backward()
    assert (fz[0].double() - plain.grad).abs().max().item() > 1e-4


def test_vgg11_bce_fused_classifier_takes_the_last_blocks_bn_reduction(monkeypatch):
    """VGG-11 at B = 32 with BinaryCrossEntropy(0.1, target_threshold=0.2): the fused classifier backward takes
    the last block's BN statistics hand-off, and every gradient matches the unfused path's."""
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    B = 32
    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    g = torch.Generator(device="cuda").manual_seed(B)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    t = torch.randint(0, 10, (B,), device="cuda", generator=g)
    crit = cdp.BinaryCrossEntropy(0.1, target_threshold=0.2)

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
def test_captured_bce_step_replays_bitwise_like_eager_and_reads_lam():
    """A VGG-11 step with BinaryCrossEntropy(label_smoothing=0.1) on a MixTarget whose lam tensor the test owns,
    captured as test_captured_smoothed_step_replays_bitwise_like_eager does: every replay, after lam was filled
    with a new value, gives the loss and the parameters of a twin's eager step with that lam."""
    import cs744_distributed_data_parallel_amd as cdp

    crit = cdp.BinaryCrossEntropy(label_smoothing=0.1)
    g = torch.Generator(device="cuda").manual_seed(1)
    xb = torch.randn(32, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    yb = torch.randint(0, 10, (32,), device="cuda", generator=g)
    yb_b = yb.flip(0).contiguous()

    def make():
        torch.manual_seed(0)
        m = cdp.VGG11().cuda()
        lam = torch.ones(1, device="cuda")
        info = torch.zeros(2, device="cuda")
        return m, cdp.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4), cdp.MixTarget(yb, yb_b, lam, info)

    def body(m, o, tgt):
        o.zero_grad()
        loss = crit(m(xb), tgt)
        loss.backward()
        o.step()
        return loss

    def step(side, lam):
        side[2].lam.fill_(lam)
        return body(*side)

    E, G, P = make(), make(), make()
    P[2].lam.fill_(0.6)
    plain = cdp.CrossEntropyLoss(label_smoothing=0.1)(P[0](xb), P[2]).item()  # a third twin: the same weights
    first = step(E, 0.6).item()
    step(G, 0.6)
    assert first != plain, (first, plain)
    for lam in (0.2, 0.8):
        step(E, lam); step(G, lam)
    step(E, 0.4)
    G[2].lam.fill_(0.4)
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
    for i, lam in enumerate((0.1, 0.9, 0.3, 0.7, 0.5)):
        le = step(E, lam).item()
        G[2].lam.fill_(lam)
        gr.replay()
        torch.cuda.synchronize()
        assert lo.item() == le, (i, lo.item(), le)
        for (n, a), b in zip(E[0].named_parameters(), G[0].parameters()):
            assert torch.equal(a, b), (i, n)
        losses.append(le)
    assert all(torch.isfinite(torch.tensor(losses)))
    assert all(a != b for a, b in zip(losses, losses[1:])), losses
