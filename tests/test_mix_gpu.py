"""Fused mixup / CutMix: the augment kernel's MIX instantiation against the unmixed batch, the
device-side parameter stream (mix_draw / mix_params), the two-target cross-entropy kernels in every
row layout against fp64 torch, the one-launch classifier backward with a target pair, and a captured
VGG-11 step whose mix changes at every replay."""
import math
import re

import pytest
import torch
import torch.nn.functional as F

from _mix_util import CASES, MIX, check_default_arguments_change_nothing, check_mixed_batches, dataset
from test_label_smoothing_gpu import SHAPES, _case, rel_err

pytestmark = pytest.mark.gpu

N_DRAWS = 4096
KS_BOUND = 1.95 * math.sqrt(2.0 / N_DRAWS)  # 0.0431: the two-sample 0.1 % critical value


def _lib():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


# ------------------------------------------------------------------------------- mixed images
@pytest.mark.parametrize("B,H,W", CASES)
def test_mixed_batches_follow_the_unmixed_batch(B, H, W):
    check_mixed_batches(B, H, W, "cuda")


def test_default_mix_arguments_change_nothing():
    check_default_arguments_change_nothing("cuda")


# ------------------------------------------------------------------------------- parameter stream
def test_published_row_is_mix_params_eagerly_and_in_replays():
    """The row a batch publishes is mix_params(seed, counter, 1, ...) bitwise: eagerly, and in replays of
    a captured batch whose counter the graph advances itself (nbatches > 0)."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 4, 8, 8
    ds = dataset(B, H, W, "cuda")
    ld = DeviceLoader(ds, B, seed=21, **MIX)
    idx = torch.arange(len(ds), device="cuda")
    lib = _lib()

    def want(ctr):
        return lib.mix_params(21, ctr, 1, MIX["mixup_alpha"], MIX["cutmix_alpha"], MIX["mix_prob"],
                              MIX["mix_switch_prob"], H, W)[0]

    for ctr in range(4):
        assert int(ld._counter.item()) == ctr
        _, tgt = ld.batch(idx, 0, B)
        assert torch.equal(tgt.info, want(ctr)), ctr
    assert torch.equal(ld.mix_schedule(0, 4), torch.stack([want(c) for c in range(4)]))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ld.batch(idx, 0, B, nbatches=3)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        data, tgt = ld.batch(idx, 0, B, nbatches=3)
    torch.cuda.synchronize()
    rows = []
    for _ in range(6):
        ctr = int(ld._counter.item())
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(tgt.info, want(ctr)), ctr
        assert tgt.lam.item() == tgt.info[1].item()
        rows.append(tuple(tgt.info.tolist()))
        assert int(ld._counter.item()) == ctr + 1
    assert len(set(rows)) > 1


def _ks(a, b):
    """Two-sample Kolmogorov-Smirnov statistic."""
    a, b = a.double().sort().values, b.double().sort().values
    allv = torch.cat([a, b])
    ca = torch.searchsorted(a, allv, right=True).double() / a.numel()
    cb = torch.searchsorted(b, allv, right=True).double() / b.numel()
    return (ca - cb).abs().max().item()


@pytest.mark.parametrize("cut", [False, True])
@pytest.mark.parametrize("alpha", [0.2, 1.0, 4.0])
def test_lam_raw_is_beta_distributed(alpha, cut):
    """4096 consecutive counters against 4096 torch Beta(alpha, alpha) samples (fixed seed; two torch samples
    with different seeds give 0.014 .. 0.021 at these alphas, inside the same bound)."""
    rows = _lib().mix_params(7, 100, N_DRAWS, 0.0 if cut else alpha, alpha if cut else 0.0, 1.0, 0.5, 32, 32).cpu()
    assert (rows[:, 0] == (2 if cut else 1)).all()
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        ref = torch.distributions.Beta(torch.tensor(alpha), torch.tensor(alpha)).sample((N_DRAWS,))
    d = _ks(rows[:, 2], ref)
    print(f"alpha {alpha} cut {cut}: KS {d:.4f} bound {KS_BOUND:.4f}")
    assert d <= KS_BOUND
    assert ((rows[:, 2] >= 0) & (rows[:, 2] <= 1)).all()
    if not cut:
        assert torch.equal(rows[:, 1], rows[:, 2])


def test_mode_frequencies_and_box_rule():
    n, H, W = N_DRAWS, 224, 160
    rows = _lib().mix_params(3, 5000, n, 0.2, 1.0, 0.7, 0.25, H, W).cpu().double()
    mode = rows[:, 0]
    for m, p in ((0, 0.3), (2, 0.7 * 0.25)):
        cnt, sd = int((mode == m).sum()), math.sqrt(n * p * (1 - p))
        print(f"mode {m}: {cnt} of {n}, expected {p * n:.1f} +- {5 * sd:.1f}")
        assert abs(cnt - p * n) <= 5 * sd, (m, cnt)
    none = rows[mode == 0]
    assert (none[:, 1] == 1).all() and (none[:, 3:] == 0).all()
    c = rows[mode == 2]
    lam_raw, y0, y1, x0, x1 = c[:, 2], c[:, 3], c[:, 4], c[:, 5], c[:, 6]
    assert ((0 <= y0) & (y0 <= y1) & (y1 <= H) & (0 <= x0) & (x0 <= x1) & (x1 <= W)).all()
    for lo, hi, S in ((y0, y1, H), (x0, x1, W)):
        exact = S * torch.sqrt(1 - lam_raw)
        cut = exact.floor()
        near = (exact - exact.round()).abs() < 1e-4  # int() of a product that close to an integer may go either way
        assert ((hi - lo) <= cut + near.double()).all()
        assert int(((hi - lo) == 2 * (cut // 2)).sum()) > 0  # boxes the image did not clip
        mid = (lo + hi) / 2
        assert int((mid < S / 2).sum()) > 0 and int((mid >= S / 2).sum()) > 0
    want = (1.0 - (y1 - y0) * (x1 - x0) / (H * W)).float()
    assert torch.equal(c[:, 1].float(), want)


def test_mix_params_argument_checks():
    lib = _lib()
    for bad in (dict(mixup_alpha=-1.0), dict(cutmix_alpha=-0.5), dict(mix_prob=1.5), dict(mix_switch_prob=-0.1)):
        with pytest.raises(RuntimeError):
            lib.mix_params(0, 0, 4, **bad)
    assert lib.mix_params(0, 0, 0, mixup_alpha=1.0).shape == (0, 8)
    off = lib.mix_params(0, 0, 3).cpu()  # both alphas 0: nothing is mixed
    assert (off[:, 0] == 0).all() and (off[:, 1] == 1).all()


# ------------------------------------------------------------------------------- two-target loss
def _pair(B, K):
    logits, t = _case(B, K)
    tb = torch.randint(0, K, (B,), device="cuda", generator=torch.Generator(device="cuda").manual_seed(B + K))
    return logits, t, tb


def _ref(logits, t, tb, lam, eps):
    lr = logits.detach().double().cpu().requires_grad_()
    ref = lam * F.cross_entropy(lr, t.cpu(), label_smoothing=eps) + (1 - lam) * F.cross_entropy(
        lr, tb.cpu(), label_smoothing=eps)
    ref.backward()
    return ref.item(), lr.grad


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("B,K", SHAPES)
def test_two_target_cross_entropy_matches_fp64(B, K, eps):
    """lam CE(z, a) + (1 - lam) CE(z, b) and its gradient in all three row layouts, with the bounds of
    test_smoothed_cross_entropy_matches_fp64; also with every row's two targets equal."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    logits, t, tb = _pair(B, K)
    for lam in (0.3, 1.0, 0.0):
        lam_t = torch.tensor([lam], device="cuda")
        for second in (tb, t.clone()):
            z = logits.clone().requires_grad_()
            loss = CF.cross_entropy(z, t, label_smoothing=eps, target_b=second, lam=lam_t)
            loss.backward()
            ref, gref = _ref(logits, t, second, lam_t.item(), eps)
            print(f"lam {lam} same {second is not tb}: loss err {abs(loss.item() - ref):.3e} "
                  f"grad err {rel_err(z.grad, gref):.3e}")
            assert abs(loss.item() - ref) < 1e-5
            assert rel_err(z.grad, gref) < 1e-5


@pytest.mark.parametrize("B,K", [(5, 10), (37, 1000), (19, 2000)])
def test_two_target_edge_cases(B, K):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    logits, t, tb = _pair(B, K)
    lam = torch.tensor([0.3], device="cuda")
    for eps in (0.0, 0.1):
        # the same target twice is the single-target loss
        one = CF.cross_entropy(logits, t, label_smoothing=eps).item()
        two = CF.cross_entropy(logits, t, label_smoothing=eps, target_b=t.clone(), lam=lam).item()
        assert abs(one - two) < 1e-6, (eps, one, two)
        # an out-of-range second (or first) target poisons the loss and reads nothing out of bounds
        for bad_v in (K, -1, 2 ** 40):
            bad = tb.clone()
            bad[B // 2] = bad_v
            z = logits.clone().requires_grad_()
            loss = CF.cross_entropy(z, t, label_smoothing=eps, target_b=bad, lam=lam)
            loss.backward()
            torch.cuda.synchronize()
            assert torch.isnan(loss).item() and torch.isfinite(z.grad).all().item()
            assert torch.isnan(CF.cross_entropy(logits, bad, label_smoothing=eps, target_b=tb, lam=lam)).item()
    # lam is read from the device at every call, not baked in
    lam = torch.tensor([0.3], device="cuda")
    a = CF.cross_entropy(logits, t, target_b=tb, lam=lam).item()
    lam.fill_(0.9)
    b = CF.cross_entropy(logits, t, target_b=tb, lam=lam).item()
    ref, _ = _ref(logits, t, tb, lam.item(), 0.0)
    assert a != b and abs(b - ref) < 1e-5


def test_native_two_target_argument_checks():
    lib = _lib()
    z = torch.randn(4, 10, device="cuda")
    t = torch.randint(0, 10, (4,), device="cuda")
    lam = torch.tensor([0.5], device="cuda")
    g = torch.ones(1, device="cuda")
    out = torch.zeros(1, dtype=torch.long, device="cuda")
    with pytest.raises(RuntimeError):  # the correct counter is not offered together with target_b
        lib.xent_fwd(z, t, out, 0.0, 1, target_b=t, lam=lam)
    with pytest.raises(RuntimeError):
        lib.xent_fwd(z, t, None, 0.0, 3, target_b=t, lam=lam)
    with pytest.raises(RuntimeError):
        lib.xent_fwd(z, t, None, 0.0, 1, target_b=t)
    with pytest.raises(RuntimeError):
        lib.xent_bwd(g, z, t, 0.0, None, lam)
    with pytest.raises(RuntimeError):
        lib.xent_fwd(z, t, None, 0.0, 1, target_b=t[:3], lam=lam)
    with pytest.raises(RuntimeError):
        lib.xent_fwd(z, t, None, 0.0, 1, target_b=t, lam=lam.cpu())
    # without a second target the calls are what they were
    assert torch.equal(lib.xent_fwd(z, t), lib.xent_fwd(z, t, None, 0.0, 1, None, None))
    assert int(out.item()) == 0


# ------------------------------------------------------------------------------- fused classifier
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("link", [False, True])
@pytest.mark.parametrize("B", [5, 64])
def test_fused_classifier_backward_with_a_target_pair(B, link, eps, monkeypatch):
    """[B, 512] -> 10 with lam = 0.3: the one-launch classifier backward (default) against
    CDP_FUSED_CLASSIFIER=0 -- dlogits, dX, dW, db bitwise equal -- and both within 1e-5 relative of fp64.
    link: the Linear's input is the pooled 1x1 output of a conv + BatchNorm + ReLU + MaxPool block, whose
    BN statistics reduction the fused launch takes over (one hand-off more)."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    g = torch.Generator(device="cuda").manual_seed(B)
    w0 = torch.randn(10, 512, device="cuda", generator=g) * 0.05
    b0 = torch.randn(10, device="cuda", generator=g)
    t = torch.randint(0, 10, (B,), device="cuda", generator=g)
    tb = torch.randint(0, 10, (B,), device="cuda", generator=g)
    tb[0] = t[0]
    lam = torch.tensor([0.3], device="cuda")
    if link:
        torch.manual_seed(0)
        conv = torch.nn.Conv2d(512, 512, 3, padding=1).cuda().to(memory_format=torch.channels_last)
        bn = torch.nn.BatchNorm2d(512).cuda()
        xin = torch.randn(B, 512, 2, 2, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    else:
        x0 = torch.randn(B, 512, device="cuda", generator=g)

    def run(fused):
        monkeypatch.setenv("CDP_FUSED_CLASSIFIER", "1" if fused else "0")
        w = w0.clone().requires_grad_()
        b = b0.clone().requires_grad_()
        n0 = CF.LINK_HANDOFFS[0]
        if link:
            conv.zero_grad(set_to_none=True)
            bn.zero_grad(set_to_none=True)
            bn.running_mean.zero_(); bn.running_var.fill_(1.0); bn.num_batches_tracked.zero_()
            h = CF.conv_bn_act(xin.clone().requires_grad_(), conv, bn, relu=True, pool=True, bn_link=True)
            x = h.reshape(B, -1)
            CF.pass_link(h, x)
            x.retain_grad()
        else:
            x = x0.clone().requires_grad_()
        logits = CF.linear(x, w, b)
        logits.retain_grad()
        loss = CF.cross_entropy(logits, t, label_smoothing=eps, target_b=tb, lam=lam)
        (loss * 0.5).backward()  # a non-unit incoming gradient
        torch.cuda.synchronize()
        return [logits.grad, x.grad, w.grad, b.grad], x.detach().clone(), CF.LINK_HANDOFFS[0] - n0

    (fz, xf, hf), (un, xu, hu) = run(True), run(False)
    assert torch.equal(xf, xu)
    if link:
        assert hf == hu + 1, (hf, hu)
    xd = xf.double().requires_grad_()
    wd = w0.double().requires_grad_()
    bd = b0.double().requires_grad_()
    ld = F.linear(xd, wd, bd)
    ld.retain_grad()
    lm = lam.item()
    ((lm * F.cross_entropy(ld, t, label_smoothing=eps) + (1 - lm) * F.cross_entropy(ld, tb, label_smoothing=eps))
     * 0.5).backward()
    ref = [ld.grad, xd.grad, wd.grad, bd.grad]
    for name, a, u, r in zip(["dlogits", "dx", "dw", "db"], fz, un, ref):
        assert torch.equal(a, u), (name, (a - u).abs().max().item())
        print(f"{name}: rel err {rel_err(a, r):.3e}")
        assert rel_err(a, r) < 1e-5, name


# ------------------------------------------------------------------------------- whole step
def _step_setup(mix=True):
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, synthetic_cifar10

    torch.manual_seed(0)
    m = cdp.VGG11().cuda()
    o = cdp.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    ds = synthetic_cifar10(64, device="cuda")
    kw = dict(mixup_alpha=0.2, cutmix_alpha=1.0) if mix else {}
    ld = DeviceLoader(ds, 16, seed=9, **kw)
    assert ld.advance_with(o)
    idx = torch.arange(64, device="cuda")
    crit = cdp.CrossEntropyLoss(label_smoothing=0.1)

    def body():
        o.zero_grad()
        data, tgt = ld.batch(idx, 0, 16, nbatches=4)
        loss = crit(m(data), tgt)
        loss.backward()
        o.step()
        return loss, tgt

    return m, o, ld, body


def test_captured_mixed_step_replays_bitwise_like_eager():
    """VGG-11, batch 16, mixup + CutMix + label smoothing, the optimizer advancing the loader's counter:
    one captured step replayed 6 times equals a twin's 7 eager steps bitwise (losses, parameters); the
    published lam changes between replays and every published row is mix_params at that counter."""
    lib = _lib()
    mE, oE, lE, bodyE = _step_setup()
    mG, oG, lG, bodyG = _step_setup()
    for _ in range(3):  # warm-up of both twins (allocator, arenas), in lockstep
        bodyE(); bodyG()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        bodyG()
    torch.cuda.current_stream().wait_stream(s)
    bodyE()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        lo, tg = bodyG()
    torch.cuda.synchronize()
    lams = []
    for i in range(7):
        ctr = int(lE._counter.item())
        assert ctr == int(lG._counter.item())
        le, te = bodyE()
        gr.replay()
        torch.cuda.synchronize()
        assert lo.item() == le.item() and math.isfinite(le.item()), (i, lo.item(), le.item())
        for (n, a), b in zip(mE.named_parameters(), mG.parameters()):
            assert torch.equal(a, b), (i, n)
        want = lib.mix_params(9, ctr, 1, 0.2, 1.0, 1.0, 0.5, 32, 32)[0]
        assert torch.equal(tg.info, want) and torch.equal(te.info, want), (i, ctr)
        assert torch.equal(tg.target, te.target) and torch.equal(tg.target_b, te.target_b)
        lams.append(tg.lam.item())
    assert len(set(lams)) > 1, lams


def _kernel_names(body):
    """Names of the GPU kernels one call of body launches."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        body()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
            and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def test_mixing_adds_no_launch_to_the_step():
    """One eager step with mixing on launches no more kernels than with mixing off: the mix rides in the
    augment launch, and the classifier backward is still the one xent_linear_bwd launch."""
    from collections import Counter

    names = {}
    for mix in (False, True):
        _, _, _, body = _step_setup(mix)
        for _ in range(3):
            body()
        _kernel_names(body)  # (a first profiled step also records whatever the profiler itself sets up)
        names[mix] = _kernel_names(body)
        assert names[mix], "the profiler recorded no kernel"
        assert sum("xent_linear_bwd" in n for n in names[mix]) == 1, names[mix]
        assert sum("xent_bwd" in n for n in names[mix]) == 0, names[mix]
        assert sum("augment_kernel" in n for n in names[mix]) == 1, names[mix]
        assert sum("mix_params" in n for n in names[mix]) == 0, names[mix]
    # The eager act-max slot pool zero-fills a fresh chunk (fill_u32*) at whichever step uses the last
    # chunk up: that launch comes every few steps with mixing on or off, so it is not part of the comparison.
    step = {m: [n for n in names[m] if "fill_u32" not in n] for m in names}
    off, on = Counter(step[False]), Counter(step[True])
    print(f"launches per step: mixing off {len(step[False])}, on {len(step[True])} (slot fills: off "
          f"{len(names[False]) - len(step[False])}, on {len(names[True]) - len(step[True])}); only off "
          f"{sorted(off - on)}, only on {sorted(on - off)}")
    assert len(step[True]) == len(step[False])
    # the same kernels, but for the three instantiations that carry the mix
    swapped = sorted(re.search(r"(\w+_kernel)<", n).group(1) for n in (on - off))
    assert swapped == ["augment_kernel", "xent_fwd_kernel", "xent_linear_bwd_kernel"], sorted(on - off)
