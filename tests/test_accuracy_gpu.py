"""fp32-class accuracy of the conv GEMM engines, per element and over a training run.

1. Per element: every output of the forward, data-gradient and weight-gradient GEMMs must satisfy
   the fp32 dot-product error bound

       |y - y_fp64| <= c * (2^-22 + K * 2^-24) * sum_i |a_i| |b_i|        (c = 4)

   where K is the reduction length (Ci*k*k forward, Co*k*k dgrad, N*P*Q wgrad). Global RMS or
   max-normalised errors (tests/test_kernels_gpu.py) are dominated by the large outputs and cannot
   see an output whose inputs all sit far below the tensor maximum; this bound can. Data: Gaussian,
   heavy-tailed (log-normal magnitudes), and structured dynamic range -- whole images or whole
   channels scaled down by up to 2^-42 (e.g. the loss gradient of confidently classified images).
   Every engine meets the bound on all of them: the f16x2 engine scales each GEMM row by its own
   image's / channel's maximum (csrc/kernels/x3_common.h). Its one remaining limit -- dynamic range
   of more than ~2^17 WITHIN one image along the reduction -- is pinned by
   test_f16x2_intra_image_range_limit.
2. Over a run: VGG-11 trained 100 steps at the reference hyperparameters (lr 0.1, momentum 0.9,
   wd 1e-4, B=256; /root/reference/src/Part 1/main.py:114-115) through the native engine follows
   the torch fp32 (MIOpen) loss curve from the same init as closely as fp32 rounding noise itself
   allows (a torch run from an init perturbed by 2^-23 relative sets the band).
"""
import os

import pytest
import torch
import torch.nn.functional as F

from _gemm_util import check_bound, make_data

pytestmark = pytest.mark.gpu

ENGINES = ["f16x2", "x3", "f32"]

CASES = [
    # N, C, H, W, Co, k, s, p
    (8, 3, 32, 32, 64, 3, 1, 1),      # VGG layer 0 (K = 27)
    (8, 64, 16, 16, 128, 3, 1, 1),    # VGG layer 1
    (8, 128, 8, 8, 256, 3, 1, 1),
    (8, 256, 8, 8, 256, 3, 1, 1),
    (8, 256, 4, 4, 512, 3, 1, 1),
    (8, 512, 2, 2, 512, 3, 1, 1),     # split-K regime
    (3, 64, 14, 14, 64, 1, 1, 0),     # 1x1, M tail
    (2, 64, 15, 15, 128, 3, 2, 1),    # strided 3x3, odd size
    (2, 128, 14, 14, 256, 1, 2, 0),   # 1x1 stride-2 downsample
    (2, 3, 64, 64, 64, 7, 2, 3),      # ResNet stem
]


def C():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _data(kind, shape, gen):
    return make_data(kind, shape, gen)


def _check(name, got, ref, absref, K):
    return check_bound(name, got, ref, absref, K)


KINDS = ["normal", "heavy", "image_spread", "channel_spread"]


@pytest.mark.parametrize("engine,kind", [pytest.param(e, k, id=f"{e}-{k}") for e in ENGINES for k in KINDS])
@pytest.mark.parametrize("N,Ci,H,W,Co,k,s,p", CASES)
def test_conv_gemms_meet_fp32_error_bound_per_element(engine, kind, N, Ci, H, W, Co, k, s, p):
    gen = torch.Generator().manual_seed(7)
    x = _data(kind, (N, Ci, H, W), gen)
    w = (torch.randn(Co, Ci, k, k, generator=gen) * (1.0 / (Ci * k * k) ** 0.5)).float()
    xd, wd = x.double(), w.double()
    y_ref = F.conv2d(xd, wd, None, s, p)
    P, Q = y_ref.shape[2], y_ref.shape[3]
    gy = _data(kind, tuple(y_ref.shape), gen)
    gyd = gy.double()
    # exact fp64 references and the sum_i |a_i||b_i| of every output
    xr = xd.clone().requires_grad_()
    wr = wd.clone().requires_grad_()
    F.conv2d(xr, wr, None, s, p).backward(gyd)
    abs_y = F.conv2d(xd.abs(), wd.abs(), None, s, p)
    xa = torch.zeros_like(xd, requires_grad=True)
    F.conv2d(xa, wd.abs(), None, s, p).backward(gyd.abs())
    wa = torch.zeros_like(wd, requires_grad=True)
    F.conv2d(xd.abs(), wa, None, s, p).backward(gyd.abs())

    xc, wc, gyc = cl(x.cuda()), cl(w.cuda()), cl(gy.cuda())
    orig = C().get_conv_gemm()
    try:
        C().set_conv_gemm(engine)
        y = C().conv2d_fwd(xc, wc, None, s, p, False)[0]
        dx = C().conv2d_dgrad(gyc, wc, list(x.shape), s, p)
        dw = C().conv2d_wgrad(gyc, xc, list(w.shape), s, p)
        torch.cuda.synchronize()
    finally:
        C().set_conv_gemm(orig)
    r = (_check("fwd", y, y_ref, abs_y, Ci * k * k),
         _check("dgrad", dx, xr.grad, xa.grad, Co * k * k),
         _check("wgrad", dw, wr.grad, wa.grad, N * P * Q))
    print(f"{engine} {kind} {(N, Ci, H, W, Co, k, s, p)} worst err/bound fwd {r[0]:.2e} dgrad {r[1]:.2e} "
          f"wgrad {r[2]:.2e}")


@pytest.mark.parametrize("engine", ["f16x2", "x3"])
def test_f16x2_intra_image_range_limit(engine):
    """The f16x2 engine's documented limit, pinned: its A-operand scale is per IMAGE, so values more
    than ~2^17 below their own image's maximum lose the low fp16 term (absolute error ~2^-39 of the
    image max). Here every image holds one pixel 2^40 above the rest: the outputs whose windows miss
    that pixel are then outside the fp32 bound for f16x2 (asserted), while x3 -- a bf16 split with an
    8-bit exponent per term -- meets it. Whole-image and whole-channel spreads, the cases a per-row
    scale can see, pass for every engine (test_conv_gemms_meet_fp32_error_bound_per_element)."""
    N, Ci, H, W, Co = 4, 64, 8, 8, 64
    gen = torch.Generator().manual_seed(11)
    x = _data("pixel_spread", (N, Ci, H, W), gen)
    w = (torch.randn(Co, Ci, 3, 3, generator=gen) * (1.0 / (Ci * 9) ** 0.5)).float()
    xd, wd = x.double(), w.double()
    y_ref = F.conv2d(xd, wd, None, 1, 1)
    abs_y = F.conv2d(xd.abs(), wd.abs(), None, 1, 1)
    orig = C().get_conv_gemm()
    try:
        C().set_conv_gemm(engine)
        y = C().conv2d_fwd(cl(x.cuda()), cl(w.cuda()), None, 1, 1, False)[0]
        torch.cuda.synchronize()
    finally:
        C().set_conv_gemm(orig)
    bound = 4.0 * (2.0 ** -22 + Ci * 9 * 2.0 ** -24) * abs_y + 1e-300
    ratio = ((y.double().cpu() - y_ref).abs() / bound).max().item()
    print(f"{engine}: worst err/bound with 2^40 intra-image spread {ratio:.3g}")
    if engine == "x3":
        assert ratio <= 1.0
    else:
        assert ratio > 1.0, "f16x2 met the bound on intra-image spread: update the documented limit"


def test_act_max_matches_torch_per_image_and_channel():
    """The standalone act max pass: exact per-image and per-channel |max| (every copy's max over the
    kActCopies copies), for 4-D NHWC (float4 and scalar channel paths, C / 4 above 256) and 2-D."""
    if C().get_conv_gemm() != "f16x2":
        pytest.skip("act max exists for the f16x2 engine only")
    K = C().act_max_copies()
    gen = torch.Generator(device="cuda").manual_seed(5)
    for shape in [(8, 64, 16, 16), (3, 3, 7, 9), (5, 2048, 2, 2), (2, 1024, 3, 3), (300, 96, 1, 1), (7, 12, 5, 5)]:
        t = torch.randn(shape, device="cuda", generator=gen) * torch.exp(
            3 * torch.randn(shape, device="cuda", generator=gen))
        s = C().act_max(cl(t))
        n, c = shape[0], shape[1]
        assert s.dtype == torch.int32 and s.numel() >= n + K * c
        img = s[:n].view(torch.float32)
        ch = s[n:n + K * c].view(torch.float32).view(K, c).amax(0)
        assert torch.equal(img, t.abs().amax(dim=(1, 2, 3))), shape
        assert torch.equal(ch, t.abs().amax(dim=(0, 2, 3))), shape
    t2 = torch.randn(37, 200, device="cuda", generator=gen)
    s2 = C().act_max(t2)
    assert torch.equal(s2[:37].view(torch.float32), t2.abs().amax(1))
    assert torch.equal(s2[37:37 + K * 200].view(torch.float32).view(K, 200).amax(0), t2.abs().amax(0))


def test_act_max_slots_ordered_across_streams():
    """Act max slots are views into chunks that one memset zeroes. A producer on another stream that
    takes slots from a chunk whose memset is still queued behind a busy stream must wait for it, or
    the late memset wipes what it wrote (csrc/runtime/ops.cpp alloc_slots, order_after)."""
    if C().get_conv_gemm() != "f16x2":
        pytest.skip("act max exists for the f16x2 engine only")
    K = C().act_max_copies()
    gen = torch.Generator(device="cuda").manual_seed(9)
    # eager slot chunks hold 2^16 slots: 0.61 of one, twice, makes the second start a chunk of its own
    tx = torch.randn(64, 4992, device="cuda", generator=gen)  # 64 + 8 x 4992 = 40000 slots
    tb = torch.randn(64, 4992, device="cuda", generator=gen)  # 40000 more: a new chunk, zeroed on s1
    tc = torch.randn(32, 2336, device="cuda", generator=gen)  # 18720 more: the same chunk, used on s2
    mx = C().act_max(tx)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    s1.wait_stream(torch.cuda.current_stream())
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s1):
        C().gpu_sleep(3000.0)  # the chunk's memset and s1's pass queue behind 3 ms
        mb = C().act_max(tb)
    with torch.cuda.stream(s2):
        mc = C().act_max(tc)
    torch.cuda.synchronize()
    assert torch.equal(mb[:64].view(torch.float32), tb.abs().amax(1))
    assert torch.equal(mx[:64].view(torch.float32), tx.abs().amax(1))
    assert torch.equal(mc[:32].view(torch.float32), tc.abs().amax(1))
    assert torch.equal(mc[32:32 + K * 2336].view(torch.float32).view(K, 2336).amax(0), tc.abs().amax(0))


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("N,Co,HW", [(32, 64, 16), (8, 512, 2), (256, 128, 8), (4, 2048, 2), (4, 4096, 2)])
def test_bn_producers_write_exact_act_max(N, Co, HW, pool):
    """The fused block forward's output carries the exact per-image / per-channel |max| of what its
    BatchNorm-apply kernel wrote (bn_fin_act or bn_act_fwd, whichever the shape takes)."""
    if C().get_conv_gemm() != "f16x2":
        pytest.skip("act max exists for the f16x2 engine only")
    if pool and HW < 2:
        pytest.skip("no pooling below 2x2")
    K = C().act_max_copies()
    gen = torch.Generator(device="cuda").manual_seed(N + Co)
    x = cl(torch.randn(N, 64, HW, HW, device="cuda", generator=gen))
    w = cl(torch.randn(Co, 64, 3, 3, device="cuda", generator=gen) * 0.05)
    b = torch.randn(Co, device="cuda", generator=gen)
    g = torch.rand(Co, device="cuda", generator=gen) + 0.5
    be = torch.randn(Co, device="cuda", generator=gen)
    out, _, _, _, amax, _, _, _ = C().conv_bn_act_fwd(x, w, b, g, be, None, None, None, 0.1, 1e-5, True, 1, 1, pool,
                                                   True, None)
    torch.cuda.synchronize()
    assert torch.equal(amax[:N].view(torch.float32), out.abs().amax(dim=(1, 2, 3)))
    assert torch.equal(amax[N:N + K * Co].view(torch.float32).view(K, Co).amax(0), out.abs().amax(dim=(0, 2, 3)))


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("N,Co,HW", [(16, 128, 8), (8, 512, 4), (2, 4096, 4)])
def test_bn_backward_producers_write_act_max(N, Co, HW, pool, fused, monkeypatch):
    """The fused block backward's dy act max (bn_bwd_fin_apply or bn_bwd_apply) matches the
    per-image / per-channel |max| of dy recomputed by torch in fp32 from the same statistics (to
    1e-5: torch's evaluation order of the BatchNorm backward formula differs in the last bits)."""
    if C().get_conv_gemm() != "f16x2":
        pytest.skip("act max exists for the f16x2 engine only")
    monkeypatch.setenv("CDP_BN_BWD_FIN", fused)
    K = C().act_max_copies()
    gen = torch.Generator(device="cuda").manual_seed(N * Co)
    x = cl(torch.randn(N, 64, HW, HW, device="cuda", generator=gen))
    w = cl(torch.randn(Co, 64, 3, 3, device="cuda", generator=gen) * 0.05)
    b = torch.randn(Co, device="cuda", generator=gen)
    g = torch.rand(Co, device="cuda", generator=gen) + 0.5
    be = torch.randn(Co, device="cuda", generator=gen)
    out, y, stats, xs, _, xa, wa, _ = C().conv_bn_act_fwd(x, w, b, g, be, None, None, None, 0.1, 1e-5, True, 1, 1, pool,
                                                       True, None)
    gout = cl(torch.randn(out.shape, device="cuda", generator=gen))
    r = C().conv_bn_act_bwd(gout, xs, w, y, stats, 1, 1, pool, True, True, True, None, True, None, None, None, None,
                            None, xa, wa)
    dy_amax = r[7]
    torch.cuda.synchronize()
    # torch fp32: dz through max-pool (first max wins) and ReLU, then the BatchNorm backward
    yr = y.detach().clone().requires_grad_()
    z = torch.relu(yr * stats[2].view(1, -1, 1, 1) + stats[3].view(1, -1, 1, 1))
    if pool:
        z = torch.nn.functional.max_pool2d(z, 2, 2)
    (dz,) = torch.autograd.grad(z, yr, gout)
    dz = dz / stats[2].view(1, -1, 1, 1)
    xh = (y - stats[0].view(1, -1, 1, 1)) * stats[1].view(1, -1, 1, 1)
    M = y.numel() // Co
    dy = stats[2].view(1, -1, 1, 1) * (dz - dz.sum((0, 2, 3), keepdim=True) / M
                                       - xh * (dz * xh).sum((0, 2, 3), keepdim=True) / M)
    img = dy_amax[:N].view(torch.float32)
    ch = dy_amax[N:N + K * Co].view(torch.float32).view(K, Co).amax(0)
    torch.testing.assert_close(img, dy.abs().amax(dim=(1, 2, 3)), rtol=1e-5, atol=0)
    torch.testing.assert_close(ch, dy.abs().amax(dim=(0, 2, 3)), rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------- long run
def _synthetic_task(steps, B, gen, distinct=8):
    """Learnable CIFAR-shaped task: the label is the argmax of a fixed random projection of the
    4x4-average-pooled image; ``distinct`` batches are cycled (epochs over a small training set)."""
    proj = torch.randn(10, 3 * 4 * 4, generator=gen)
    xs, ys = [], []
    for _ in range(distinct):
        x = torch.randn(B, 3, 32, 32, generator=gen)
        feat = F.adaptive_avg_pool2d(x, 4).reshape(B, -1)
        xs.append(x)
        ys.append((feat @ proj.t()).argmax(1))
    return [xs[i % distinct] for i in range(steps)], [ys[i % distinct] for i in range(steps)]


def _train(model, opt, crit, xs, ys, reference):
    prev = os.environ.get("CDP_FORCE_REFERENCE")
    os.environ["CDP_FORCE_REFERENCE"] = "1" if reference else "0"
    losses = []
    try:
        model.train()
        for x, y in zip(xs, ys):
            x, y = x.cuda(non_blocking=True), y.cuda(non_blocking=True)
            if not reference:
                x = cl(x)
            opt.zero_grad()
            loss = crit(model(x), y)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
        torch.cuda.synchronize()
    finally:
        if prev is None:
            os.environ.pop("CDP_FORCE_REFERENCE", None)
        else:
            os.environ["CDP_FORCE_REFERENCE"] = prev
    return torch.stack(losses).double().cpu()


@pytest.mark.parametrize("engine", ["f16x2", "x3"])
def test_vgg11_loss_curve_tracks_torch_fp32(engine):
    import cs744_distributed_data_parallel_amd as cdp

    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    steps, B = 100, 256
    xs, ys = _synthetic_task(steps, B, torch.Generator().manual_seed(3))
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in cdp.VGG11(channels_last=False).state_dict().items()}

    def torch_run(perturb):
        m = cdp.VGG11(channels_last=False)
        m.load_state_dict(init)
        if perturb:
            g = torch.Generator().manual_seed(11)
            with torch.no_grad():
                for prm in m.parameters():
                    prm.mul_(1 + 2.0 ** -23 * torch.randn(prm.shape, generator=g))
        m = m.cuda()
        opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        return _train(m, opt, torch.nn.CrossEntropyLoss(), xs, ys, reference=True)

    ref = torch_run(False)
    pert = torch_run(True)
    orig = C().get_conv_gemm()
    try:
        C().set_conv_gemm(engine)
        m = cdp.VGG11()
        m.load_state_dict(init)
        m = m.cuda()
        opt = cdp.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        nat = _train(m, opt, cdp.CrossEntropyLoss(), xs, ys, reference=False)
    finally:
        C().set_conv_gemm(orig)
    noise = (pert - ref).abs()
    dev = (nat - ref).abs()
    print(f"{engine}: loss ref {ref[0]:.4f} -> {ref[-1]:.4f}, native {nat[0]:.4f} -> {nat[-1]:.4f}; "
          f"mean |native-ref| {dev.mean():.2e} vs fp32-noise {noise.mean():.2e}; "
          f"max {dev.max():.2e} vs {noise.max():.2e}")
    assert torch.isfinite(nat).all()
    assert ref[-10:].mean() < ref[0]  # below the initial loss after the early lr-0.1 transient
    # the first two steps see (nearly) identical weights: rounding-level agreement (from step 3 on
    # the lr-0.1 transient amplifies any rounding difference, which is what the band is for)
    assert (dev[:2] <= 1e-4 * ref[:2].abs() + 1e-5).all(), dev[:5]
    # over the run: within the spread that fp32 rounding noise itself induces (+ a small floor)
    assert dev.mean() <= 3.0 * noise.mean() + 0.02, (dev.mean(), noise.mean())
    assert abs(nat[-10:].mean() - ref[-10:].mean()) <= 3.0 * (pert[-10:].mean() - ref[-10:].mean()).abs() + 0.05


# --------------------------------------------------------------------- headline GEMM plans
# VGG-11 layers 1-7 (layer 0 runs the exact-fp32 stem kernels, test_kernels_gpu.py) at the bench's
# batch (B=256) and at the reference's 8-rank strong-scaling batch (B=32): the conv entry points
# plan tiles and split-K exactly as the training step does (plan_gemm / plan_wgrad in
# csrc/runtime/ops.cpp), so these launches are the headline's GEMM configurations.
VGG_LAYERS = [(64, 128, 16), (128, 256, 8), (256, 256, 8), (256, 512, 4), (512, 512, 4), (512, 512, 2),
              (512, 512, 2)]


def _patches(xp, n, p, q):
    """[S, Ci*9] rows of the zero-padded input around output pixels (n, p, q), (ci, kh, kw) order."""
    idx_h = p[:, None] + torch.arange(3, device=xp.device)[None, :]
    idx_w = q[:, None] + torch.arange(3, device=xp.device)[None, :]
    g = xp[n[:, None, None, None], torch.arange(xp.shape[1], device=xp.device)[None, :, None, None],
           idx_h[:, None, :, None], idx_w[:, None, None, :]]
    return g.reshape(len(n), -1)


@pytest.mark.parametrize("engine", ["f16x2", "x3"])
@pytest.mark.parametrize("B", [256, 32])
@pytest.mark.parametrize("layer", range(1, 8))
def test_headline_plan_gemms_meet_fp32_bound_on_samples(engine, B, layer):
    Ci, Co, HW = VGG_LAYERS[layer - 1]
    gen = torch.Generator(device="cuda").manual_seed(100 + layer)
    x = torch.randn(B, Ci, HW, HW, device="cuda", generator=gen)
    w = torch.randn(Co, Ci, 3, 3, device="cuda", generator=gen) * (1.0 / (Ci * 9) ** 0.5)
    gy = torch.randn(B, Co, HW, HW, device="cuda", generator=gen)
    orig = C().get_conv_gemm()
    try:
        C().set_conv_gemm(engine)
        y = C().conv2d_fwd(cl(x), cl(w), None, 1, 1, False)[0]
        dx = C().conv2d_dgrad(cl(gy), cl(w), list(x.shape), 1, 1)
        dw = C().conv2d_wgrad(cl(gy), cl(x), list(w.shape), 1, 1)
        torch.cuda.synchronize()
    finally:
        C().set_conv_gemm(orig)
    xd, wd, gyd = x.double(), w.double(), gy.double()
    S = 4096 // Co + 1  # output pixels sampled for fwd (x Co columns >= 4096 outputs)
    n = torch.randint(0, B, (S,), device="cuda", generator=gen)
    p = torch.randint(0, HW, (S,), device="cuda", generator=gen)
    q = torch.randint(0, HW, (S,), device="cuda", generator=gen)
    # forward: y[n, :, p, q] = patches(x) @ W^T
    px = _patches(F.pad(xd, (1, 1, 1, 1)), n, p, q)
    wm = wd.reshape(Co, -1)
    ratios = [_check("fwd", y[n, :, p, q], (px @ wm.t()).cpu(), (px.abs() @ wm.abs().t()).cpu(), Ci * 9)]
    # data gradient: a stride-1 pad-1 conv of gy with the flipped, transposed filter
    S2 = 4096 // Ci + 1
    n2 = torch.randint(0, B, (S2,), device="cuda", generator=gen)
    p2 = torch.randint(0, HW, (S2,), device="cuda", generator=gen)
    q2 = torch.randint(0, HW, (S2,), device="cuda", generator=gen)
    pg = _patches(F.pad(gyd, (1, 1, 1, 1)), n2, p2, q2)
    wt = wd.flip(2, 3).transpose(0, 1).reshape(Ci, -1)
    ratios.append(_check("dgrad", dx[n2, :, p2, q2], (pg @ wt.t()).cpu(), (pg.abs() @ wt.abs().t()).cpu(), Co * 9))
    # weight gradient: whole rows of dW for a few output channels, reduction over all B*HW*HW pixels
    rows = torch.randperm(Co, device="cuda", generator=gen)[: 4096 // (Ci * 9) + 1]
    xu = F.unfold(xd, 3, padding=1)  # [B, Ci*9, HW*HW]
    g_sel = gyd[:, rows].reshape(B, len(rows), -1)
    ref = torch.einsum("bkp,bcp->ck", xu, g_sel)
    absref = torch.einsum("bkp,bcp->ck", xu.abs(), g_sel.abs())
    ratios.append(_check("wgrad", dw[rows].reshape(len(rows), -1), ref.cpu(), absref.cpu(), B * HW * HW))
    print(f"{engine} B={B} layer {layer}: worst err/bound fwd {ratios[0]:.2e} dgrad {ratios[1]:.2e} "
          f"wgrad {ratios[2]:.2e}")
