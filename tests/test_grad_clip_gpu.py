"""Gradient-norm clipping and non-finite step skipping on the GPU (csrc/kernels/grad_norm.hip,
grad_clip.h, the clip block of sgd_kernel / sgd_prep_kernel).

Bounds. grad_sumsq accumulates exact fp64 squares, so the fp64 sum has relative error at most
n * 2^-53 (far below one fp32 ulp for every n here); sqrt and the one rounding to fp32 give
``|norm - fl32(norm_fp64)| <= 1 ulp``. The coefficient is a correctly rounded fp32 division and must
EQUAL ``torch.clamp(max_norm / (norm + 1e-6), max=1.0)`` evaluated in fp32 on the host from the
device's own norm (NaN propagates). Everything that compares two device paths is bitwise.
"""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _C():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


def _sizes():
    C = _C()
    P, chunk = C.grad_norm_parts, C.grad_norm_chunk
    sizes = [1, 3, 4, 5, 1027]
    for k in (1, 2, 5):
        sizes += [4 * 1024 * k - 1, 4 * 1024 * k + 1]
    # the size at which a second workgroup starts, and one workgroup's chunk boundary inside a range
    two = next(n for n in range(4, 1 << 20, 4) if P(n) > 1)
    sizes += [two - 2, two - 1, two, two + 1]
    n0 = 6 * two
    c = chunk(n0)
    assert P(n0) > 2 and c < n0
    sizes += [c - 1, c + 1, n0, n0 + 2]
    # small enough that trailing workgroups get no element
    empty = next(n for n in range(two, 1 << 22, 1024) if (P(n) - 1) * chunk(n) >= n)
    sizes.append(empty + 3)
    for n in sizes:
        # the chunks cover every whole float4 (workgroup 0 takes the n & 3 tail)
        assert 1 <= P(n) <= 1024 and P(n) * chunk(n) >= (n & ~3) and chunk(n) % 1024 == 0
    return sizes, empty + 3


def _data(kind, n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g)
    if kind == "huge":
        x = x * 1e30  # fp32 squares overflow; the fp64 accumulation must not
    elif kind == "inf":
        x[n // 2] = float("inf")
    elif kind == "nan":
        x[n // 3] = float("nan")
    return x


def _norm_coef(x_dev, max_norm, prefill_nan=True):
    """(partials, norm, coef) of the two-launch path on a copy of x_dev."""
    C = _C()
    n = x_dev.numel()
    part = torch.full((C.grad_norm_parts(n),), float("nan"), dtype=torch.float64, device="cuda")
    stats = torch.full((3,), -1.0, device="cuda")
    C.grad_sumsq(x_dev, part)
    g = x_dev.clone()
    C.clip_scale(g, part, max_norm, stats)
    return part, stats[0].cpu(), stats[1].cpu(), g


def _check_norm(norm, x64):
    """|norm - fl32(norm_fp64)| <= 1 ulp (inf / NaN: the same class)."""
    ref = np.float32(np.sqrt(np.sum(np.square(x64), dtype=np.float64)))
    got = np.float32(norm.item())
    if np.isnan(ref) or np.isinf(ref):
        assert np.isnan(got) == np.isnan(ref) and np.isinf(got) == np.isinf(ref), (got, ref)
        return
    assert np.isfinite(got), (got, ref)
    ulp = np.spacing(ref)
    print(f"norm {got!r} ref {ref!r} diff/ulp {abs(float(got) - float(ref)) / float(ulp):.3f}")
    assert abs(float(got) - float(ref)) <= float(ulp), (got, ref)


def _check_coef(coef, norm, max_norm):
    want = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
    assert want.dtype == torch.float32
    if torch.isnan(want):
        assert torch.isnan(coef), (coef, want)
    else:
        assert coef.item() == want.item(), (coef.item(), want.item(), norm.item())


@pytest.mark.parametrize("kind", ["gauss", "huge", "inf", "nan"])
def test_sumsq_and_coefficient_against_fp64(kind):
    sizes, empty = _sizes()
    C = _C()
    for i, n in enumerate(sizes):
        x = _data(kind, n, i)
        xd = x.cuda()
        x64 = x.double().numpy()
        for max_norm in (1.0, 1e35 if kind == "huge" else 1e4):
            part, norm, coef, _ = _norm_coef(xd, max_norm)  # the partials start as NaN: all must be rewritten
            if kind != "nan":
                assert not torch.isnan(part).any(), n
            if n == empty:
                P, ch = C.grad_norm_parts(n), C.grad_norm_chunk(n)
                assert (P - 1) * ch >= n and part[-1].item() == 0.0
            _check_norm(norm, x64)
            if kind == "huge":
                assert torch.isfinite(norm)
            _check_coef(coef, norm, max_norm)


def test_norm_and_coefficient_are_bitwise_reproducible():
    sizes, _ = _sizes()
    for n in (sizes[-1], 1 << 20):
        xd = _data("gauss", n, 7).cuda()
        a = _norm_coef(xd, 1.0)
        b = _norm_coef(xd, 1.0)
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
        assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        assert torch.equal(a[2].view(torch.int32), b[2].view(torch.int32))
        assert torch.equal(a[3], b[3])


# ----------------------------------------------------------------------------- VGG-11 fixtures
def _vgg(seed=0, **kw):
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(seed)
    model = cdp.VGG11().cuda()
    opt = cdp.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, **kw)
    return cdp, model, opt


def _batch(step, B=16):
    g = torch.Generator(device="cuda").manual_seed(1000 + step)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    return x, y


def _fwd_bwd(cdp, model, opt, step):
    x, y = _batch(step)
    opt.zero_grad()
    cdp.CrossEntropyLoss()(model(x), y).backward()


def _pad_mask(arena):
    m = torch.ones(arena.total, dtype=torch.bool)
    for off, n in zip(arena.offsets, arena.numels):
        m[off:off + n] = False
    return m.cuda()


def _state(model, opt):
    ps = [p.detach().clone() for p in model.parameters()]
    ms = [opt.state[p]["momentum_buffer"].detach().clone() for p in model.parameters()]
    return ps + ms


def _same(a, b):
    return all(torch.equal(u, v) for u, v in zip(a, b))


def test_norm_over_the_padded_arena_equals_the_parameter_norm():
    cdp, model, opt = _vgg()
    _fwd_bwd(cdp, model, opt, 0)
    arena = opt._arena
    params = list(model.parameters())
    assert any(p.numel() % 4 for p in params)  # bias 10: the arena does hold pad floats
    s, e = arena.contiguous_range(params)
    assert (s, e) == (0, arena.total) and all(p.grad.data_ptr() == v.data_ptr()
                                              for p, v in zip(arena.params, arena.grad_views()))
    mask = _pad_mask(arena)
    assert int(mask.sum()) > 0 and not arena.grad[mask].any()
    _, norm, _, _ = _norm_coef(arena.grad[s:e], 1.0)
    x64 = torch.cat([p.grad.detach().reshape(-1).double() for p in params]).cpu().numpy()
    _check_norm(norm, x64)


@pytest.mark.parametrize("variant", ["first", "later", "nesterov", "wd0"])
def test_fused_clip_is_bitwise_the_host_grad_scale(variant):
    """sgd_step and sgd_step_prep with the device coefficient against the same entry points with the
    host grad_scale = coef.item(): parameters, momentum, |max| partials and W^T."""
    cdp, model, opt = _vgg()
    C = _C()
    _fwd_bwd(cdp, model, opt, 0)  # registers the weight-prep request; real layout
    arena = opt._arena
    s, e = 0, arena.total
    plan = arena.prep_plan_for(s, e)
    assert plan is not None and "desc" in plan
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randn(arena.total, device="cuda", generator=gen) * 0.1
    g[_pad_mask(arena)] = 0
    buf0 = torch.randn(arena.total, device="cuda", generator=gen) * 0.1
    p0 = arena.data.clone()
    first = variant == "first"
    nest = variant == "nesterov"
    wd = 0.0 if variant == "wd0" else 1e-4
    part = torch.empty(C.grad_norm_parts(e - s), dtype=torch.float64, device="cuda")
    C.grad_sumsq(g, part)
    max_norm = 1.0

    def run(path, clipped, gs=1.0):
        p, buf = p0.clone(), buf0.clone()
        stats = torch.zeros(3, device="cuda")
        kw = dict(clip_part=part, max_norm=max_norm, stats=stats) if clipped else {}
        if path == "sgd_step":
            C.sgd_step(p, g, buf, None, 0.1, 0.9, 0.0, wd, gs, nest, first, False, None, **kw)
            prods = []
        else:
            amax = torch.zeros_like(plan["amax"])
            C.sgd_step_prep(p, g, buf, None, 0.1, 0.9, 0.0, wd, gs, nest, first, False, plan["desc"], plan["meta"],
                            amax, None, **kw)
            prods = [amax] + [t.clone() for t in plan["wts"] if t is not None]
        return [p, buf] + prods, stats

    for path in ("sgd_step", "sgd_step_prep"):
        got, stats = run(path, True)
        coef = stats[1].item()
        assert 0.0 < coef < 1.0, coef  # the clip is active
        _check_coef(stats[1].cpu(), stats[0].cpu(), max_norm)
        want, _ = run(path, False, gs=coef)
        assert len(got) == len(want) and (path == "sgd_step" or len(got) > 3)
        assert _same(got, want), (path, variant)
        assert not torch.equal(got[0], p0)


def test_inactive_clip_is_bitwise_no_clip():
    cdp, m1, o1 = _vgg()
    _, m2, o2 = _vgg(max_grad_norm=1e9)
    for step in range(2):
        _fwd_bwd(cdp, m1, o1, step)
        _fwd_bwd(cdp, m2, o2, step)
        o1.step()
        o2.step()
        assert o2.clip_coef.item() == 1.0 and o2.grad_norm.item() > 0
        assert _same(_state(m1, o1), _state(m2, o2)), step


def test_skip_nonfinite_leaves_the_step_out():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    cdp, model, opt = _vgg(max_grad_norm=1e9, skip_nonfinite=True)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    opt.advance_each_step(ctr)
    for step in range(2):
        _fwd_bwd(cdp, model, opt, step)
        opt.step()
    _fwd_bwd(cdp, model, opt, 2)
    before = _state(model, opt)
    opt._arena.grad[12345] = float("inf")
    opt.step()
    assert _same(before, _state(model, opt))
    assert int(ctr.item()) == 3  # the step counter still advances
    assert opt.skipped_steps.item() == 1 and not np.isfinite(opt.grad_norm.item())
    # the products the skipped step wrote for the next forward are those of the unchanged weights
    x, _ = _batch(3)
    h0 = CF.PREP_HITS[0]
    out = model(x)
    assert CF.PREP_HITS[0] == h0 + 1
    assert opt.refresh_weight_prep()
    assert torch.equal(out, model(x))
    _fwd_bwd(cdp, model, opt, 4)
    opt.step()
    assert opt.skipped_steps.item() == 1 and int(ctr.item()) == 4
    assert not _same(before, _state(model, opt))


def test_skipped_first_step_then_clean_step_equals_one_first_step():
    cdp, m1, o1 = _vgg(skip_nonfinite=True)
    _, m2, o2 = _vgg(skip_nonfinite=True)
    _fwd_bwd(cdp, m1, o1, 0)
    o1._arena.grad[7] = float("nan")
    o1.step()
    assert o1.skipped_steps.item() == 1
    assert all(not opt_buf.any() for opt_buf in [o1._arena.momentum_buffer()])
    _fwd_bwd(cdp, m1, o1, 1)
    o1.step()
    _fwd_bwd(cdp, m2, o2, 1)
    o2.step()
    assert o2.skipped_steps.item() == 0 and o1.skipped_steps.item() == 1
    assert _same(_state(m1, o1), _state(m2, o2))


def test_clip_grad_norm_function():
    import cs744_distributed_data_parallel_amd as cdp

    _, model, opt = _vgg()
    _fwd_bwd(cdp, model, opt, 0)
    arena = opt._arena
    params = list(model.parameters())
    g0 = arena.grad.clone()
    x64 = torch.cat([p.grad.detach().reshape(-1).double() for p in params]).cpu().numpy()
    max_norm = 0.25 * float(np.sqrt(np.sum(np.square(x64))))
    norm = cdp.clip_grad_norm_(model.parameters(), max_norm)
    assert norm.dim() == 0 and norm.is_cuda
    _check_norm(norm.cpu(), x64)
    coef = torch.clamp(max_norm / (norm.cpu() + 1e-6), max=1.0)
    assert coef.item() < 1.0
    assert torch.equal(arena.grad, g0 * coef.cuda())  # exactly g * coef, in place, pads still zero
    assert all(p.grad.data_ptr() == v.data_ptr() for p, v in zip(arena.params, arena.grad_views()))
    # fall-backs: another norm type, a parameter outside the arena -- torch's result
    for extra, kw in ((False, dict(norm_type=float("inf"))), (True, dict())):
        arena.grad.copy_(g0)
        ps = list(params)
        twin = [g.clone() for g in arena.grad_views()]
        if extra:
            q = torch.nn.Parameter(torch.ones(5, device="cuda"))
            q.grad = torch.full((5,), 3.0, device="cuda")
            ps.append(q)
            twin.append(q.grad.clone())
        holders = [torch.nn.Parameter(torch.empty_like(t)) for t in twin]
        for h, t in zip(holders, twin):
            h.grad = t
        n1 = cdp.clip_grad_norm_(ps, 0.5, **kw)
        n2 = torch.nn.utils.clip_grad_norm_(holders, 0.5, **kw)
        assert torch.equal(n1, n2)
        for p, h in zip(ps, holders):
            assert torch.equal(p.grad, h.grad)
    with pytest.raises(RuntimeError, match="non-finite"):
        arena.grad[3] = float("inf")
        cdp.clip_grad_norm_(params, 1.0, error_if_nonfinite=True)


def test_captured_step_clips_with_each_replays_norm():
    """Four replays of a captured VGG-11 step (16 images) against four eager steps of a twin; then a
    captured opt.step() alone with an inf poked into the gradient arena between replays."""
    runs = []
    xb, yb = (torch.empty_like(t) for t in _batch(0))
    for _ in range(2):
        cdp, model, opt = _vgg(max_grad_norm=1.0, skip_nonfinite=True)
        opt.param_groups[0]["lr"] = 0.05
        runs.append((model, opt))
    crit = cdp.CrossEntropyLoss()

    def body(model, opt):
        opt.zero_grad()
        crit(model(xb), yb).backward()
        opt.step()

    def feed(step):
        x, y = _batch(step)
        xb.copy_(x)
        yb.copy_(y)

    for step in range(3):
        feed(step)
        for m, o in runs:
            body(m, o)
    feed(3)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for m, o in runs:
            body(m, o)
    torch.cuda.current_stream().wait_stream(s)
    (m1, o1), (m2, o2) = runs
    assert _same(_state(m1, o1), _state(m2, o2))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body(m1, o1)
    norms, coefs = [], []
    for step in range(4, 8):
        feed(step)
        g.replay()
        body(m2, o2)
        torch.cuda.synchronize()
        assert _same(_state(m1, o1), _state(m2, o2)), step
        assert o1.grad_norm.item() == o2.grad_norm.item() and o1.clip_coef.item() == o2.clip_coef.item()
        norms.append(o1.grad_norm.item())
        coefs.append(o1.clip_coef.item())
    assert len(set(norms)) == 4, norms  # each replay's own norm
    assert min(coefs) < 1.0, coefs  # the clip was active
    assert o1.skipped_steps.item() == 0

    # a captured opt.step() alone: only the replay that sees the inf is skipped
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        o1.step()
    torch.cuda.synchronize()
    st0 = _state(m1, o1)
    g2.replay()
    st1 = _state(m1, o1)
    assert not _same(st0, st1) and o1.skipped_steps.item() == 0
    keep = o1._arena.grad[999].clone()
    o1._arena.grad[999] = float("inf")
    g2.replay()
    assert _same(st1, _state(m1, o1)) and o1.skipped_steps.item() == 1
    o1._arena.grad[999] = keep
    g2.replay()
    assert not _same(st1, _state(m1, o1)) and o1.skipped_steps.item() == 1


# ----------------------------------------------------------------------------- one-rank RCCL DDP
DDP_SCRIPT = textwrap.dedent(
    r"""
    import torch
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd import distributed as dist
    dist.init_process_group("rccl", rank=0, world_size=1)
    assert dist.native_communicator() is not None
    crit = cdp.CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(16, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
          for _ in range(4)]
    ys = [torch.randint(0, 10, (16,), device="cuda", generator=g) for _ in range(4)]
    xb = torch.empty_like(xs[0]); yb = torch.empty_like(ys[0])

    def make(kind):
        torch.manual_seed(0)
        model = cdp.VGG11().cuda()
        if kind != "plain":
            model = cdp.DistributedDataParallel(model)
        opt = cdp.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, max_grad_norm=1.0)
        if kind == "overlap":
            model.overlap_optimizer(opt)
        return model, opt

    runs = {k: make(k) for k in ("plain", "ddp", "overlap")}

    def body(model, opt):
        opt.zero_grad()
        crit(model(xb), yb).backward()
        opt.step()

    def state(model, opt):
        ps = [p.detach().clone() for p in model.parameters()]
        ms = [opt.state[p]["momentum_buffer"].detach().clone() for p in model.parameters()]
        return ps + ms

    def check(what):
        ref = state(*runs["plain"])
        for k in ("ddp", "overlap"):
            for u, v in zip(ref, state(*runs[k])):
                assert torch.equal(u, v), (what, k)
            assert runs[k][1].clip_coef.item() == runs["plain"][1].clip_coef.item(), (what, k)

    coefs = []
    for step in range(4):
        xb.copy_(xs[step]); yb.copy_(ys[step])
        for m, o in runs.values():
            body(m, o)
        check(f"eager {step}")
        coefs.append(runs["plain"][1].clip_coef.item())
        assert runs["overlap"][0].reducer.stepped_buckets() == 0
    graphs = []
    for m, o in runs.values():
        s = torch.cuda.Stream(); s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            body(m, o)
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            body(m, o)
        graphs.append(gr)
    torch.cuda.synchronize()
    check("after capture")
    for step in range(4):
        xb.copy_(xs[step]); yb.copy_(ys[step])
        for gr in graphs:
            gr.replay()
        torch.cuda.synchronize()
        check(f"replay {step}")
        coefs.append(runs["plain"][1].clip_coef.item())
        assert runs["overlap"][0].reducer.stepped_buckets() == 0
    assert min(coefs) < 1.0, coefs
    dist.destroy_process_group()
    print("CLIP_DDP_OK", coefs)
    """
)


def test_one_rank_ddp_with_max_grad_norm_is_bitwise_the_plain_model():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", DDP_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert "CLIP_DDP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
