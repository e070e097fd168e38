"""cdp.LARS on the GPU (csrc/kernels/lars.hip, lars.h, the LARS block of sgd_kernel / sgd_prep_kernel).

Bounds. The norms pass accumulates exact fp64 squares, so each fp64 sum has relative error at most
n * 2^-53 (far below 2^-24 at these sizes) and q, evaluated in fp64 and rounded once, satisfies
``|q - fl32(q_fp64)| <= 1 ulp``. Given the device's own ratios the update is the existing ``sgd_one``
with gs_eff = (gs * coef) * q and wd_eff = wd_w * q, so it must EQUAL today's non-LARS ``sgd_step``
run per parameter with those two values as host scalars. Everything that compares two device paths
is bitwise.
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


def _pad4(n):
    return (n + 3) // 4 * 4


def _plan(C, arena, slots=None, prep=None):
    n = len(arena.params)
    r = C.lars_plan(arena.data, 0, arena.total, list(arena.offsets), list(arena.numels), [p.dim() for p in arena.params],
                    list(range(n)) if slots is None else slots, prep["desc"] if prep else None,
                    prep["meta"] if prep else None)
    return {"desc": r[0], "meta": r[1], "part": r[2]}


def _lars(C, lp, ratios, eta, eps, exclude):
    return C.LarsStep(desc=lp["desc"], meta=lp["meta"], part=lp["part"], ratios=ratios, trust_coefficient=eta, eps=eps,
                      exclude=exclude)


# ----------------------------------------------------------------------------- synthetic arena
def _synthetic():
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.utils.arena import FlatArena

    C = _C()
    one = 8192  # the largest parameter of one chunk
    assert C.lars_nparts(one) == 1 and C.lars_chunk(one) == one and C.lars_nparts(one + 1) == 2
    big = 3 * one + 5
    assert C.lars_nparts(big) >= 3
    shapes = [(1,), (3,), (4,), (5,), (10,), (64,), (8, 3, 3, 3), (32, 32, 3, 3), (40, 36, 3, 3), (10, 512), (one,),
              (one + 1,), (big,), (7, 9), (6, 5)]
    g = torch.Generator().manual_seed(11)
    ws = [torch.randn(s, generator=g) * 0.05 for s in shapes]
    gs = [torch.randn(s, generator=g) * 0.01 for s in shapes]
    ws[-2].zero_()  # an all-zero weight
    gs[-1].zero_()  # an all-zero gradient
    params = [torch.nn.Parameter(w.cuda()) for w in ws]
    arena = FlatArena(params)
    for p, gg in zip(params, gs):
        p.grad.copy_(gg.cuda())
    for n in (p.numel() for p in params):
        assert C.lars_chunk(n) % 1024 == 0 and 1 <= C.lars_nparts(n) <= 256 and C.lars_nparts(n) * C.lars_chunk(n) >= n
    return cdp, C, arena, ws, gs


def _q64(w, g, eta, wd, eps, gsc=1.0):
    w, g = w.double().numpy().ravel(), g.double().numpy().ravel()
    wn, gn = np.sqrt(np.sum(w * w)), abs(gsc) * np.sqrt(np.sum(g * g))
    return 1.0 if (wn == 0 or gn == 0) else eta * wn / (gn + wd * wn + eps)


def _check_q(got, q64, what):
    ref = np.float32(q64)
    assert np.isfinite(got) and np.isfinite(ref), (what, got, ref)
    ulp = float(np.spacing(ref))
    print(f"{what}: q {got!r} ref {ref!r} diff/ulp {abs(float(got) - float(ref)) / ulp:.3f}")
    assert abs(float(got) - float(ref)) <= ulp, (what, got, ref)


@pytest.mark.parametrize("scale", [1.0, 1e30])
def test_ratios_against_fp64(scale):
    cdp, C, arena, ws, gs = _synthetic()
    eta, wd, eps = 0.02, 1e-3, 1e-8
    arena.grad.mul_(scale)  # 1e30: fp32 squares would overflow; the fp64 accumulation must not
    gs = [(g.cuda() * scale).cpu() for g in gs]
    lp = _plan(C, arena)
    lp["part"].fill_(float("nan"))  # all of them must be rewritten
    ratios = torch.full((len(ws),), float("nan"), device="cuda")
    C.lars_norms(arena.data, arena.grad, lp["desc"], lp["meta"], lp["part"])
    assert not torch.isnan(lp["part"]).any() and torch.isfinite(lp["part"]).all()
    assert lp["part"].numel() == 2 * sum(C.lars_nparts(n) for n in arena.numels)
    p = arena.data.clone()
    C.sgd_step(p, arena.grad, None, None, 0.1, 0.0, 0.0, wd, 1.0, False, True, False,
               lars=_lars(C, lp, ratios, eta, eps, False))
    got = ratios.cpu().numpy()
    for k, (w, g) in enumerate(zip(ws, gs)):
        _check_q(got[k], _q64(w, g, eta, wd, eps), f"param {k} {tuple(w.shape)}")
    assert got[-2] == 1.0 and got[-1] == 1.0  # zero weight, zero gradient
    # with the exclusion the 1-D parameters get exactly 1, the others the same bits
    ratios2 = torch.full((len(ws),), float("nan"), device="cuda")
    C.sgd_step(arena.data.clone(), arena.grad, None, None, 0.1, 0.0, 0.0, wd, 1.0, False, True, False,
               lars=_lars(C, lp, ratios2, eta, eps, True))
    got2 = ratios2.cpu().numpy()
    for k, w in enumerate(ws):
        assert got2[k] == (got[k] if w.dim() > 1 else 1.0)


def test_norms_ratios_and_step_are_bitwise_reproducible():
    cdp, C, arena, ws, gs = _synthetic()

    def run():
        lp = _plan(C, arena)
        lp["part"].fill_(float("nan"))
        ratios = torch.zeros(len(ws), device="cuda")
        C.lars_norms(arena.data, arena.grad, lp["desc"], lp["meta"], lp["part"])
        p = arena.data.clone()
        buf = torch.zeros_like(p)
        C.sgd_step(p, arena.grad, buf, None, 0.1, 0.9, 0.0, 1e-3, 1.0, False, True, False,
                   lars=_lars(C, lp, ratios, 0.02, 1e-8, False))
        return lp["part"].view(torch.int64), ratios.view(torch.int32), p, buf

    a, b = run(), run()
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert not torch.equal(a[2], arena.data)


# ----------------------------------------------------------------------------- VGG-11 fixtures
def _vgg(seed=0, **kw):
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(seed)
    model = cdp.VGG11().cuda()
    hp = dict(momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02)
    hp.update(kw)
    opt = cdp.LARS(model.parameters(), 0.1, **hp)
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


_FIX = {}


def _vgg_arena():
    """One VGG-11 after a 16-image forward/backward (real layout, registered weight-prep request),
    random gradients and momentum with zero pads; shared, and left unchanged, by the tests below."""
    if not _FIX:
        cdp, model, opt = _vgg()
        C = _C()
        _fwd_bwd(cdp, model, opt, 0)
        arena = opt._arena
        prep = arena.prep_plan_for(0, arena.total, cut=True)
        assert prep is not None and "desc" in prep and prep["cut"]
        gen = torch.Generator(device="cuda").manual_seed(5)
        mask = _pad_mask(arena)
        assert int(mask.sum()) > 0
        g = torch.randn(arena.total, device="cuda", generator=gen) * 0.1
        buf0 = torch.randn(arena.total, device="cuda", generator=gen) * 0.1
        g[mask] = 0
        buf0[mask] = 0
        _FIX.update(cdp=cdp, model=model, opt=opt, C=C, arena=arena, prep=prep, g=g, buf0=buf0, mask=mask,
                    p0=arena.data.clone(), plain=_plan(C, arena), prepped=_plan(C, arena, prep=prep))
    return _FIX


def _run_lars(fx, path, *, wd, nest, first, g=None, clip=None, eta=0.02, eps=1e-8, mom=0.9):
    """The LARS step through one entry point on copies (the prep path: on the arena itself, restored
    by the caller): [p, buf, ratios, stats, products...]."""
    C, arena, prep = fx["C"], fx["arena"], fx["prep"]
    g = fx["g"] if g is None else g
    lp = fx["plain"] if path == "sgd_step" else fx["prepped"]
    lp["part"].fill_(float("nan"))
    C.lars_norms(fx["p0"], g, lp["desc"], lp["meta"], lp["part"])
    assert not torch.isnan(lp["part"]).any()
    ratios = torch.full((len(arena.params),), float("nan"), device="cuda")
    stats = torch.zeros(3, device="cuda")
    kw = {}
    if clip is not None:
        part = torch.empty(C.grad_norm_parts(arena.total), dtype=torch.float64, device="cuda")
        C.grad_sumsq(g, part)
        kw = dict(clip_part=part, max_norm=clip, stats=stats)
    buf = fx["buf0"].clone() if mom else None
    lars = _lars(C, lp, ratios, eta, eps, True)
    if path == "sgd_step":
        p = fx["p0"].clone()
        C.sgd_step(p, g, buf, None, 0.1, mom, 0.0, wd, 1.0, nest, first, False, None, lars=lars, **kw)
        return [p, buf, ratios, stats]
    assert torch.equal(arena.data, fx["p0"])
    amax = torch.full_like(prep["amax"], float("nan"))
    C.sgd_step_prep(arena.data, g, buf, None, 0.1, mom, 0.0, wd, 1.0, nest, first, False, prep["desc"], prep["meta"],
                    amax, None, lars=lars, **kw)
    return [arena.data.clone(), buf, ratios, stats, amax] + [t.clone() for t in prep["wts"] if t is not None]


@pytest.mark.parametrize("variant", ["first", "later", "nesterov", "wd0", "clip"])
def test_update_is_bitwise_todays_kernel_per_parameter(variant):
    fx = _vgg_arena()
    C, arena = fx["C"], fx["arena"]
    first, nest = variant == "first", variant == "nesterov"
    wd = 0.0 if variant == "wd0" else 1e-4
    clip = 1.0 if variant == "clip" else None
    for path in ("sgd_step", "sgd_step_prep"):
        try:
            got = _run_lars(fx, path, wd=wd, nest=nest, first=first, clip=clip)
            p, buf, ratios, stats = got[:4]
            q = ratios.cpu().numpy()
            coef = np.float32(1.0)
            if clip is not None:
                coef = np.float32(stats[1].item())
                assert 0.0 < coef < 1.0, coef  # the clip is active
            # today's kernel, one launch per parameter, host scalars recomputed in fp32 from the device's q / coef
            wp, wb = fx["p0"].clone(), fx["buf0"].clone()
            for k, (prm, off, n) in enumerate(zip(arena.params, arena.offsets, arena.numels)):
                matrix = prm.dim() > 1
                assert np.isfinite(q[k]) and (q[k] != 1.0 if matrix else q[k] == 1.0), (k, q[k])
                gsc = np.float32(1.0) * coef
                _check_q(q[k], _q64(fx["p0"][off:off + n].cpu(), fx["g"][off:off + n].cpu(), 0.02, wd, 1e-8, float(gsc))
                         if matrix else 1.0, f"{variant} {path} param {k}")
                gs_eff = np.float32(gsc * q[k])
                wd_eff = np.float32(np.float32(wd if matrix else 0.0) * q[k])
                sl = slice(off, off + _pad4(n))
                C.sgd_step(wp[sl], fx["g"][sl], wb[sl], None, 0.1, 0.9, 0.0, float(wd_eff), float(gs_eff), nest, first,
                           False)
            assert torch.equal(p, wp), (variant, path)
            assert torch.equal(buf, wb), (variant, path)
            assert not torch.equal(p, fx["p0"])
            assert not p[fx["mask"]].any() and not buf[fx["mask"]].any()  # the pad floats stay zero
            if path == "sgd_step_prep":
                # the products are those of the new weights
                weights, want = arena.prep_request
                amax2 = torch.full_like(fx["prep"]["amax"], float("nan"))
                wts2 = [torch.empty_like(t) if t is not None else None for t in fx["prep"]["wts"]]
                C.weight_prep_into([w.data for w in weights], list(want), amax2, wts2)
                assert torch.equal(got[4], amax2)
                assert len(got) > 5 and _same(got[5:], [t for t in wts2 if t is not None])
        finally:
            arena.data.copy_(fx["p0"])


def test_scale_invariance():
    fx = _vgg_arena()
    arena = fx["arena"]
    a = _run_lars(fx, "sgd_step", wd=0.0, nest=False, first=True, eps=0.0, mom=0.0)
    b = _run_lars(fx, "sgd_step", wd=0.0, nest=False, first=True, eps=0.0, mom=0.0, g=fx["g"] * 1024)
    qa, qb = a[2].cpu(), b[2].cpu()
    n_adapted = 0
    for k, (prm, off, n) in enumerate(zip(arena.params, arena.offsets, arena.numels)):
        if prm.dim() > 1:
            n_adapted += 1
            assert qb[k].item() * 1024 == qa[k].item(), k  # exactly 1 / 1024
            assert torch.equal(a[0][off:off + n], b[0][off:off + n]), k
            assert not torch.equal(a[0][off:off + n], fx["p0"][off:off + n])
        else:
            assert qa[k] == 1.0 and qb[k] == 1.0
    assert n_adapted >= 9


def test_optimizer_step_is_the_entry_points_and_survives_relayout():
    """cdp.LARS.step() (prep form after a forward) equals the low-level launches; after a relayout the
    plan is rebuilt and trust_ratios keep the param group's order."""
    cdp, m1, o1 = _vgg()
    _, m2, o2 = _vgg()
    for step in range(2):
        _fwd_bwd(cdp, m1, o1, step)
        _fwd_bwd(cdp, m2, o2, step)
        o1.step()
        o2.step()
    assert o1._lars_fused and o1._lars_plan is not None and o1._arena.prep_valid is not None
    n = len(o2._arena.params)
    o2._arena.relayout(list(reversed(range(n))))
    assert o2._lars_plan is None
    for step in range(2, 4):
        _fwd_bwd(cdp, m1, o1, step)
        _fwd_bwd(cdp, m2, o2, step)
        o1.step()
        o2.step()
        assert _same(_state(m1, o1), _state(m2, o2)), step
        assert torch.equal(o1.trust_ratios, o2.trust_ratios)
    q = o1.trust_ratios.cpu()
    for k, p in enumerate(m1.parameters()):
        assert (q[k] != 1.0) == (p.dim() > 1)


def test_skip_nonfinite_leaves_the_step_out():
    cdp, model, opt = _vgg(skip_nonfinite=True)
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
    assert opt.skipped_steps.item() == 1
    _fwd_bwd(cdp, model, opt, 3)
    opt.step()
    assert opt.skipped_steps.item() == 1 and int(ctr.item()) == 4
    assert not _same(before, _state(model, opt))


def test_captured_step_adapts_with_each_replays_norms():
    """Four replays of a captured VGG-11 step (16 images) against four eager steps of a twin."""
    runs = []
    xb, yb = (torch.empty_like(t) for t in _batch(0))
    for _ in range(2):
        cdp, model, opt = _vgg()
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
    seen = []
    for step in range(4, 8):
        feed(step)
        g.replay()
        body(m2, o2)
        torch.cuda.synchronize()
        assert _same(_state(m1, o1), _state(m2, o2)), step
        assert torch.equal(o1.trust_ratios, o2.trust_ratios)
        seen.append(o1.trust_ratios.clone())
    assert all(not torch.equal(seen[i], seen[j]) for i in range(4) for j in range(i))  # each replay's own norms


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
        opt = cdp.LARS(model.parameters(), 0.05, momentum=0.9, weight_decay=1e-4, trust_coefficient=0.02)
        if kind == "overlap":
            model.overlap_optimizer(opt)
        return model, opt

    runs = {k: make(k) for k in ("plain", "ddp", "overlap")}
    gen0 = runs["ddp"][1]._arena.layout_gen

    def body(model, opt):
        opt.zero_grad()
        crit(model(xb), yb).backward()
        opt.step()

    def state(model, opt):
        ps = [p.detach().clone() for p in model.parameters()]
        ms = [opt.state[p]["momentum_buffer"].detach().clone() for p in model.parameters()]
        return ps + ms + [opt.trust_ratios.clone()]

    def check(what):
        ref = state(*runs["plain"])
        for k in ("ddp", "overlap"):
            for u, v in zip(ref, state(*runs[k])):
                assert torch.equal(u, v), (what, k)

    for step in range(4):
        xb.copy_(xs[step]); yb.copy_(ys[step])
        for m, o in runs.values():
            body(m, o)
        check(f"eager {step}")
        assert runs["overlap"][0].reducer.stepped_buckets() == 0
    # the ready-order relayout after the first iteration was survived
    assert runs["ddp"][1]._arena.layout_gen > gen0, "no relayout happened"
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
        assert runs["overlap"][0].reducer.stepped_buckets() == 0
    q = runs["plain"][1].trust_ratios
    assert (q != 1).sum().item() >= 9
    dist.destroy_process_group()
    print("LARS_DDP_OK")
    """
)


def test_one_rank_ddp_with_lars_is_bitwise_the_plain_model():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", DDP_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert "LARS_DDP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
