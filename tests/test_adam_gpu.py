"""cdp.AdamW / cdp.LAMB on the GPU (csrc/kernels/adam.hip, adam.h).

Bounds, with u = 2^-24 (one fp32 rounding, relative) and the fp64 reference evaluated from the same fp32
inputs with the hyperparameters as Python doubles. The counts are read off ``adam_one`` / ``adam_apply`` /
``adam_prologue`` in adam.hip, a constant converted to fp32 counting as one rounding:

* ``m = fmaf(g, omb1, m * b1)``: b1, omb1, the product, the fma: K_M = 4, relative to the operands'
  magnitude ``b1 |m0| + (1 - b1) |g|`` (the two terms can cancel).
* ``v = fmaf(g * g, omb2, v * b2)``: b2, omb2, g * g, v * b2, the fma: K_V = 5, relative to v itself (all
  terms are positive).
* ``a = (m * rbc1) / fmaf(sqrtf(v), rbc2s, eps)``: m 4, rbc1, the product: 6; v 5 (counted whole although
  the square root halves them), sqrtf, rbc2s, eps, the fma: 9; the division: K_A = 16.
* ``r = fmaf(w, wd, a)``: wd and the fma: K_R = 18.
* ``w' = fmaf(r, -lr, w)``: lr: K = 19 roundings from the inputs to the update ``lr r``; the final fma's own
  rounding is the ``|w64|`` term. LAMB's rate is ``lr * q``: q's rounding and the product, K = 21.

Everything that compares two device paths is bitwise.
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

U = 2.0 ** -24
SLACK = 1.0 + 1e-6  # second-order terms of the first-order counts
K_M, K_V, K_A, K_R, K_W, K_W_LAMB = 4, 5, 16, 18, 19, 21
B1, B2 = 0.9, 0.999
LR = 1e-3


def _C():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


# ----------------------------------------------------------------------------- synthetic arena
_SYN = {}


def _synthetic():
    """The arena of tests/test_lars_gpu.py::_synthetic, with moments; shared and left unchanged."""
    if _SYN:
        return _SYN
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
    mask = torch.ones(arena.total, dtype=torch.bool)
    for off, n in zip(arena.offsets, arena.numels):
        mask[off:off + n] = False
    mask = mask.cuda()
    assert int(mask.sum()) > 0
    gen = torch.Generator(device="cuda").manual_seed(5)
    m0 = torch.randn(arena.total, device="cuda", generator=gen) * 0.01
    v0 = (torch.randn(arena.total, device="cuda", generator=gen) * 0.01).square()
    e0 = arena.data + torch.randn(arena.total, device="cuda", generator=gen) * 0.001
    for t in (m0, v0, e0):
        t[mask] = 0
    assert not arena.data[mask].any() and not arena.grad[mask].any()
    r = C.lars_plan(arena.data, 0, arena.total, list(arena.offsets), list(arena.numels), [p.dim() for p in params],
                    list(range(len(params))), None, None)
    _SYN.update(cdp=cdp, C=C, arena=arena, params=params, mask=mask, w0=arena.data.clone(), g=arena.grad.clone(),
                m0=m0, v0=v0, e0=e0, plan={"desc": r[0], "meta": r[1], "part": r[2]},
                matrix=[p.dim() > 1 for p in params])
    return _SYN


def _step(fx, T, *, lamb=False, wd=0.01, eps=1e-8, lr=LR, exclude=True, ema=False, clip=None, skip_nonfinite=False,
          g=None, moments=True, per_param=False, nan_part=False):
    """One step of the step count T (t = T - 1 on the device) through the entry points, on copies:
    dict(w, m, v, e, q, t, stats)."""
    C, arena = fx["C"], fx["arena"]
    g = fx["g"] if g is None else g
    w = fx["w0"].clone()
    m = fx["m0"].clone() if moments else torch.zeros_like(w)
    v = fx["v0"].clone() if moments else torch.zeros_like(w)
    e = fx["e0"].clone() if ema else None
    state = torch.tensor([T - 1, 0], dtype=torch.int64, device="cuda")
    stats = torch.zeros(4, device="cuda")
    ratios = torch.full((len(arena.params),), float("nan"), device="cuda")
    kw = {}
    if clip is not None or skip_nonfinite:
        part = torch.full((C.grad_norm_parts(arena.total),), float("nan"), dtype=torch.float64, device="cuda")
        C.grad_sumsq(g, part)
        kw = dict(clip_part=part, max_norm=clip if clip is not None else float("inf"), skip_nonfinite=skip_nonfinite)
    if ema:
        coef = torch.tensor([0.99, 1.0 - 0.99], dtype=torch.float64).float().cuda()
    if per_param:
        assert not lamb and not kw
        for k, (off, n) in enumerate(zip(arena.offsets, arena.numels)):
            sl = slice(off, off + n)
            ek = dict(ema=e[sl], ema_coef=coef) if ema else {}
            C.adam_step(w[sl], g[sl], m[sl], v[sl], None, lr, B1, B2, eps, wd, False, state,
                        k == len(arena.offsets) - 1, **ek)
    else:
        if lamb:
            lp = fx["plan"]
            if nan_part:
                lp["part"].fill_(float("nan"))
            lb = C.LambStep(desc=lp["desc"], meta=lp["meta"], part=lp["part"], ratios=ratios, exclude=exclude)
            C.lamb_moments(w, g, m, v, B1, B2, eps, wd, False, state, lb, **kw)
            kw["lamb"] = lb
        if kw.get("clip_part") is not None:
            kw["stats"] = stats
        if ema:
            kw.update(ema=e, ema_coef=coef)
        C.adam_step(w, g, m, v, None, lr, B1, B2, eps, wd, False, state, True, **kw)
    return dict(w=w, m=m, v=v, e=e, q=ratios, t=state, stats=stats,
                part=fx["plan"]["part"].clone() if lamb else None)


def _ref64(fx, T, *, lamb, wd, eps, lr=LR, exclude=True, g=None, moments=True):
    """The step in fp64 (numpy) from the same fp32 inputs, and the magnitudes the bounds need."""
    arena = fx["arena"]
    w = fx["w0"].double().cpu().numpy()
    g = (fx["g"] if g is None else g).double().cpu().numpy()
    m0 = fx["m0"].double().cpu().numpy() if moments else np.zeros_like(w)
    v0 = fx["v0"].double().cpu().numpy() if moments else np.zeros_like(w)
    m = B1 * m0 + (1 - B1) * g
    v = B2 * v0 + (1 - B2) * g * g
    a = (m / (1 - B1 ** T)) / (np.sqrt(v / (1 - B2 ** T)) + eps)
    wdv = np.zeros_like(w)
    qv = np.ones_like(w)
    qs, qb = [], []
    for off, n, mat in zip(arena.offsets, arena.numels, fx["matrix"]):
        sl = slice(off, off + n)
        adapted = mat or not exclude
        wdv[sl] = wd if (adapted or not lamb) else 0.0
        q, bound = 1.0, 0.0
        if lamb and adapted:
            r = a[sl] + wd * w[sl]
            wn, rn = np.sqrt(np.sum(w[sl] ** 2)), np.sqrt(np.sum(r ** 2))
            if wn != 0 and rn != 0:
                q = wn / rn
                an = np.sqrt(np.sum(a[sl] ** 2))
                bound = U * q * (1 + K_R * (an + wd * wn) / rn)
        qv[sl] = q
        qs.append(q)
        qb.append(bound)
    r = a + wdv * w
    return dict(w=w - lr * qv * r, m=m, v=v, a=a, r=r, q=np.array(qs), q_bound=np.array(qb), w0=w, wdv=wdv, qv=qv,
                m_mag=B1 * np.abs(m0) + (1 - B1) * np.abs(g))


def _check(fx, got, ref, what, lamb, lr=LR):
    """The bounds of the module docstring; prints the largest observed ratio to each bound."""
    real = ~fx["mask"].cpu().numpy()
    w, m, v = (got[k].double().cpu().numpy() for k in ("w", "m", "v"))
    kw = K_W_LAMB if lamb else K_W
    bw = U * (np.abs(ref["w"]) + kw * lr * ref["qv"] * (np.abs(ref["a"]) + ref["wdv"] * np.abs(ref["w0"]))) * SLACK
    bm = U * K_M * ref["m_mag"] * SLACK
    bv = U * K_V * ref["v"] * SLACK
    ratios = {}
    for name, err, b in (("w", np.abs(w - ref["w"]), bw), ("m", np.abs(m - ref["m"]), bm), ("v", np.abs(v - ref["v"]), bv)):
        err, b = err[real], b[real]
        assert np.isfinite(err).all(), (what, name)
        ok = err <= b
        ratios[name] = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)))
        print(f"{what}: largest |{name} - {name}64| / bound = {ratios[name]:.3f}")
        assert ok.all(), (what, name, int((~ok).sum()), ratios[name])
    if lamb:
        q = got["q"].double().cpu().numpy()
        err = np.abs(q - ref["q"])
        nz = ref["q_bound"] > 0
        ratios["q"] = float(np.max(err[nz] / ref["q_bound"][nz])) if nz.any() else 0.0
        print(f"{what}: largest |q - q64| / bound = {ratios['q']:.3f}")
        assert (err[nz] <= ref["q_bound"][nz] * SLACK).all(), (what, q, ref["q"])
        assert (q[~nz] == 1.0).all(), (what, q)
    # the arena's pad floats are still exactly zero
    for k in ("w", "m", "v"):
        assert not got[k][fx["mask"]].any(), (what, k)
    return ratios


# ----------------------------------------------------------------------------- test 5
@pytest.mark.parametrize("T", [1, 2, 1000])
def test_adamw_step_against_fp64(T):
    fx = _synthetic()
    for wd in (0.0, 0.01):
        got = _step(fx, T, wd=wd, moments=T > 1)
        ref = _ref64(fx, T, lamb=False, wd=wd, eps=1e-8, moments=T > 1)
        _check(fx, got, ref, f"adamw T={T} wd={wd}", False)
        assert int(got["t"][0]) == T and int(got["t"][1]) == 0
        assert not torch.equal(got["w"], fx["w0"])


@pytest.mark.parametrize("T", [1, 2, 1000])
def test_lamb_step_against_fp64(T):
    fx = _synthetic()
    for wd, exclude in ((0.0, True), (0.01, True), (0.01, False)):
        got = _step(fx, T, lamb=True, wd=wd, eps=1e-6, exclude=exclude, moments=T > 1, nan_part=True)
        ref = _ref64(fx, T, lamb=True, wd=wd, eps=1e-6, exclude=exclude, moments=T > 1)
        _check(fx, got, ref, f"lamb T={T} wd={wd} exclude={exclude}", True)
        q = got["q"].cpu().numpy()
        assert q[-2] == 1.0  # the all-zero weight: |w| = 0
        if T == 1 and wd == 0.0:
            assert q[-1] == 1.0  # the all-zero gradient with zero moments and no decay: |r| = 0
        for k, mat in enumerate(fx["matrix"]):
            if exclude and not mat:
                assert q[k] == 1.0  # (and no decay: the weights are checked against wd = 0 above)
        adapted = ref["q_bound"] > 0  # neither excluded nor degenerate
        assert ((q != 1.0) == adapted).all() and int(adapted.sum()) >= (4 if exclude else 12)
        assert int(got["t"][0]) == T and int(got["t"][1]) == 0


# ----------------------------------------------------------------------------- test 6
def test_lamb_partials_stay_finite_with_gradients_scaled_by_1e30():
    fx = _synthetic()
    C, arena = fx["C"], fx["arena"]
    g = fx["g"] * 1e30  # fp32 squares overflow (v becomes inf); the fp64 partials must not
    got = _step(fx, 1, lamb=True, wd=0.01, eps=1e-6, exclude=False, g=g, moments=False, nan_part=True)
    part = got["part"]
    assert part.numel() == 2 * sum(C.lars_nparts(n) for n in arena.numels)
    assert not torch.isnan(part).any() and torch.isfinite(part).all()  # every pair was rewritten
    assert torch.isfinite(got["q"]).all() and torch.isfinite(got["w"]).all() and torch.isfinite(got["m"]).all()
    assert torch.isinf(got["v"]).any()


# ----------------------------------------------------------------------------- test 7
def _bits(r, keys=("w", "m", "v", "q")):
    return [r[k].view(torch.int32) for k in keys]


@pytest.mark.parametrize("lamb", [False, True])
def test_two_runs_give_the_same_bits(lamb):
    fx = _synthetic()
    a = _step(fx, 3, lamb=lamb, nan_part=True)
    b = _step(fx, 3, lamb=lamb, nan_part=True)
    assert all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))
    assert not torch.equal(a["w"], fx["w0"]) and not torch.equal(a["m"], fx["m0"])


def test_flat_adamw_is_bitwise_the_per_parameter_launches():
    fx = _synthetic()
    a = _step(fx, 3)
    b = _step(fx, 3, per_param=True)
    assert all(torch.equal(x, y) for x, y in zip(_bits(a, ("w", "m", "v")), _bits(b, ("w", "m", "v"))))
    assert int(b["t"][0]) == 3 and int(b["t"][1]) == 0  # only the last launch advanced t


@pytest.mark.parametrize("lamb", [False, True])
def test_ema_rides_along_without_changing_the_step(lamb):
    fx = _synthetic()
    a = _step(fx, 3, lamb=lamb)
    b = _step(fx, 3, lamb=lamb, ema=True)
    assert all(torch.equal(x, y) for x, y in zip(_bits(a), _bits(b)))
    d, omd = np.float32(0.99), np.float32(1.0 - 0.99)
    ed = (fx["e0"] * float(d)).double()  # the fp32 product e * d, then the fma exactly
    want = (b["w"].double() * float(omd) + ed).float()
    assert torch.equal(b["e"], want)
    assert not b["e"][fx["mask"]].any()
    if not lamb:
        c = _step(fx, 3, ema=True, per_param=True)
        assert torch.equal(b["e"], c["e"])


# ----------------------------------------------------------------------------- test 8
@pytest.mark.parametrize("lamb", [False, True])
def test_fused_clip_is_a_step_on_scaled_gradients(lamb):
    fx = _synthetic()
    eps = 1e-6 if lamb else 1e-8
    got = _step(fx, 3, lamb=lamb, eps=eps, clip=0.5, nan_part=True)
    coef = got["stats"][1]
    assert 0.0 < coef.item() < 1.0  # the clip is active
    norm = torch.linalg.vector_norm(fx["g"].double()).item()
    assert abs(got["stats"][0].item() - norm) <= 2 * U * norm
    scaled = fx["g"] * coef  # fp32, as clip_grad_norm_ scales them
    ref = _ref64(fx, 3, lamb=lamb, wd=0.01, eps=eps, g=scaled)
    _check(fx, got, ref, f"clip lamb={lamb}", lamb)
    plain = _step(fx, 3, lamb=lamb, eps=eps, g=scaled, nan_part=True)
    assert all(torch.equal(x, y) for x, y in zip(_bits(got), _bits(plain)))
    assert not torch.equal(got["w"], _step(fx, 3, lamb=lamb, eps=eps)["w"])


@pytest.mark.parametrize("lamb", [False, True])
def test_skip_nonfinite_leaves_the_step_out(lamb):
    fx = _synthetic()
    g = fx["g"].clone()
    g[fx["arena"].offsets[8] + 77] = float("inf")
    got = _step(fx, 3, lamb=lamb, ema=True, skip_nonfinite=True, g=g)
    for k, ref in (("w", "w0"), ("m", "m0"), ("v", "v0"), ("e", "e0")):
        assert torch.equal(got[k].view(torch.int32), fx[ref].view(torch.int32)), k
    assert int(got["t"][0]) == 2 and int(got["t"][1]) == 0  # t stays
    assert got["stats"][2].item() == 1.0 and not torch.isfinite(got["stats"][0])
    ok = _step(fx, 3, lamb=lamb, ema=True, skip_nonfinite=True)  # finite gradients: the step happens
    assert int(ok["t"][0]) == 3 and ok["stats"][2].item() == 0.0 and not torch.equal(ok["w"], fx["w0"])


# ----------------------------------------------------------------------------- test 9
def _flat_optimizer(cls_name, **kw):
    """An optimizer over fresh parameters of the synthetic shapes (their own arena)."""
    import cs744_distributed_data_parallel_amd as cdp

    fx = _synthetic()
    params = [torch.nn.Parameter(p.detach().clone()) for p in fx["params"]]
    return params, getattr(cdp, cls_name)(params, lr=LR, **kw)


def _feed(fx, opt, step):
    g = torch.Generator(device="cuda").manual_seed(400 + step)
    a = opt._arena
    a.grad.copy_(torch.randn(a.total, device="cuda", generator=g) * 0.01)
    a.grad[fx["mask"]] = 0


def _opt_state(params, opt):
    out = [p.detach().clone() for p in params]
    for k in ("exp_avg", "exp_avg_sq", "ema_buffer"):
        out += [opt.state[p][k].detach().clone() for p in params if k in opt.state[p]]
    if hasattr(opt, "trust_ratios"):
        out.append(opt.trust_ratios.clone())
    return out


@pytest.mark.parametrize("cls_name", ["AdamW", "LAMB"])
def test_captured_step_counts_its_own_steps(cls_name):
    fx = _synthetic()
    import cs744_distributed_data_parallel_amd as cdp

    runs = [_flat_optimizer(cls_name, ema_decay=0.99,
                            lr_schedule=cdp.LRSchedule("cosine", total_steps=200, warmup_steps=3)) for _ in range(2)]
    (p1, o1), (p2, o2) = runs
    for o in (o1, o2):  # one eager step: state, plans and the EMA exist before the capture
        _feed(fx, o, 0)
        o.step()
        o.set_adam_step(0)
        o.set_schedule_step(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _feed(fx, o1, 1)
        _feed(fx, o2, 1)
        o1.step()
        o2.step()
    torch.cuda.current_stream().wait_stream(s)
    for o in (o1, o2):
        o.set_adam_step(0)
        o.set_schedule_step(0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o1.step()
    table = o1.lr_schedule_table(0, 8).cpu()
    for step in range(4):
        _feed(fx, o1, 10 + step)
        _feed(fx, o2, 10 + step)
        graph.replay()
        o2.step()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(_opt_state(p1, o1), _opt_state(p2, o2))), step
        assert o1.last_lr.item() == table[step].item() and o2.last_lr.item() == table[step].item()
    assert int(o1.adam_step) == 4 and int(o2.adam_step) == 4 and int(o1.schedule_step) == 4
    # the step count is a device word: a new value takes effect without re-capture
    for o in (o1, o2):
        o.set_adam_step(100)
    _feed(fx, o1, 20)
    _feed(fx, o2, 20)
    graph.replay()
    o2.step()
    torch.cuda.synchronize()
    assert int(o1.adam_step) == 101 and int(o2.adam_step) == 101
    assert all(torch.equal(x, y) for x, y in zip(_opt_state(p1, o1), _opt_state(p2, o2)))


@pytest.mark.parametrize("cls_name", ["AdamW", "LAMB"])
def test_optimizer_fuses_the_clip_and_advances_a_loader_counter(cls_name):
    """step() with max_grad_norm / skip_nonfinite and advance_each_step is the entry points' step on gradients
    scaled by the recorded coefficient; a non-finite gradient leaves everything but the counter."""
    fx = _synthetic()
    p1, o1 = _flat_optimizer(cls_name, max_grad_norm=0.5, skip_nonfinite=True, ema_decay=0.99)
    p2, o2 = _flat_optimizer(cls_name, ema_decay=0.99)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    o1.advance_each_step(ctr)
    for step in range(2):
        _feed(fx, o1, step)
        o1.step()
        assert o1._clip_fused and 0.0 < o1.clip_coef.item() < 1.0
        norm = torch.linalg.vector_norm(o1._arena.grad.double()).item()
        assert abs(o1.grad_norm.item() - norm) <= 2 * U * norm
        o2._arena.grad.copy_(o1._arena.grad * o1.clip_coef)
        o2.step()
        assert all(torch.equal(x, y) for x, y in zip(_opt_state(p1, o1), _opt_state(p2, o2))), step
    before = _opt_state(p1, o1)
    _feed(fx, o1, 2)
    o1._arena.grad[o1._arena.offsets[8] + 3] = float("nan")
    o1.step()
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(before, _opt_state(p1, o1)))
    assert int(o1.adam_step) == 2 and o1.skipped_steps.item() == 1 and int(ctr) == 3


# ----------------------------------------------------------------------------- test 10
def _vgg(cls_name, seed=0, **kw):
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(seed)
    model = cdp.VGG11().cuda()
    opt = getattr(cdp, cls_name)(model.parameters(), lr=LR, **kw)
    return cdp, model, opt


def _batch(step, B=8):
    g = torch.Generator(device="cuda").manual_seed(1000 + step)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    return x, y


def _fwd_bwd(cdp, model, opt, step):
    x, y = _batch(step)
    opt.zero_grad()
    cdp.CrossEntropyLoss()(model(x), y).backward()


@pytest.mark.parametrize("cls_name", ["AdamW", "LAMB"])
def test_optimizer_matches_the_reference_path_and_survives_relayout(cls_name, monkeypatch):
    lamb = cls_name == "LAMB"
    cdp, m1, o1 = _vgg(cls_name, ema_decay=0.9)
    _, m2, o2 = _vgg(cls_name, ema_decay=0.9)
    wd, eps = o1.param_groups[0]["weight_decay"], o1.param_groups[0]["eps"]
    worst = 0.0
    for step in range(3):
        _fwd_bwd(cdp, m1, o1, step)
        # the twin steps from the same weights, moments and gradients, on the reference path
        with torch.no_grad():
            for p, q in zip(m1.parameters(), m2.parameters()):
                q.copy_(p)
                q.grad = p.grad.detach().clone()
                if step:
                    for k in ("exp_avg", "exp_avg_sq"):
                        o2.state[q][k].copy_(o1.state[p][k])
        if step == 2:
            n = len(o1._arena.params)
            o1._arena.relayout(list(reversed(range(n))))  # m, v and the ratios stay with their parameters
            for p, q in zip(m1.parameters(), m2.parameters()):
                assert torch.equal(o1.state[p]["exp_avg"], o2.state[q]["exp_avg"])
                assert torch.equal(o1.state[p]["exp_avg_sq"], o2.state[q]["exp_avg_sq"])
                assert torch.equal(p.grad, q.grad)
        before = [(p.detach().double(), p.grad.double(), o1.state[p]["exp_avg"].double().clone() if step else None,
                   o1.state[p]["exp_avg_sq"].double().clone() if step else None) for p in m1.parameters()]
        o1.step()
        monkeypatch.setenv("CDP_FORCE_REFERENCE", "1")
        o2.step()
        monkeypatch.delenv("CDP_FORCE_REFERENCE")
        assert o1._arena.prep_valid is None
        T = step + 1
        for k, ((w, g, m0, v0), p, q) in enumerate(zip(before, m1.parameters(), m2.parameters())):
            m = (B1 * m0 if step else 0) + (1 - B1) * g
            v = (B2 * v0 if step else 0) + (1 - B2) * g * g
            a = (m / (1 - B1 ** T)) / ((v / (1 - B2 ** T)).sqrt() + eps)
            adapted = p.dim() > 1
            wdp = wd if (adapted or not lamb) else 0.0
            qq = o1.trust_ratios[k].double() if lamb else 1.0
            bound = 3 * U * (w.abs() + (K_W_LAMB if lamb else K_W) * LR * qq * (a.abs() + wdp * w.abs())) * SLACK
            err = (p.detach().double() - q.detach().double()).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert (err <= bound).all(), (step, k, float((err / bound.clamp_min(1e-300)).max()))
            assert not torch.equal(p.detach().double(), w)
        if lamb:
            tq1, tq2 = o1.trust_ratios.double(), o2.trust_ratios.double()
            assert ((tq1 - tq2).abs() <= 64 * U * tq2).all()  # fp32 sums of the reference's r against the fused ones
            assert all((tq1[k] != 1.0) == (p.dim() > 1) for k, p in enumerate(m1.parameters()))
    print(f"{cls_name}: largest |w_fused - w_reference| / (3 x bound) = {worst:.3f}")
    assert int(o1.adam_step) == 3 and int(o2.adam_step) == 3
    # ema_weights exchanges the contents and restores them
    ws = [p.detach().clone() for p in m1.parameters()]
    es = [o1.state[p]["ema_buffer"].detach().clone() for p in m1.parameters()]
    with o1.ema_weights():
        assert all(torch.equal(p.detach(), e) for p, e in zip(m1.parameters(), es))
        assert all(torch.equal(o1.state[p]["ema_buffer"], w) for p, w in zip(m1.parameters(), ws))
    assert all(torch.equal(p.detach(), w) for p, w in zip(m1.parameters(), ws))
    assert all(torch.equal(o1.state[p]["ema_buffer"], e) for p, e in zip(m1.parameters(), es))
    assert not all(torch.equal(w, e) for w, e in zip(ws, es))


def test_sgd_and_lars_allocate_no_second_moment():
    import cs744_distributed_data_parallel_amd as cdp

    fx = _synthetic()
    for make in (lambda ps: cdp.SGD(ps, lr=0.1, momentum=0.9), lambda ps: cdp.LARS(ps, 0.1, momentum=0.9)):
        params = [torch.nn.Parameter(p.detach().clone()) for p in fx["params"]]
        opt = make(params)
        _feed(fx, opt, 0)
        opt.step()
        assert opt._arena.second is None and opt._arena.momentum is not None
    params, opt = _flat_optimizer("AdamW")
    _feed(fx, opt, 0)
    opt.step()
    a = opt._arena
    assert a.second is not None and a.second.numel() == a.total and not a.second[fx["mask"]].any()
    assert opt.state[params[7]]["exp_avg_sq"].data_ptr() == a.second.data_ptr() + 4 * a.offsets[7]
    assert opt.state[params[7]]["exp_avg"].data_ptr() == a.momentum.data_ptr() + 4 * a.offsets[7]
    # loaded moments are copied into the arena's storages, and t comes from the loaded step
    import copy

    sd = copy.deepcopy(opt.state_dict())
    params2, opt2 = _flat_optimizer("AdamW")
    opt2.load_state_dict(sd)
    b = opt2._arena
    assert int(opt2.adam_step) == 1
    assert torch.equal(b.momentum, a.momentum) and torch.equal(b.second, a.second)
    assert opt2.state[params2[7]]["exp_avg_sq"].data_ptr() == b.second.data_ptr() + 4 * b.offsets[7]
    with torch.no_grad():
        for p, q in zip(params, params2):
            q.copy_(p)
    for o in (opt, opt2):
        _feed(fx, o, 1)
        o.step()
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(params, params2))
    assert int(opt2.adam_step) == 2


DDP_SCRIPT = textwrap.dedent(
    r"""
    import torch
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd import distributed as dist
    dist.init_process_group("rccl", rank=0, world_size=1)
    assert dist.native_communicator() is not None
    crit = cdp.CrossEntropyLoss()
    g = torch.Generator(device="cuda").manual_seed(1)
    xs = [torch.randn(8, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
          for _ in range(4)]
    ys = [torch.randint(0, 10, (8,), device="cuda", generator=g) for _ in range(4)]
    xb = torch.empty_like(xs[0]); yb = torch.empty_like(ys[0])

    def make(kind):
        torch.manual_seed(0)
        model = cdp.VGG11().cuda()
        if kind != "plain":
            model = cdp.DistributedDataParallel(model)
        opt = cdp.LAMB(model.parameters(), 1e-3, weight_decay=0.01)
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
        ms = [opt.state[p][k].detach().clone() for p in model.parameters() for k in ("exp_avg", "exp_avg_sq")]
        return ps + ms + [opt.trust_ratios.clone(), opt.adam_step.clone()]

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
    assert int(runs["plain"][1].adam_step) == 9
    q = runs["plain"][1].trust_ratios
    assert (q != 1).sum().item() >= 9
    dist.destroy_process_group()
    print("LAMB_DDP_OK")
    """
)


def test_one_rank_ddp_with_lamb_is_bitwise_the_plain_model():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", DDP_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert "LAMB_DDP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
