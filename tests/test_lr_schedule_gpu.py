"""The learning-rate schedule inside the fused SGD / LARS step on the GPU (the SCHED instantiations of
sgd_kernel / sgd_prep_kernel and lr_sched_table_kernel in csrc/kernels/misc.hip, csrc/kernels/lr_sched.h,
``SGD(lr_schedule=...)``).

The rate of step t is ``float32(double(base) * f(t))`` with ``base`` the fp32 rate the kernel would use
otherwise and ``f`` evaluated in fp64.

Bound of the table against numpy's fp64 formula (derived, not measured): both sides evaluate the same
formula in fp64, where their results differ by a few fp64 ulps at most (cos / pow of two libraries, a
contracted multiply-add); rounded to fp32 such a pair is either equal or, when it straddles a rounding
boundary, one fp32 ulp = at most 2^-23 relative apart. The bound is twice that: ``|a - b| <= 2^-22 |b|``.
The points where f is exact (t = 0, the constant phase, every t >= total_steps) are bitwise.

Everything that compares two device paths is bitwise.
"""
import copy
import math
import os
import re
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, MOM = 0.1, 0.9
BASE32 = float(np.float32(LR))  # the base rate as the kernels get it
PATHS = ["flat", "prep", "lars_flat", "lars_prep", "per_param", "flat_clip", "prep_clip"]
MAX_NORM = 0.5
W, T, MILESTONES = 3, 17, (5, 11)
KINDS = {
    "constant": dict(kind="constant", warmup_steps=W, warmup_start_factor=0.25),
    "cosine": dict(kind="cosine", total_steps=T, warmup_steps=W, warmup_start_factor=0.1, end_factor=0.01),
    "poly": dict(kind="poly", total_steps=T, warmup_steps=W, warmup_start_factor=0.1, end_factor=0.01, power=2.0),
    "step": dict(kind="step", warmup_steps=W, warmup_start_factor=0.5, milestones=MILESTONES, gamma=0.1),
}


def _cdp():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp


def _sched(name="cosine", **kw):
    return _cdp().LRSchedule(**dict(KINDS[name], **kw))


def _cfg(sched):
    """The schedule's device configuration, as the optimizer fills it."""
    return _cdp()._native.lib().lr_sched_pack(*sched._pack_args()).cuda()


def _f64_factor(c, t):
    """numpy fp64, written from the formulas (not LRSchedule.factor)."""
    Wc, s = c.get("warmup_steps", 0), c.get("warmup_start_factor", 0.0)
    t = np.float64(t)
    if t < Wc:
        return np.float64(s) + (np.float64(1.0) - np.float64(s)) * t / np.float64(Wc)
    if c["kind"] == "constant":
        return np.float64(1.0)
    if c["kind"] in ("cosine", "poly"):
        r, Tc = np.float64(c.get("end_factor", 0.0)), c["total_steps"]
        if t >= Tc:
            return r
        u = (t - Wc) / np.float64(Tc - Wc)
        if c["kind"] == "cosine":
            return r + (1.0 - r) * 0.5 * (1.0 + np.cos(np.pi * u))
        return r + (1.0 - r) * np.power(1.0 - u, np.float64(c.get("power", 2.0)))
    f = np.float64(1.0)
    for m in c["milestones"]:
        if m <= t:
            f = f * np.float64(c["gamma"])
    return f


# ----------------------------------------------------------------------------- the table
@pytest.mark.parametrize("name", list(KINDS))
def test_table_against_fp64(name):
    C = _cdp()._native.lib()
    c = KINDS[name]
    n = 23
    tab = C.lr_sched_table(_cfg(_sched(name)), None, LR, 0, n)
    assert tab.dtype == torch.float32 and tab.shape == (n,) and tab.is_cuda
    a = tab.double().cpu().numpy()
    b = np.array([np.float64(np.float32(np.float64(BASE32) * _f64_factor(c, t))) for t in range(n)])
    err, bound = np.abs(a - b), 2.0 ** -22 * np.abs(b)
    print(f"{name}: worst |a - b| / bound {float(np.max(err / bound)):.3f} at t = {int(np.argmax(err / bound))}")
    assert np.all(err <= bound), (name, a, b)
    f32 = lambda x: float(np.float32(x))
    assert a[0] == f32(BASE32 * c["warmup_start_factor"])  # bitwise: t = 0
    if name == "constant":
        assert all(a[t] == BASE32 for t in range(W, n))  # bitwise: the constant phase is the base rate itself
    if name in ("cosine", "poly"):
        assert all(a[t] == f32(BASE32 * c["end_factor"]) for t in range(T, n))  # bitwise: the end branch
        assert a[W] == BASE32 and len(set(a[:T + 1])) == T + 1
    if name == "step":
        assert a[4] == BASE32 and a[5] == f32(BASE32 * 0.1) and a[10] == a[5] and a[11] == f32(BASE32 * (0.1 * 0.1))
    # a window of the table is the table, and the base rate can come from the device
    assert torch.equal(C.lr_sched_table(_cfg(_sched(name)), None, LR, 7, 9), tab[7:16])
    lr_t = torch.tensor([0.3], dtype=torch.float32, device="cuda")
    tab3 = C.lr_sched_table(_cfg(_sched(name)), lr_t, LR, 0, n).double().cpu().numpy()
    b3 = np.array([np.float64(np.float32(np.float64(np.float32(0.3)) * _f64_factor(c, t))) for t in range(n)])
    assert np.all(np.abs(tab3 - b3) <= 2.0 ** -22 * np.abs(b3))
    assert C.lr_sched_table(_cfg(_sched(name)), None, LR, 0, 0).numel() == 0


# ----------------------------------------------------------------------------- synthetic arena
# conv [40, 36, 3, 3]: Co and Ci tails of the 32 x 32 tile, three full tap groups; [33, 8, 1, 1]: one tap, a
# partial group; [8, 4, 7, 7]: 49 taps, 49 mod 3 = 1; [16, 3, 3, 3]: the Ci % 4 != 0 scalar tile path; a
# [10, 520] linear: more than one 4096-float rest chunk; a bias of 7 and a BN weight of 33: padding and
# the n & 3 tail of the per-parameter launches
SHAPES = [(40, 36, 3, 3), (7,), (33, 8, 1, 1), (33,), (8, 4, 7, 7), (10, 520), (16, 3, 3, 3)]
NSTEP = 6


def _synthetic(seed=21):
    from cs744_distributed_data_parallel_amd.utils.arena import FlatArena

    gen = torch.Generator().manual_seed(seed)
    params = []
    for s in SHAPES:
        w = (torch.randn(s, generator=gen) * 0.05).cuda()
        if len(s) == 4:
            w = w.contiguous(memory_format=torch.channels_last)
        params.append(torch.nn.Parameter(w))
    arena = FlatArena(params)
    for p, off in zip(params, arena.offsets):
        p._fx_off = off
    convs = [p for p in params if p.dim() == 4]
    arena.prep_request = (convs, [True] * len(convs))
    return arena, convs


def _flat_random(arena, seed, scale):
    gen = torch.Generator().manual_seed(seed)
    t = torch.zeros(arena.total)
    for off, n in zip(arena.offsets, arena.numels):
        t[off:off + n] = torch.randn(n, generator=gen) * scale
    return t.cuda()


_FIX = {}


def _fx():
    """The layout, plans and inputs shared (and left unchanged) by the low-level tests."""
    if not _FIX:
        cdp = _cdp()
        C = cdp._native.lib()
        arena, convs = _synthetic()
        prep = arena.prep_plan_for(0, arena.total, cut=True)
        assert prep is not None and prep["cut"] and all(t is not None for t in prep["wts"])
        nseg, nblk, nchunk = (int(v) for v in prep["meta"])
        assert nseg == 4 and nchunk >= 4
        n = len(arena.params)

        def lars_plan(pp):
            r = C.lars_plan(arena.data, 0, arena.total, list(arena.offsets), list(arena.numels),
                            [p.dim() for p in arena.params], list(range(n)), pp["desc"] if pp else None,
                            pp["meta"] if pp else None)
            return {"desc": r[0], "meta": r[1], "part": r[2]}

        sched = _sched("cosine")
        cfg = _cfg(sched)
        _FIX.update(cdp=cdp, C=C, arena=arena, prep=prep, p0=arena.data.clone(),
                    gs=[_flat_random(arena, 300 + k, 0.01) for k in range(NSTEP)], e0=_flat_random(arena, 77, 0.05),
                    buf1=_flat_random(arena, 78, 0.01), lars_plain=lars_plan(None), lars_prep=lars_plan(prep),
                    sched=sched, cfg=cfg, table=C.lr_sched_table(cfg, None, LR, 0, 64))
        tab = _FIX["table"][:NSTEP].tolist()
        assert len(set(tab)) == NSTEP  # the warm-up runs into the cosine: every step has a rate of its own
    return _FIX


def _coef(d=0.9):
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).item()
    return torch.tensor([f32(d), f32(1.0 - d)], dtype=torch.float32, device="cuda")


class _Sched:
    """The device words of a schedule block: state {t, arrivals}, the configuration, the last rate."""

    def __init__(self, cfg, t=0):
        self.state = torch.tensor([t, 0], dtype=torch.int64, device="cuda")
        self.cfg = cfg
        self.last = torch.full((1,), float("nan"), dtype=torch.float32, device="cuda")

    def kw(self, advance=True):
        return dict(sched_state=self.state, sched_cfg=self.cfg, sched_last=self.last, sched_advance=advance)


def _launch(fx, path, p, g, buf, e, *, first, lr_t=None, sched=None, skip_nonfinite=False, wd=1e-4):
    """One step through one entry point, in place on p / buf / e (e None: EMA off). The rate comes from
    the schedule block (sched) or from lr_t: {ratios, stats, prods}."""
    C, arena, prep = fx["C"], fx["arena"], fx["prep"]
    lars, clip = path.startswith("lars"), "clip" in path
    prepped = path in ("prep", "lars_prep", "prep_clip")
    kw = {}
    stats = torch.zeros(3, device="cuda")
    ratios = torch.full((len(arena.params),), float("nan"), device="cuda")
    if clip or skip_nonfinite:
        part = torch.empty(C.grad_norm_parts(arena.total), dtype=torch.float64, device="cuda")
        C.grad_sumsq(g, part)
        kw.update(clip_part=part, max_norm=MAX_NORM if clip else float("inf"), stats=stats, skip_nonfinite=skip_nonfinite)
    if lars:
        lp = fx["lars_prep"] if prepped else fx["lars_plain"]
        lp["part"].fill_(float("nan"))
        C.lars_norms(p, g, lp["desc"], lp["meta"], lp["part"])
        kw["lars"] = C.LarsStep(desc=lp["desc"], meta=lp["meta"], part=lp["part"], ratios=ratios, trust_coefficient=0.02,
                                eps=1e-8, exclude=True)
    prods = []
    if path == "per_param":
        # one launch per parameter: every launch reads t, the last one of the step advances it
        last = len(arena.offsets) - 1
        for k, (off, n) in enumerate(zip(arena.offsets, arena.numels)):
            sl = slice(off, off + n)
            ek = dict(ema=e[sl], ema_coef=_coef()) if e is not None else {}
            if sched is not None:
                ek.update(sched.kw(advance=k == last))
            C.sgd_step(p[sl], g[sl], buf[sl], lr_t, LR, MOM, 0.0, wd, 1.0, False, first, False, **ek)
    else:
        if e is not None:
            kw.update(ema=e, ema_coef=_coef())
        if sched is not None:
            kw.update(sched.kw())
        if prepped:
            amax = torch.full_like(prep["amax"], float("nan"))
            for t in prep["wts"]:
                t.fill_(float("nan"))
            C.sgd_step_prep(p, g, buf, lr_t, LR, MOM, 0.0, wd, 1.0, False, first, False, prep["desc"], prep["meta"], amax,
                            None, **kw)
            prods = [amax] + [t.clone() for t in prep["wts"]]
        else:
            C.sgd_step(p, g, buf, lr_t, LR, MOM, 0.0, wd, 1.0, False, first, False, None, **kw)
    return dict(ratios=ratios, stats=stats, prods=prods)


def _run(fx, path, ema, scheduled):
    """NSTEP steps through one entry point, the rate from the schedule block or fed by hand through a
    device rate filled from the table before each step."""
    p, buf = fx["p0"].clone(), torch.zeros_like(fx["p0"])
    e = fx["e0"].clone() if ema else None
    sched = _Sched(fx["cfg"]) if scheduled else None
    lr_t = None if scheduled else torch.zeros(1, dtype=torch.float32, device="cuda")
    recs = []
    for step in range(NSTEP):
        if lr_t is not None:
            lr_t.copy_(fx["table"][step:step + 1])
        r = _launch(fx, path, p, fx["gs"][step], buf, e, first=step == 0, lr_t=lr_t, sched=sched)
        r.update(w=p.clone(), buf=buf.clone(), e=e.clone() if ema else None,
                 state=sched.state.clone() if scheduled else None, last=sched.last.clone() if scheduled else None)
        recs.append(r)
    torch.cuda.synchronize()
    return recs


@pytest.mark.parametrize("ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("path", PATHS)
def test_every_path_steps_at_the_rates_of_the_table(path, ema):
    fx = _fx()
    on, off = _run(fx, path, ema, True), _run(fx, path, ema, False)
    prev = fx["p0"]
    for step, (a, b) in enumerate(zip(on, off)):
        what = (path, ema, step)
        assert torch.equal(a["w"], b["w"]), what
        assert torch.equal(a["buf"], b["buf"]), what
        if ema:
            assert torch.equal(a["e"], b["e"]), what
        assert torch.equal(a["ratios"].view(torch.int32), b["ratios"].view(torch.int32)), what  # NaN where unused
        assert torch.equal(a["stats"], b["stats"]), what
        assert len(a["prods"]) == len(b["prods"]) == (5 if "prep" in path else 0)
        for u, v in zip(a["prods"], b["prods"]):
            assert not torch.isnan(u).any() and torch.equal(u, v), what
        assert a["state"].tolist() == [step + 1, 0], what  # t advanced by one, the arrival word is back at 0
        assert torch.equal(a["last"], fx["table"][step:step + 1]), what
        assert not torch.equal(a["w"], prev)
        prev = a["w"]
    assert on[-1]["state"].tolist() == [NSTEP, 0] and on[-1]["last"].item() == fx["table"][NSTEP - 1].item()


def test_a_launch_that_does_not_advance_only_reads_t():
    fx = _fx()
    C = fx["C"]
    s = _Sched(fx["cfg"], t=4)
    p, q = fx["p0"].clone(), fx["p0"].clone()
    C.sgd_step(p, fx["gs"][0], None, None, LR, 0.0, 0.0, 0.0, 1.0, False, True, False, None, **s.kw(advance=False))
    assert s.state.tolist() == [4, 0] and torch.equal(s.last, fx["table"][4:5])  # the rate is recorded all the same
    s.last.fill_(float("nan"))
    C.sgd_step(q, fx["gs"][0], None, fx["table"][4:5].clone(), LR, 0.0, 0.0, 0.0, 1.0, False, True, False, None)
    assert torch.equal(p, q) and not torch.equal(p, fx["p0"])
    C.lr_sched_advance(s.state, s.cfg, s.last, None, LR)  # the step() that launches nothing
    assert s.state.tolist() == [5, 0] and torch.equal(s.last, fx["table"][4:5])


def test_the_bindings_refuse_half_a_schedule_block():
    fx = _fx()
    C = fx["C"]
    p = fx["p0"].clone()
    s = _Sched(fx["cfg"])
    for kw in (dict(sched_state=s.state), dict(sched_cfg=s.cfg), dict(sched_last=s.last), dict(sched_advance=True),
               dict(sched_state=s.state.int(), sched_cfg=s.cfg), dict(sched_state=s.state[:1], sched_cfg=s.cfg),
               dict(sched_state=s.state, sched_cfg=s.cfg[:64]), dict(sched_state=s.state, sched_cfg=s.cfg.cpu()),
               dict(sched_state=s.state, sched_cfg=s.cfg, sched_last=s.last.double())):
        with pytest.raises(RuntimeError, match="sched"):
            C.sgd_step(p, fx["gs"][0], None, None, LR, 0.0, 0.0, 0.0, 1.0, False, True, False, None, **kw)
    assert torch.equal(p, fx["p0"]) and s.state.tolist() == [0, 0]


# ----------------------------------------------------------------------------- the advance under many workgroups
def test_the_advance_under_many_workgroups():
    """One flat launch of more than 1024 workgroups, 50 steps at 50 different rates: a workgroup that saw
    t + 1 would step at the next rate and break the equality with the run fed by hand."""
    fx = _fx()
    C = fx["C"]
    n = 1_050_003  # also the n & 3 tail
    assert C.sgd_grid(n) >= 1024
    gen = torch.Generator().manual_seed(5)
    p0 = (torch.randn(n, generator=gen) * 0.05).cuda()
    g = (torch.randn(n, generator=gen) * 0.01).cuda()
    sched = _cdp().LRSchedule("cosine", total_steps=60, warmup_steps=5, warmup_start_factor=0.1)
    cfg = _cfg(sched)
    table = C.lr_sched_table(cfg, None, LR, 0, 50)
    assert len(set(table.tolist())) == 50
    s = _Sched(cfg)
    pa, ba = p0.clone(), torch.zeros_like(p0)
    pb, bb = p0.clone(), torch.zeros_like(p0)
    lr_t = torch.zeros(1, dtype=torch.float32, device="cuda")
    for step in range(50):
        C.sgd_step(pa, g, ba, None, LR, MOM, 0.0, 1e-4, 1.0, False, step == 0, False, None, **s.kw())
        lr_t.copy_(table[step:step + 1])
        C.sgd_step(pb, g, bb, lr_t, LR, MOM, 0.0, 1e-4, 1.0, False, step == 0, False, None)
    torch.cuda.synchronize()
    assert s.state.tolist() == [50, 0]
    assert torch.equal(s.last, table[49:50])
    assert torch.equal(pa, pb) and torch.equal(ba, bb) and not torch.equal(pa, p0)


# ----------------------------------------------------------------------------- the optimizer on the synthetic arena
def _view(flat, arena, p):
    return torch.as_strided(flat, p.size(), p.stride(), p._fx_off)


def _opt(kind="sgd", prep=True, sched="cosine", **kw):
    cdp = _cdp()
    fx = _fx()
    arena, _ = _synthetic()
    if not prep:
        arena.prep_request = None
    assert torch.equal(arena.data, fx["p0"]) and arena.offsets == fx["arena"].offsets
    hp = dict(momentum=MOM, weight_decay=1e-4)
    if sched is not None:
        hp["lr_schedule"] = _sched(sched)
    hp.update(kw)
    if kind == "lars":
        opt = cdp.LARS(arena.params, LR, trust_coefficient=0.02, **hp)
    else:
        opt = cdp.SGD(arena.params, lr=LR, **hp)
    return arena, opt


def _set_grads(arena, g):
    for p in arena.params:
        if p.grad is None:
            p.grad = torch.zeros_like(p)
        p.grad.copy_(_view(g, arena, p))


def _opt_state(arena, opt):
    return [p.detach().clone() for p in arena.params] + [opt.state[p]["momentum_buffer"].clone() for p in arena.params]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


@pytest.mark.parametrize("form", ["prep", "flat", "lars", "per_param"])
def test_optimizer_step_is_the_entry_points(form):
    fx = _fx()
    kind = "lars" if form == "lars" else "sgd"
    arena, opt = _opt(kind, prep=form != "flat", **(dict(flat=False) if form == "per_param" else {}))
    recs = _run(fx, {"prep": "prep", "flat": "flat", "lars": "lars_prep", "per_param": "per_param"}[form], False, True)
    assert opt.schedule_step.dim() == 0 and opt.schedule_step.dtype == torch.int64 and opt.schedule_step.is_cuda
    assert opt.last_lr.dim() == 0 and opt.last_lr.dtype == torch.float32 and opt.last_lr.is_cuda
    assert torch.equal(opt.lr_schedule_table(0, 64), fx["table"])
    for step in range(NSTEP):
        _set_grads(arena, fx["gs"][step])
        opt.step()  # (per_param: seven launches, and t advances by exactly one)
        assert opt.schedule_step.item() == step + 1 and opt._sched_state[1].item() == 0, (form, step)
        assert opt.last_lr.item() == fx["table"][step].item(), (form, step)
        assert torch.equal(arena.data, recs[step]["w"]), (form, step)
    assert opt.param_groups[0]["lr"] == LR


def test_the_schedule_composes_with_lr_tensor_and_a_step_without_gradients_counts():
    fx = _fx()
    arena, opt = _opt()
    twin_arena, twin = _opt(sched=None)
    opt.lr_tensor().fill_(0.3)
    table = opt.lr_schedule_table(0, 8)
    assert table[W].item() == float(np.float32(0.3))  # the top of the warm-up is the base rate itself
    for step in range(3):
        twin.lr_tensor().copy_(table[step:step + 1])
        for a, o in ((arena, opt), (twin_arena, twin)):
            _set_grads(a, fx["gs"][step])
            o.step()
        assert torch.equal(arena.data, twin_arena.data) and opt.last_lr.item() == table[step].item()
    opt.zero_grad()
    w = arena.data.clone()
    opt.step()  # nothing to launch: the schedule counts the iteration all the same
    assert opt.schedule_step.item() == 4 and opt.last_lr.item() == table[3].item() and torch.equal(arena.data, w)


def test_several_param_groups_advance_t_once():
    cdp = _cdp()
    fx = _fx()
    arena, _ = _synthetic()
    ps = list(arena.params)
    opt = cdp.SGD([dict(params=ps[:3]), dict(params=ps[3:], lr=0.2)], lr=LR, momentum=MOM, lr_schedule=_sched("cosine"))
    for step in range(3):
        _set_grads(arena, fx["gs"][step])
        w = arena.data.clone()
        opt.step()
        assert opt._sched_state.tolist() == [step + 1, 0] and opt.last_lr.item() == fx["table"][step].item()
        assert not torch.equal(arena.data, w)


@pytest.mark.parametrize("kind", ["sgd", "lars"])
def test_a_skipped_step_advances_t_and_changes_nothing_else(kind):
    fx = _fx()
    arena, opt = _opt(kind, skip_nonfinite=True, ema_decay=0.9)
    for step in range(2):
        _set_grads(arena, fx["gs"][step])
        opt.step()
    assert opt.skipped_steps.item() == 0 and opt.schedule_step.item() == 2
    w, m, e = arena.data.clone(), arena.momentum.clone(), arena.ema.clone()
    _set_grads(arena, fx["gs"][2])
    arena.params[0].grad[3, 4, 1, 1] = float("inf")
    opt.step()
    assert opt.skipped_steps.item() == 1
    assert torch.equal(arena.data, w) and torch.equal(arena.momentum, m) and torch.equal(arena.ema, e)
    assert opt._sched_state.tolist() == [3, 0] and opt.last_lr.item() == fx["table"][2].item()
    _set_grads(arena, fx["gs"][2])
    opt.step()
    assert opt.skipped_steps.item() == 1 and not torch.equal(arena.data, w)
    assert opt._sched_state.tolist() == [4, 0] and opt.last_lr.item() == fx["table"][3].item()


def test_captured_step_follows_the_schedule_at_every_replay_and_the_setters():
    """Twin A steps eagerly, twin B replays one captured step: bitwise equal after every step."""
    fx = _fx()
    C = fx["C"]
    (aa, oa), (ab, ob) = _opt(), _opt()
    gs = [_flat_random(aa, 500 + k, 0.01) for k in range(14)]
    for step in range(2):  # the first momentum step and one more, eagerly in both
        for a, o in ((aa, oa), (ab, ob)):
            _set_grads(a, gs[step])
            o.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ob.step()
    torch.cuda.synchronize()
    assert ob.schedule_step.item() == 2  # the capture ran nothing

    def both(step):
        _set_grads(aa, gs[step])
        oa.step()
        _set_grads(ab, gs[step])
        graph.replay()
        torch.cuda.synchronize()
        assert _same(_opt_state(aa, oa), _opt_state(ab, ob)), step
        assert torch.equal(oa._sched_state, ob._sched_state) and ob._sched_state[1].item() == 0
        assert oa.last_lr.item() == ob.last_lr.item()

    seen = []
    for step in range(2, 12):  # ten replays, ten rates
        both(step)
        assert ob.schedule_step.item() == step + 1 and ob.last_lr.item() == fx["table"][step].item()
        seen.append(ob.last_lr.item())
    assert len(set(seen)) == 10
    for o in (oa, ob):
        o.set_schedule_step(3)  # no re-capture
    both(12)
    assert ob.schedule_step.item() == 4 and ob.last_lr.item() == fx["table"][3].item()
    poly = _sched("poly")
    for o in (oa, ob):
        o.set_lr_schedule(poly)
    both(13)
    assert ob.schedule_step.item() == 5
    assert ob.last_lr.item() == C.lr_sched_table(_cfg(poly), None, LR, 4, 1).item() != fx["table"][4].item()
    # the setters (and the host read of state_dict) are refused while a stream is capturing
    scratch = torch.zeros(8, device="cuda")
    for call in (lambda: ob.set_schedule_step(1), lambda: ob.set_lr_schedule(poly), lambda: ob.state_dict()):
        g2 = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="capturing"):
            with torch.cuda.graph(g2):
                scratch.add_(1.0)
                call()
        torch.cuda.synchronize()
    assert ob.schedule_step.item() == 5


def test_checkpoint_save_load_and_continue_is_the_uninterrupted_run(tmp_path):
    fx = _fx()
    (a1, o1), (a2, o2) = _opt(), _opt()
    for step in range(3):
        _set_grads(a1, fx["gs"][step])
        o1.step()
    path = str(tmp_path / "opt.pt")
    torch.save({"w": a1.data.clone(), "optimizer": o1.state_dict()}, path)
    st = torch.load(path, weights_only=True)
    assert st["optimizer"]["param_groups"][0]["lr_schedule_step"] == 3
    a2.data.copy_(st["w"])
    o2.load_state_dict(st["optimizer"])
    assert o2._sched_state.tolist() == [3, 0] and "lr_schedule_step" not in o2.param_groups[0]
    for step in range(3, NSTEP):
        for a, o in ((a1, o1), (a2, o2)):
            _set_grads(a, fx["gs"][step])
            o.step()
        assert _same(_opt_state(a1, o1), _opt_state(a2, o2)), step
        assert o2.last_lr.item() == fx["table"][step].item() and o2.schedule_step.item() == step + 1
    sd = copy.deepcopy(o1.state_dict())
    for g in sd["param_groups"]:
        del g["lr_schedule_step"]
    o2.set_schedule_step(11)
    o2.load_state_dict(sd)  # no step in the state: t stays
    assert o2.schedule_step.item() == 11


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
          for _ in range(3)]
    ys = [torch.randint(0, 10, (16,), device="cuda", generator=g) for _ in range(3)]

    def make(kind):
        torch.manual_seed(0)
        model = cdp.VGG11().cuda()
        if kind != "plain":
            model = cdp.DistributedDataParallel(model)
        sched = cdp.LRSchedule("cosine", total_steps=17, warmup_steps=2, warmup_start_factor=0.1)
        opt = cdp.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, lr_schedule=sched)
        if kind == "overlap":
            model.overlap_optimizer(opt)
        return model, opt

    runs = {k: make(k) for k in ("plain", "overlap")}

    def state(model, opt):
        ps = list(model.parameters())
        return [p.detach().clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps]

    table = runs["plain"][1].lr_schedule_table(0, 3)
    assert len(set(table.tolist())) == 3
    for step in range(3):
        for m, o in runs.values():
            o.zero_grad()
            crit(m(xs[step]), ys[step]).backward()
            o.step()
        ref = state(*runs["plain"])
        for u, v in zip(ref, state(*runs["overlap"])):
            assert torch.equal(u, v), step
        # bucket_steps declined: the step ran whole at step()
        assert runs["overlap"][0].reducer.stepped_buckets() == 0
        assert runs["overlap"][1]._overlap is None
        for m, o in runs.values():
            assert o._sched_state.tolist() == [step + 1, 0] and o.last_lr.item() == table[step].item()
    dist.destroy_process_group()
    print("LRS_DDP_OK")
    """
)


def test_one_rank_ddp_with_a_schedule_is_bitwise_the_plain_model():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", DDP_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert "LRS_DDP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]


# ----------------------------------------------------------------------------- CLI
def test_train_cli_with_a_schedule_on_the_gpu():
    """(320 synthetic images: 20 batches of 16, so that the epoch reaches iteration 20 and its log lines.)"""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "cs744_distributed_data_parallel_amd.train", "--model", "vgg11",
                        "--synthetic-size", "320", "--batch-size", "16", "--iters", "20", "--lr-schedule", "cosine",
                        "--warmup-iters", "5"], env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    losses = re.findall(r"Training loss after 20 epochs is (?:tensor\()?([-0-9.eE+naif]+)", r.stdout)
    assert len(losses) == 1 and math.isfinite(float(losses[0])), r.stdout
    assert "[cdp]" not in r.stdout
    got = re.findall(r"^\[cdp\] rank 0: lr in iter 20 is ([-0-9.eE+]+) \(schedule step 20\)$", r.stderr, flags=re.M)
    assert len(got) == 1, r.stderr[-3000:]
    want = np.float32(_cdp().LRSchedule("cosine", total_steps=20, warmup_steps=5).rate(0.1, 19))  # the rate of step 19
    assert abs(np.float64(np.float32(float(got[0]))) - np.float64(want)) <= 2.0 ** -22 * np.float64(want), (got, want)
