"""Weight EMA inside the fused SGD / LARS step on the GPU (the EMA block of sgd_kernel / sgd_prep_kernel in
csrc/kernels/misc.hip, ``SGD(ema_decay=...)``, ``FlatArena.ema``).

Per element the kernels compute ``e = fmaf(w_new, omd, e * d)`` with ``d = float32(decay)`` and
``omd = float32(1.0 - decay)``.

Bound against fp64 (derived, not measured). With ``M = max(|e_before|, |w_after|)``: the product
``e * d`` is rounded once (at most 2^-24 |e d| <= 2^-24 M), the fma rounds once more (at most 2^-24 of
a result whose magnitude is at most (d + omd) M (1 + 2^-24), and d + omd <= 1 + 2^-24), and the
reference uses the same fp32 coefficients, so they add nothing. Allowing a third rounding for
implementations that round ``w * omd`` separately, every element must satisfy
``|e_after - (double(d) * e_before + double(omd) * w_after)| <= 3 * 2^-24 M <= 2^-22 M``.

Everything that compares two device paths is bitwise.
"""
import copy
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR, MOM = 0.1, 0.9
PATHS = ["flat", "prep", "lars_flat", "lars_prep", "per_param", "flat_clip", "prep_clip"]
VARIANTS = ["plain", "nesterov", "wd0"]
MAX_NORM = 0.5


def _f32(x):
    return torch.tensor(x, dtype=torch.float32).item()


def _coef(d):
    return torch.tensor([_f32(d), _f32(1.0 - d)], dtype=torch.float32, device="cuda")


# ----------------------------------------------------------------------------- synthetic arena
# conv [40, 36, 3, 3]: Co and Ci tails of the 32 x 32 tile, three full tap groups; [33, 8, 1, 1]: one tap, a
# partial group; [8, 4, 7, 7]: 49 taps, 49 mod 3 = 1; [16, 3, 3, 3]: the Ci % 4 != 0 scalar tile path; a
# [10, 520] linear: more than one 4096-float rest chunk; a bias of 7 and a BN weight of 33: padding and
# the n & 3 tail of the per-parameter launches
SHAPES = [(40, 36, 3, 3), (7,), (33, 8, 1, 1), (33,), (8, 4, 7, 7), (10, 520), (16, 3, 3, 3)]


def _synthetic(seed=21):
    """(arena, conv weights): a fresh arena over the shapes above with a registered weight-preparation
    request for the conv weights (W^T wanted for all of them)."""
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
        p._fx_off = off  # its place in the flat tensors of _fx(), whatever a relayout does to the arena
    convs = [p for p in params if p.dim() == 4]
    arena.prep_request = (convs, [True] * len(convs))
    return arena, convs


def _flat_random(arena, seed, scale):
    """Seeded Gaussian values over the arena's floats, zero in the pads."""
    gen = torch.Generator().manual_seed(seed)
    t = torch.zeros(arena.total)
    for off, n in zip(arena.offsets, arena.numels):
        t[off:off + n] = torch.randn(n, generator=gen) * scale
    return t.cuda()


def _pad_mask(arena):
    m = torch.ones(arena.total, dtype=torch.bool)
    for off, n in zip(arena.offsets, arena.numels):
        m[off:off + n] = False
    return m.cuda()


_FIX = {}


def _fx():
    """The layout, plans and inputs shared (and left unchanged) by the low-level tests: weights p0,
    three gradients, an EMA e0 seeded differently from the weights."""
    if not _FIX:
        import cs744_distributed_data_parallel_amd as cdp

        C = cdp._native.lib()
        arena, convs = _synthetic()
        prep = arena.prep_plan_for(0, arena.total, cut=True)
        assert prep is not None and prep["cut"] and all(t is not None for t in prep["wts"])
        nseg, nblk, nchunk = (int(v) for v in prep["meta"])
        assert nseg == 4 and nchunk >= 4  # the linear alone is two rest chunks
        n = len(arena.params)

        def lars_plan(pp):
            r = C.lars_plan(arena.data, 0, arena.total, list(arena.offsets), list(arena.numels),
                            [p.dim() for p in arena.params], list(range(n)), pp["desc"] if pp else None,
                            pp["meta"] if pp else None)
            return {"desc": r[0], "meta": r[1], "part": r[2]}

        mask = _pad_mask(arena)
        assert int(mask.sum()) == 4  # 7 -> 8 and 33 -> 36
        _FIX.update(cdp=cdp, C=C, arena=arena, prep=prep, mask=mask, p0=arena.data.clone(),
                    gs=[_flat_random(arena, 300 + k, 0.01) for k in range(3)], e0=_flat_random(arena, 77, 0.05),
                    buf1=_flat_random(arena, 78, 0.01), lars_plain=lars_plan(None), lars_prep=lars_plan(prep))
        assert not _FIX["p0"][mask].any() and not _FIX["e0"][mask].any()
    return _FIX


def _hp(variant):
    return variant == "nesterov", (0.0 if variant == "wd0" else 1e-4)


def _launch(fx, path, p, g, buf, e, coef, *, first, nest, wd, skip_nonfinite=False, mom=MOM):
    """One step through one entry point, in place on p / buf / e (e None: EMA off):
    {ratios, stats, prods}."""
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
        # one launch per parameter over exactly its numel floats (the n & 3 tail), its own slice of e
        for off, n in zip(arena.offsets, arena.numels):
            sl = slice(off, off + n)
            ek = dict(ema=e[sl], ema_coef=coef) if e is not None else {}
            C.sgd_step(p[sl], g[sl], buf[sl], None, LR, mom, 0.0, wd, 1.0, nest, first, False, **ek)
    else:
        if e is not None:
            kw.update(ema=e, ema_coef=coef)
        if prepped:
            amax = torch.full_like(prep["amax"], float("nan"))
            for t in prep["wts"]:
                t.fill_(float("nan"))
            C.sgd_step_prep(p, g, buf, None, LR, mom, 0.0, wd, 1.0, nest, first, False, prep["desc"], prep["meta"], amax,
                            None, **kw)
            prods = [amax] + [t.clone() for t in prep["wts"]]
        else:
            C.sgd_step(p, g, buf, None, LR, mom, 0.0, wd, 1.0, nest, first, False, None, **kw)
    return dict(ratios=ratios, stats=stats, prods=prods)


_RUNS = {}


def _run(path, variant, ema, d=0.9):
    """Three steps (a first momentum step, then two later ones) through one entry point; per step
    e_before, and w / e / momentum / ratios / stats / products after. Computed once per key."""
    key = (path, variant, ema, d)
    if key not in _RUNS:
        fx = _fx()
        nest, wd = _hp(variant)
        p, buf = fx["p0"].clone(), torch.zeros_like(fx["p0"])
        e = fx["e0"].clone() if ema else None
        coef = _coef(d)
        recs = []
        for step in range(3):
            eb = e.clone() if ema else None
            r = _launch(fx, path, p, fx["gs"][step], buf, e, coef, first=step == 0, nest=nest, wd=wd)
            r.update(eb=eb, w=p.clone(), buf=buf.clone(), e=e.clone() if ema else None)
            recs.append(r)
        torch.cuda.synchronize()
        _RUNS[key] = recs
    return _RUNS[key]


def _check_fp64(eb, w, e, d, what):
    d64, omd64 = float(np.float32(d)), float(np.float32(1.0 - d))
    assert d64 == _f32(d) and omd64 == _f32(1.0 - d)
    eb, w, e = (t.double().cpu().numpy() for t in (eb, w, e))
    err = np.abs(e - (d64 * eb + omd64 * w))
    bound = 2.0 ** -22 * np.maximum(np.abs(eb), np.abs(w))
    k = int(np.argmax(err - bound))
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{what}: max err / bound {worst:.3f} at {k}")
    assert np.all(err <= bound), (what, k, err[k], bound[k])  # every element, the pads included (0 <= 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("path", PATHS)
def test_against_fp64_per_step_per_path(path, variant):
    fx = _fx()
    recs = _run(path, variant, True)
    for step, r in enumerate(recs):
        _check_fp64(r["eb"], r["w"], r["e"], 0.9, f"{path} {variant} step {step}")
        assert not r["e"][fx["mask"]].any()  # the pad floats of e stay zero
        assert not torch.equal(r["e"], r["eb"]) and not torch.equal(r["e"], r["w"])
        if "clip" in path:
            assert 0.0 < r["stats"][1].item() < 1.0  # the clip is active
        if step:
            assert torch.equal(r["eb"], recs[step - 1]["e"])
    assert not torch.equal(recs[0]["w"], fx["p0"])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("path", PATHS)
def test_weights_momentum_ratios_stats_and_products_are_those_without_the_ema(path, variant):
    on, off = _run(path, variant, True), _run(path, variant, False)
    for step, (a, b) in enumerate(zip(on, off)):
        what = (path, variant, step)
        assert torch.equal(a["w"], b["w"]), what
        assert torch.equal(a["buf"], b["buf"]), what
        assert torch.equal(a["ratios"].view(torch.int32), b["ratios"].view(torch.int32)), what  # NaN where unused
        assert torch.equal(a["stats"], b["stats"]), what
        assert len(a["prods"]) == len(b["prods"]) == (5 if "prep" in path else 0)
        for u, v in zip(a["prods"], b["prods"]):
            assert not torch.isnan(u).any() and torch.equal(u, v), what
        if path.startswith("lars"):
            q = a["ratios"].cpu()
            assert all(torch.isfinite(q[k]) and (q[k] != 1.0) == (len(s) > 1) for k, s in enumerate(SHAPES)), q


def _ema_by_identity_step(C, eb, w, d):
    """e after a plain flat step that leaves w as it is (lr 0, zero gradient, no momentum, no wd)."""
    p, e = w.clone(), eb.clone()
    C.sgd_step(p, torch.zeros_like(p), None, None, 0.0, 0.0, 0.0, 0.0, 1.0, False, True, False, None, ema=e,
               ema_coef=_coef(d))
    assert torch.equal(p, w)
    return e


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_path_gives_the_same_ema_bitwise(variant):
    C = _fx()["C"]
    runs = {path: _run(path, variant, True) for path in PATHS}
    for step in range(3):
        ref = runs["flat"][step]
        for path in ("prep", "per_param"):  # the same step: the same w, so the same e
            assert torch.equal(runs[path][step]["w"], ref["w"]), (path, step)
            assert torch.equal(runs[path][step]["e"], ref["e"]), (path, step)
        assert torch.equal(runs["flat_clip"][step]["w"], runs["prep_clip"][step]["w"]), step
        assert torch.equal(runs["flat_clip"][step]["e"], runs["prep_clip"][step]["e"]), step
        assert torch.equal(runs["lars_flat"][step]["w"], runs["lars_prep"][step]["w"]), step
        assert torch.equal(runs["lars_flat"][step]["e"], runs["lars_prep"][step]["e"]), step
        assert not torch.equal(runs["lars_flat"][step]["w"], ref["w"])
        # LARS and the clip move the weights elsewhere: against a non-LARS launch fed the same resulting w
        for path in PATHS:
            r = runs[path][step]
            assert torch.equal(r["e"], _ema_by_identity_step(C, r["eb"], r["w"], 0.9)), (path, step)


@pytest.mark.parametrize("path", PATHS)
def test_decay_0_and_1_are_bitwise_edges(path):
    fx = _fx()
    for step, r in enumerate(_run(path, "plain", True, d=0.0)):
        assert torch.equal(r["e"], r["w"]), (path, step)
    for step, r in enumerate(_run(path, "plain", True, d=1.0)):
        assert torch.equal(r["e"], fx["e0"]), (path, step)
        assert not torch.equal(r["w"], fx["p0"])


@pytest.mark.parametrize("path", ["flat", "prep", "lars_flat", "lars_prep"])
def test_a_skipped_step_leaves_the_ema_weights_and_momentum_unchanged(path):
    fx = _fx()
    g = fx["gs"][1].clone()
    g[fx["arena"].offsets[4] + 5] = float("inf")
    p, buf, e = fx["p0"].clone(), fx["buf1"].clone(), fx["e0"].clone()
    r = _launch(fx, path, p, g, buf, e, _coef(0.9), first=False, nest=False, wd=1e-4, skip_nonfinite=True)
    assert r["stats"][2].item() == 1.0
    assert torch.equal(p, fx["p0"]) and torch.equal(buf, fx["buf1"]) and torch.equal(e, fx["e0"])
    # the same launch with a finite gradient does step
    r = _launch(fx, path, p, fx["gs"][1], buf, e, _coef(0.9), first=False, nest=False, wd=1e-4, skip_nonfinite=True)
    assert r["stats"][2].item() == 0.0
    assert not torch.equal(p, fx["p0"]) and not torch.equal(e, fx["e0"])
    _check_fp64(fx["e0"], p, e, 0.9, f"{path} after the skip")


def test_the_bindings_refuse_half_an_ema_block():
    fx = _fx()
    C = fx["C"]
    p, e = fx["p0"].clone(), fx["e0"].clone()
    for kw in (dict(ema=e), dict(ema_coef=_coef(0.9)), dict(ema=e[:-4], ema_coef=_coef(0.9)),
               dict(ema=p, ema_coef=_coef(0.9)), dict(ema=e.double(), ema_coef=_coef(0.9))):
        with pytest.raises(RuntimeError, match="ema"):
            C.sgd_step(p, fx["gs"][0], None, None, LR, 0.0, 0.0, 0.0, 1.0, False, True, False, None, **kw)
    assert torch.equal(p, fx["p0"]) and torch.equal(e, fx["e0"])


# ----------------------------------------------------------------------------- the optimizer on the synthetic arena
def _view(flat, arena, p):
    """p's values in a flat tensor laid out as the arena was at construction (the layout of _fx())."""
    return torch.as_strided(flat, p.size(), p.stride(), p._fx_off)


def _opt(kind="sgd", prep=True, **kw):
    import cs744_distributed_data_parallel_amd as cdp

    fx = _fx()
    arena, _ = _synthetic()
    if not prep:
        arena.prep_request = None
    assert torch.equal(arena.data, fx["p0"]) and arena.offsets == fx["arena"].offsets
    hp = dict(momentum=MOM, weight_decay=1e-4, ema_decay=0.9)
    hp.update(kw)
    if kind == "lars":
        opt = cdp.LARS(arena.params, LR, trust_coefficient=0.02, **hp)
    else:
        opt = cdp.SGD(arena.params, lr=LR, **hp)
    # e starts as a copy of the weights; from here on it is seeded differently
    es = [opt.state[p]["ema_buffer"] for p in arena.params]
    assert all(torch.equal(e, p.detach()) and e.data_ptr() != p.data_ptr() for e, p in zip(es, arena.params))
    for p, e in zip(arena.params, es):
        e.copy_(_view(fx["e0"], arena, p))
    return arena, opt


def _set_grads(arena, g):
    for p in arena.params:
        p.grad.copy_(_view(g, arena, p))


@pytest.mark.parametrize("form", ["prep", "flat", "lars", "per_param"])
def test_optimizer_step_is_the_entry_points(form):
    fx = _fx()
    kind = "lars" if form == "lars" else "sgd"
    arena, opt = _opt(kind, prep=form != "flat", **(dict(flat=False) if form == "per_param" else {}))
    recs = _run({"prep": "prep", "flat": "flat", "lars": "lars_prep", "per_param": "per_param"}[form], "plain", True)
    if form == "per_param":
        assert opt._arena is None and arena.ema is None
    else:
        assert all(opt.state[p]["ema_buffer"].data_ptr() == arena.ema.data_ptr() + 4 * arena.offsets[p._cdp_index]
                   for p in arena.params)
        assert torch.equal(arena.ema, fx["e0"])
    for step in range(3):
        _set_grads(arena, fx["gs"][step])
        opt.step()
        assert torch.equal(arena.data, recs[step]["w"]), (form, step)
        for p in arena.params:
            assert torch.equal(opt.ema_state()[p], _view(recs[step]["e"], arena, p)), (form, step)
        assert (arena.prep_valid is not None) == (form in ("prep", "lars"))
    if form != "per_param":
        assert torch.equal(arena.ema, recs[2]["e"])


@pytest.mark.parametrize("kind", ["sgd", "lars"])
def test_optimizer_skip_nonfinite_leaves_the_ema_and_counts_the_step(kind):
    fx = _fx()
    arena, opt = _opt(kind, skip_nonfinite=True)
    for step in range(2):
        _set_grads(arena, fx["gs"][step])
        opt.step()
    assert opt.skipped_steps.item() == 0
    w, m, e = arena.data.clone(), arena.momentum.clone(), arena.ema.clone()
    _set_grads(arena, fx["gs"][2])
    arena.params[0].grad[3, 4, 1, 1] = float("inf")
    opt.step()
    assert opt.skipped_steps.item() == 1
    assert torch.equal(arena.data, w) and torch.equal(arena.momentum, m) and torch.equal(arena.ema, e)
    _set_grads(arena, fx["gs"][2])
    opt.step()
    assert opt.skipped_steps.item() == 1 and not torch.equal(arena.ema, e)


def test_relayout_moves_the_ema_with_its_parameters():
    fx = _fx()
    (a1, o1), (a2, o2) = _opt(), _opt()
    for step in range(2):
        for a, o in ((a1, o1), (a2, o2)):
            _set_grads(a, fx["gs"][step])
            o.step()
    old = a2.ema
    params = list(a1.params), list(a2.params)  # in the order of construction
    a2.relayout(list(reversed(range(len(a2.params)))))
    assert a2.ema is not old and a2.ema.numel() == a2.total and not a2.ema[_pad_mask(a2)].any()
    for p in a2.params:
        e = o2.state[p]["ema_buffer"]
        assert e.data_ptr() == a2.ema.data_ptr() + 4 * a2.offsets[p._cdp_index]  # a view into the new storage
        assert e.stride() == p.stride()
    for p, q in zip(*params):
        assert torch.equal(o1.state[p]["ema_buffer"], o2.state[q]["ema_buffer"])
    for a, o in ((a1, o1), (a2, o2)):
        _set_grads(a, fx["gs"][2])
        o.step()
        assert a.prep_valid is not None
    for p, q in zip(*params):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(o1.state[p]["ema_buffer"], o2.state[q]["ema_buffer"])
        assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"])
    assert torch.equal(a1.data, _run("prep", "plain", True)[2]["w"])
    assert torch.equal(a1.ema, _run("prep", "plain", True)[2]["e"])


def test_load_state_dict_adopts_the_ema_into_the_arena():
    fx = _fx()
    (a1, o1), (a2, o2) = _opt(), _opt()
    for step in range(2):
        _set_grads(a1, fx["gs"][step])
        o1.step()
    a2.data.copy_(a1.data)
    o2.load_state_dict(copy.deepcopy(o1.state_dict()))  # tensors of its own, as from a file
    assert torch.equal(a2.ema, a1.ema) and a2.ema.data_ptr() != a1.ema.data_ptr()
    assert all(o2.state[p]["ema_buffer"].data_ptr() == a2.ema.data_ptr() + 4 * a2.offsets[p._cdp_index]
               for p in a2.params)
    for a, o in ((a1, o1), (a2, o2)):
        _set_grads(a, fx["gs"][2])
        o.step()
    assert torch.equal(a1.data, a2.data) and torch.equal(a1.ema, a2.ema)
    sd = o1.state_dict()
    sd["state"] = {k: {n: t for n, t in st.items() if n != "ema_buffer"} for k, st in sd["state"].items()}
    o2.load_state_dict(sd)  # no EMA in the state: e starts again from the current weights
    assert torch.equal(a2.ema, a2.data)
    o1.reset_ema()
    assert torch.equal(a1.ema, a1.data)


# ----------------------------------------------------------------------------- VGG-11
def _vgg(**kw):
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    hp = dict(momentum=MOM, weight_decay=1e-4, ema_decay=0.9)
    hp.update(kw)
    return cdp, model, cdp.SGD(model.parameters(), lr=LR, **hp)


def _batch(step, B=16):
    g = torch.Generator(device="cuda").manual_seed(1000 + step)
    x = torch.randn(B, 3, 32, 32, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    return x, y


def _state(model, opt):
    ps = list(model.parameters())
    return ([p.detach().clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps]
            + [opt.state[p]["ema_buffer"].clone() for p in ps])


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


class _Runs:
    """n identical VGG-11 + SGD(ema_decay=0.9) pairs stepped together on a shared static batch; the
    first one's step is captured after three eager steps and one on a side stream."""

    def __init__(self, n):
        self.xb, self.yb = (torch.empty_like(t) for t in _batch(0))
        self.runs = []
        for _ in range(n):
            self.cdp, model, opt = _vgg()
            self.runs.append((model, opt))
        self.crit = self.cdp.CrossEntropyLoss()
        for step in range(3):
            self.feed(step)
            for m, o in self.runs:
                self.body(m, o)
        self.feed(3)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for m, o in self.runs:
                self.body(m, o)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.body(*self.runs[0])
        torch.cuda.synchronize()
        self.step = 4

    def body(self, model, opt):
        opt.zero_grad()
        self.crit(model(self.xb), self.yb).backward()
        opt.step()

    def feed(self, step):
        x, y = _batch(step)
        self.xb.copy_(x)
        self.yb.copy_(y)

    def advance(self):
        """One more step of every pair (the first by replay); all must agree bitwise."""
        self.feed(self.step)
        self.graph.replay()
        for m, o in self.runs[1:]:
            self.body(m, o)
        torch.cuda.synchronize()
        ref = _state(*self.runs[0])
        for k, (m, o) in enumerate(self.runs[1:]):
            assert _same(ref, _state(m, o)), (self.step, k)
        self.step += 1


def test_captured_step_averages_at_every_replay_and_follows_set_ema_decay():
    r = _Runs(2)
    (m1, o1), (m2, o2) = r.runs
    assert _same(_state(m1, o1), _state(m2, o2))
    seen = [o1._arena.ema.clone()]
    for _ in range(3):
        r.advance()
        seen.append(o1._arena.ema.clone())
    for o in (o1, o2):
        o.set_ema_decay(0.5)  # no re-capture
    assert o1.ema_decay == 0.5
    before, w_before = o1._arena.ema.clone(), o1._arena.data.clone()
    r.advance()
    seen.append(o1._arena.ema.clone())
    assert all(not torch.equal(seen[i], seen[j]) for i in range(len(seen)) for j in range(i))
    assert not torch.equal(o1._arena.data, w_before)
    _check_fp64(before, o1._arena.data, o1._arena.ema, 0.5, "replay at decay 0.5")
    assert o1._arena.prep_valid is not None


def test_ema_weights_swaps_for_evaluation_and_training_continues_bitwise():
    """Pair 0 replays its captured step, pair 1 steps eagerly, pair 2 is the twin that never swaps."""
    r = _Runs(3)
    cdp = r.cdp
    r.advance()
    x, _ = _batch(77)
    for k in (0, 1):
        model, opt = r.runs[k]
        arena = opt._arena
        w, e = arena.data.clone(), arena.ema.clone()
        assert not torch.equal(w, e)
        fresh = cdp.VGG11().cuda()
        fresh.load_state_dict(model.state_dict())  # the live BatchNorm buffers
        with torch.no_grad():
            for p, q in zip(fresh.parameters(), model.parameters()):
                p.copy_(opt.ema_state()[q])
        model.eval()
        fresh.eval()
        with torch.no_grad():
            y_live = model(x).clone()
            with opt.ema_weights():
                assert torch.equal(arena.data, e) and torch.equal(arena.ema, w)
                y_ema = model(x).clone()
                assert torch.equal(y_ema, fresh(x)), k
            assert torch.equal(arena.data, w) and torch.equal(arena.ema, e)
            assert torch.equal(model(x), y_live), k
        assert not torch.equal(y_ema, y_live)
        model.train()
    r.advance()  # replay (the refreshed weight products), eager, and the twin
    r.advance()
    # entering while a stream is capturing is refused, and the weights stay where they are
    model, opt = r.runs[1]
    w = opt._arena.data.clone()
    scratch = torch.zeros(8, device="cuda")
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="capturing"):
        with torch.cuda.graph(g2):
            scratch.add_(1.0)
            with opt.ema_weights():
                pass
    torch.cuda.synchronize()
    assert torch.equal(opt._arena.data, w)


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
        opt = cdp.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4, ema_decay=0.9)
        if kind == "overlap":
            model.overlap_optimizer(opt)
        return model, opt

    runs = {k: make(k) for k in ("plain", "ddp", "overlap")}
    gen0 = runs["ddp"][1]._arena.layout_gen

    def state(model, opt):
        ps = list(model.parameters())
        return ([p.detach().clone() for p in ps] + [opt.state[p]["momentum_buffer"].clone() for p in ps]
                + [opt.state[p]["ema_buffer"].clone() for p in ps])

    for step in range(3):
        for m, o in runs.values():
            o.zero_grad()
            crit(m(xs[step]), ys[step]).backward()
            o.step()
        ref = state(*runs["plain"])
        for k in ("ddp", "overlap"):
            for u, v in zip(ref, state(*runs[k])):
                assert torch.equal(u, v), (step, k)
        # bucket_steps declined: the step ran whole at step()
        assert runs["overlap"][0].reducer.stepped_buckets() == 0
        assert runs["overlap"][1]._overlap is None
    m, o = runs["plain"]
    assert any(not torch.equal(o.state[p]["ema_buffer"], p.detach()) for p in m.parameters())
    assert runs["ddp"][1]._arena.layout_gen > gen0, "no relayout happened"
    for k in ("ddp", "overlap"):
        a = runs[k][1]._arena
        assert all(runs[k][1].state[p]["ema_buffer"].data_ptr() == a.ema.data_ptr() + 4 * a.offsets[p._cdp_index]
                   for p in a.params)
    dist.destroy_process_group()
    print("EMA_DDP_OK")
    """
)


def test_one_rank_ddp_with_ema_is_bitwise_the_plain_model():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", DDP_SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert "EMA_DDP_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-5000:]
