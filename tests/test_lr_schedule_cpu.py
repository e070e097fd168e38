"""The learning-rate schedule of the fused SGD / LARS step, host side: ``LRSchedule.factor`` (the formula the
kernels evaluate on the device, in Python floats), its validation, the CPU / reference path of
``SGD(lr_schedule=...)`` / ``LARS(lr_schedule=...)``, the state round trips and the CLI.

Rates are compared after rounding to fp32, as the step uses them: two correct fp64 evaluations of one
formula can land on either side of an fp32 rounding boundary, so "equal" is "at most one fp32 ulp apart".
"""
import io
import math
import re
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest
import torch

import cs744_distributed_data_parallel_amd as cdp
from cs744_distributed_data_parallel_amd import LRSchedule

BASE = 0.1
W, T, MILESTONES = 3, 17, (5, 11)


def _closed_form(kind, t, *, W=0, s=0.0, T=0, r=0.0, power=2.0, milestones=(), gamma=0.1):
    """The issue's formulas with numpy fp64, written independently of LRSchedule.factor."""
    t = np.float64(t)
    if t < W:
        return np.float64(s) + (np.float64(1.0) - np.float64(s)) * t / np.float64(W)
    if kind == "constant":
        return np.float64(1.0)
    if kind in ("cosine", "poly"):
        if t >= T:
            return np.float64(r)
        u = (t - W) / np.float64(T - W)
        if kind == "cosine":
            return r + (1.0 - r) * 0.5 * (1.0 + np.cos(np.pi * u))
        return r + (1.0 - r) * np.power(1.0 - u, np.float64(power))
    f = np.float64(1.0)
    for m in milestones:
        if m <= t:
            f = f * np.float64(gamma)
    return f


def _rate32(base, f):
    return np.float32(np.float64(base) * np.float64(f))


def _one_ulp(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(np.float64(a) - np.float64(b)) <= np.float64(np.spacing(np.float32(max(abs(a), abs(b)))))


CONFIGS = [
    dict(kind="constant", warmup_steps=W, warmup_start_factor=0.25),
    dict(kind="cosine", total_steps=T, warmup_steps=W, warmup_start_factor=0.1, end_factor=0.01),
    dict(kind="cosine", total_steps=T),
    dict(kind="poly", total_steps=T, warmup_steps=W, end_factor=0.001, power=2.0),
    dict(kind="poly", total_steps=T, warmup_steps=0, end_factor=0.0, power=1.0),
    dict(kind="poly", total_steps=T, warmup_steps=W, warmup_start_factor=1.0, power=0.5),
    dict(kind="step", warmup_steps=W, milestones=MILESTONES, gamma=0.1),
    dict(kind="step", milestones=(0, 1, 2, 3, 4, 5, 6, 7), gamma=0.5),
]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(f"{k[0]}{v}" for k, v in c.items()))
def test_factor_is_the_closed_form(cfg):
    sched = LRSchedule(**cfg)
    kw = dict(W=cfg.get("warmup_steps", 0), s=cfg.get("warmup_start_factor", 0.0), T=cfg.get("total_steps", 0),
              r=cfg.get("end_factor", 0.0), power=cfg.get("power", 2.0), milestones=cfg.get("milestones", ()),
              gamma=cfg.get("gamma", 0.1))
    for t in range(0, 23):
        f, ref = sched.factor(t), _closed_form(cfg["kind"], t, **kw)
        assert isinstance(f, float)
        assert _one_ulp(_rate32(BASE, f), _rate32(BASE, ref)), (t, f, ref)
        assert sched.rate(BASE, t) == float(_rate32(BASE, f))
    # the exact points: the start of the warm-up, the constant phase, the end branch
    if kw["W"]:
        assert sched.factor(0) == kw["s"]
    if cfg["kind"] == "constant":
        assert all(sched.factor(t) == 1.0 for t in range(kw["W"], 23))
    if cfg["kind"] in ("cosine", "poly"):
        assert all(sched.factor(t) == kw["r"] for t in (T, T + 1, 10 ** 9))
        assert sched.factor(kw["W"]) == 1.0
    if cfg["kind"] == "step" and cfg["gamma"] == 0.1 and not kw["W"] == 0:
        assert sched.factor(4) == 1.0 and sched.factor(5) == 0.1 and sched.factor(11) == 0.1 * 0.1


def _torch_rates(make, n):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    s = make(opt)
    out = []
    for _ in range(n):
        out.append(s.get_last_lr()[0])
        opt.step()
        s.step()
    return out


def test_factor_against_torch_schedulers_where_they_coincide():
    from torch.optim import lr_scheduler as tls

    n = T + 1  # torch's cosine and polynomial forms are periodic / clamped differently past T: up to T itself
    cases = [
        (LRSchedule("cosine", total_steps=T, end_factor=0.01),
         lambda o: tls.CosineAnnealingLR(o, T_max=T, eta_min=BASE * 0.01), n),
        (LRSchedule("cosine", total_steps=T), lambda o: tls.CosineAnnealingLR(o, T_max=T), n),
        (LRSchedule("poly", total_steps=T, power=2.0), lambda o: tls.PolynomialLR(o, total_iters=T, power=2.0), n + 5),
        (LRSchedule("poly", total_steps=T, power=1.0), lambda o: tls.PolynomialLR(o, total_iters=T, power=1.0), n + 5),
        (LRSchedule("step", milestones=MILESTONES, gamma=0.1),
         lambda o: tls.MultiStepLR(o, milestones=list(MILESTONES), gamma=0.1), n + 5),
        (LRSchedule("constant", warmup_steps=5, warmup_start_factor=0.25),
         lambda o: tls.LinearLR(o, start_factor=0.25, end_factor=1.0, total_iters=5), 12),
    ]
    for sched, make, steps in cases:
        ref = _torch_rates(make, steps)
        for t, r in enumerate(ref):
            assert _one_ulp(np.float32(sched.rate(BASE, t)), np.float32(r)), (sched, t, sched.rate(BASE, t), r)
        assert len(set(ref)) > 1


BAD = [
    dict(kind="exponential"),
    dict(kind="cosine"),  # no total_steps
    dict(kind="cosine", total_steps=5, warmup_steps=5),
    dict(kind="poly", total_steps=4, warmup_steps=5),
    dict(kind="poly", total_steps=10.5),
    dict(kind="constant", warmup_steps=-1),
    dict(kind="constant", warmup_steps=2.5),
    dict(kind="constant", warmup_start_factor=-0.1),
    dict(kind="constant", warmup_start_factor=1.1),
    dict(kind="constant", warmup_start_factor=float("nan")),
    dict(kind="cosine", total_steps=10, end_factor=-0.01),
    dict(kind="cosine", total_steps=10, end_factor=float("nan")),
    dict(kind="poly", total_steps=10, power=0.0),
    dict(kind="poly", total_steps=10, power=-1.0),
    dict(kind="step", gamma=0.0),
    dict(kind="step", gamma=-0.5),
    dict(kind="step", milestones=(3, 3)),
    dict(kind="step", milestones=(5, 2)),
    dict(kind="step", milestones=(-1, 2)),
    dict(kind="step", milestones=tuple(range(9))),
]


@pytest.mark.parametrize("kw", BAD, ids=lambda c: "-".join(f"{k[0]}{v}" for k, v in c.items()))
def test_every_bad_value_is_a_value_error(kw):
    with pytest.raises(ValueError):
        LRSchedule(**kw)


def test_bad_arguments_of_the_optimizer_and_the_handles():
    p = torch.nn.Parameter(torch.zeros(3))
    with pytest.raises(TypeError):
        cdp.SGD([p], lr=0.1, lr_schedule="cosine")
    plain = cdp.SGD([p], lr=0.1)
    assert plain.lr_schedule is None and plain.schedule_step is None and plain.last_lr is None
    assert "lr_schedule_step" not in plain.state_dict()["param_groups"][0]
    for call in (lambda: plain.set_schedule_step(1), lambda: plain.set_lr_schedule(LRSchedule("constant")),
                 lambda: plain.lr_schedule_table(0, 2)):
        with pytest.raises(RuntimeError, match="without lr_schedule"):
            call()
    opt = cdp.SGD([p], lr=0.1, lr_schedule=LRSchedule("constant"))
    with pytest.raises(ValueError):
        opt.set_schedule_step(-1)
    with pytest.raises(ValueError):
        LRSchedule("constant").factor(-1)
    with pytest.raises(TypeError):
        opt.set_lr_schedule("poly")
    assert opt.schedule_step.dtype == torch.int64 and opt.schedule_step.dim() == 0
    assert opt.last_lr.dtype == torch.float32 and opt.last_lr.dim() == 0


# ----------------------------------------------------------------------------- the CPU path
def _mlp(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def _backward(model, opt, step):
    g = torch.Generator().manual_seed(100 + step)
    x = torch.randn(4, 6, generator=g)
    opt.zero_grad()
    model(x).square().sum().backward()


def _make(cls, seed=0, **kw):
    model = _mlp(seed)
    if cls == "lars":
        opt = cdp.LARS(model.parameters(), lr=BASE, momentum=0.9, weight_decay=1e-3, trust_coefficient=0.02, **kw)
    else:
        opt = cdp.SGD(model.parameters(), lr=BASE, momentum=0.9, weight_decay=1e-3, nesterov=True, **kw)
    return model, opt


def _snapshot(model, opt):
    return [p.detach().clone() for p in model.parameters()] + [opt.state[p]["momentum_buffer"].clone()
                                                               for p in model.parameters()]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


SCHED = dict(kind="cosine", total_steps=10, warmup_steps=4, warmup_start_factor=0.1, end_factor=0.05)


@pytest.mark.parametrize("cls", ["sgd", "lars"])
def test_twelve_scheduled_steps_are_twelve_steps_at_the_rates_set_by_hand(cls):
    sched = LRSchedule(**SCHED)
    m1, o1 = _make(cls, lr_schedule=sched)
    m2, o2 = _make(cls)
    rates = []
    for t in range(12):  # the warm-up, the cosine phase and two steps past its end
        assert int(o1.schedule_step) == t
        rate = torch.tensor(BASE * sched.factor(t), dtype=torch.float64).to(torch.float32).item()
        o2.param_groups[0]["lr"] = rate
        for m, o in ((m1, o1), (m2, o2)):
            _backward(m, o, t)
            o.step()
        assert _same(_snapshot(m1, o1), _snapshot(m2, o2)), t
        assert float(o1.last_lr) == rate
        rates.append(rate)
    assert int(o1.schedule_step) == 12 and o1.param_groups[0]["lr"] == BASE  # the base rate is untouched
    assert len(set(rates[:10])) == 10 and rates[10] == rates[11] == float(np.float32(BASE * 0.05))
    assert torch.equal(o1.lr_schedule_table(0, 12), torch.tensor(rates, dtype=torch.float32))


def test_a_step_without_gradients_and_a_skipped_step_still_count():
    m, o = _make("sgd", lr_schedule=LRSchedule(**SCHED), skip_nonfinite=True)
    o.step()  # no parameter has a gradient
    assert int(o.schedule_step) == 1
    _backward(m, o, 0)
    before = _snapshot_params(m)
    next(m.parameters()).grad[0, 0] = float("inf")
    o.step()
    assert int(o.schedule_step) == 2 and int(o.skipped_steps) == 1 and _same(before, _snapshot_params(m))
    o.set_schedule_step(7)
    assert int(o.schedule_step) == 7
    _backward(m, o, 1)
    o.step()
    assert float(o.last_lr) == LRSchedule(**SCHED).rate(BASE, 7) and int(o.schedule_step) == 8
    o.set_lr_schedule(LRSchedule("step", milestones=(8,), gamma=0.5))
    _backward(m, o, 2)
    o.step()
    assert float(o.last_lr) == float(np.float32(BASE * 0.5)) and int(o.schedule_step) == 9


def _snapshot_params(model):
    return [p.detach().clone() for p in model.parameters()]


def test_several_param_groups_share_the_step_and_the_factor():
    sched = LRSchedule(**SCHED)
    m1, m2 = _mlp(0), _mlp(0)
    groups = lambda m: [dict(params=list(m[0].parameters()), lr=0.2), dict(params=list(m[2].parameters()))]
    o1 = cdp.SGD(groups(m1), lr=BASE, momentum=0.9, lr_schedule=sched)
    o2 = cdp.SGD(groups(m2), lr=BASE, momentum=0.9)
    for t in range(5):
        for g, base in zip(o2.param_groups, (0.2, BASE)):
            g["lr"] = sched.rate(base, t)
        for m, o in ((m1, o1), (m2, o2)):
            _backward(m, o, t)
            o.step()
        assert _same(_snapshot_params(m1), _snapshot_params(m2)), t
        assert int(o1.schedule_step) == t + 1 and float(o1.last_lr) == sched.rate(0.2, t)


# ----------------------------------------------------------------------------- state round trips
@pytest.mark.parametrize("cls", ["sgd", "lars"])
def test_state_dict_round_trip_continues_the_schedule_bitwise(cls, tmp_path):
    m1, o1 = _make(cls, lr_schedule=LRSchedule(**SCHED))
    for step in range(3):
        _backward(m1, o1, step)
        o1.step()
    path = cdp.utils.save_checkpoint(str(tmp_path / "c.pt"), m1, o1)
    st = torch.load(path, weights_only=True)
    assert [g["lr_schedule_step"] for g in st["optimizer"]["param_groups"]] == [3]
    m2, o2 = _make(cls, seed=7, lr_schedule=LRSchedule(**SCHED))
    cdp.utils.load_checkpoint(path, m2, o2)
    assert int(o2.schedule_step) == 3 and "lr_schedule_step" not in o2.param_groups[0]
    for step in range(3, 7):
        for m, o in ((m1, o1), (m2, o2)):
            _backward(m, o, step)
            o.step()
        assert _same(_snapshot(m1, o1), _snapshot(m2, o2)), step
        assert float(o1.last_lr) == float(o2.last_lr) == LRSchedule(**SCHED).rate(BASE, step)


def test_a_state_with_the_step_loads_into_torch_sgd_and_one_without_it_leaves_the_step(tmp_path):
    m1, o1 = _make("sgd", lr_schedule=LRSchedule("constant"))  # factor 1: torch's SGD takes the same steps
    for step in range(2):
        _backward(m1, o1, step)
        o1.step()
    path = cdp.utils.save_checkpoint(str(tmp_path / "c.pt"), m1, o1)
    st = torch.load(path, weights_only=True)
    m2 = _mlp(3)
    m2.load_state_dict(st["model"])
    o2 = torch.optim.SGD(m2.parameters(), lr=BASE, momentum=0.9, weight_decay=1e-3, nesterov=True)
    o2.load_state_dict(st["optimizer"])  # the extra key is inert
    _backward(m1, o1, 2)
    _backward(m2, o2, 2)
    o1.step()
    o2.step()
    for a, b in zip(m1.parameters(), m2.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)
    # a state without the key (torch's own optimizer, one of ours without a schedule): t stays where it is
    assert int(o1.schedule_step) == 3
    o1.load_state_dict(torch.optim.SGD(_mlp(4).parameters(), lr=BASE, momentum=0.9).state_dict())
    assert int(o1.schedule_step) == 3
    m3, o3 = _make("sgd")
    o1.load_state_dict(o3.state_dict())
    assert int(o1.schedule_step) == 3
    # and a state with the key into an optimizer without a schedule: ignored, never a live entry
    o3.load_state_dict(st["optimizer"])
    assert "lr_schedule_step" not in o3.param_groups[0] and o3.schedule_step is None


# ----------------------------------------------------------------------------- CLI
def test_train_cli_lr_schedule(tmp_path):
    from cs744_distributed_data_parallel_amd import train

    base = ["--epochs", "1", "--iters", "20", "--batch-size", "8", "--synthetic-size", "160", "--device", "cpu"]

    def run(extra, args=base):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(args + extra)
        return out.getvalue(), err.getvalue()

    def shape(s):  # the lines with their figures blanked
        return [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", ln) for ln in s.splitlines()]

    plain, plain_err = run([])
    assert "lr in iter" not in plain_err  # with none of the flags nothing changes
    ckpt = str(tmp_path / "ck")
    out, err = run(["--lr-schedule", "cosine", "--warmup-iters", "5", "--checkpoint-dir", ckpt])
    assert shape(out) == shape(plain) and "[cdp]" not in out  # stdout keeps the reference's lines
    assert len(re.findall(r"Training loss after 20 epochs is ", out)) == 1
    sched = LRSchedule("cosine", total_steps=20, warmup_steps=5)
    want = "[cdp] rank 0: lr in iter 20 is {} (schedule step 20)".format(sched.rate(0.1, 19))
    assert [ln for ln in err.splitlines() if "lr in iter" in ln] == [want], err
    # --warmup-iters alone: a constant schedule behind the warm-up
    _, err = run(["--warmup-iters", "30", "--warmup-start-factor", "0.5"])
    want = "[cdp] rank 0: lr in iter 20 is {} (schedule step 20)".format(
        LRSchedule("constant", warmup_steps=30, warmup_start_factor=0.5).rate(0.1, 19))
    assert [ln for ln in err.splitlines() if "lr in iter" in ln] == [want], err
    # --resume continues the schedule from the checkpoint: the second epoch's steps are 20 .. 39
    out, err = run(["--lr-schedule", "step", "--lr-milestones", "1", "--lr-gamma", "0.5", "--checkpoint-dir", ckpt,
                    "--resume", "--epochs", "2"])
    assert "Resumed from" in out and "(epoch 1)" in out
    want = "[cdp] rank 0: lr in iter 20 is {} (schedule step 40)".format(float(np.float32(0.1 * 0.5)))
    assert [ln for ln in err.splitlines() if "lr in iter" in ln] == [want], err
