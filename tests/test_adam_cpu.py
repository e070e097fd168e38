"""cdp.AdamW / cdp.LAMB on the CPU: the reference path (the formulas with torch ops per parameter).

Tolerance of the fp64 comparisons: both sides are fp64, about 20 operations per element per step and 10
steps: relative differences of a few 1e-15 at most, far below ``rtol=1e-10``.
"""
import copy
import io
import os
import re
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest
import torch

import cs744_distributed_data_parallel_amd as cdp

SHAPES = [(1,), (3,), (5,), (64,), (4, 3, 3, 3), (10, 16), (7, 9)]


def _params(seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g, dtype=torch.float64) * 0.05).to(dtype)) for s in SHAPES]


def _grads(step, scale=0.01):
    g = torch.Generator().manual_seed(100 + step)
    return [torch.randn(s, generator=g, dtype=torch.float64) * scale for s in SHAPES]


def _set_grads(ps, gs):
    for p, g in zip(ps, gs):
        p.grad = g.to(p.dtype).clone()


def _close(a, b):
    return all(torch.allclose(u, v, rtol=1e-10, atol=0.0) for u, v in zip(a, b))


# ----------------------------------------------------------------------------- test 1
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("maximize", [False, True])
def test_adamw_against_torch_in_fp64(wd, maximize):
    ps, qs = _params(), _params()
    a = cdp.AdamW(ps, lr=1e-2, weight_decay=wd, maximize=maximize)
    b = torch.optim.AdamW(qs, lr=1e-2, weight_decay=wd, maximize=maximize)
    for step in range(10):
        _set_grads(ps, _grads(step))
        _set_grads(qs, _grads(step))
        a.step()
        b.step()
    assert _close([p.detach() for p in ps], [q.detach() for q in qs])
    assert _close([a.state[p]["exp_avg"] for p in ps], [b.state[q]["exp_avg"] for q in qs])
    assert _close([a.state[p]["exp_avg_sq"] for p in ps], [b.state[q]["exp_avg_sq"] for q in qs])
    assert int(a.adam_step) == 10
    assert not torch.equal(ps[0].detach(), _params()[0].detach())


def _lamb_numpy(ws, grads_of, steps, lr, b1, b2, eps, wd, exclude):
    """LAMB's formulas (cdp.LAMB's docstring), transcribed: r = m^ / (sqrt(v^) + eps) + wd w, q = |w| / |r|, w -= lr q r."""
    ws = [w.copy() for w in ws]
    ms = [np.zeros_like(w) for w in ws]
    vs = [np.zeros_like(w) for w in ws]
    qs = [1.0] * len(ws)
    for t in range(1, steps + 1):
        for k, g in enumerate(grads_of(t - 1)):
            ms[k] = b1 * ms[k] + (1 - b1) * g
            vs[k] = b2 * vs[k] + (1 - b2) * g * g
            mh, vh = ms[k] / (1 - b1 ** t), vs[k] / (1 - b2 ** t)
            adapted = ws[k].ndim > 1 or not exclude
            r = mh / (np.sqrt(vh) + eps) + (wd * ws[k] if adapted else 0.0)
            wn, rn = np.sqrt(np.sum(ws[k] ** 2)), np.sqrt(np.sum(r ** 2))
            qs[k] = wn / rn if adapted and wn != 0 and rn != 0 else 1.0
            ws[k] = ws[k] - lr * qs[k] * r
    return ws, ms, vs, qs


@pytest.mark.parametrize("exclude", [True, False])
def test_lamb_against_a_numpy_transcription_in_fp64(exclude):
    ps = _params()
    with torch.no_grad():
        ps[-1].zero_()  # |w| = 0: q = 1
    opt = cdp.LAMB(ps, lr=1e-2, weight_decay=0.01, exclude_bias_and_norm=exclude)
    w0 = [p.detach().numpy().copy() for p in ps]
    for step in range(10):
        _set_grads(ps, _grads(step))
        opt.step()
        if step == 0:
            assert opt.trust_ratios[-1].item() == 1.0
    ws, ms, vs, qs = _lamb_numpy(w0, lambda s: [g.numpy() for g in _grads(s)], 10, 1e-2, 0.9, 0.999, 1e-6, 0.01, exclude)
    for p, w, m, v in zip(ps, ws, ms, vs):
        np.testing.assert_allclose(p.detach().numpy(), w, rtol=1e-10, atol=0)
        np.testing.assert_allclose(opt.state[p]["exp_avg"].numpy(), m, rtol=1e-10, atol=0)
        np.testing.assert_allclose(opt.state[p]["exp_avg_sq"].numpy(), v, rtol=1e-10, atol=0)
    np.testing.assert_allclose(opt.trust_ratios.numpy(), np.array(qs, dtype=np.float32), rtol=1e-6)
    for k, p in enumerate(ps):
        if exclude and p.dim() <= 1:
            assert opt.trust_ratios[k].item() == 1.0
        else:
            assert opt.trust_ratios[k].item() != 1.0


# ----------------------------------------------------------------------------- test 2
def test_state_dict_loads_into_torch_and_back():
    ps, qs = _params(), _params()
    a = cdp.AdamW(ps, lr=1e-2, ema_decay=0.9)  # (ema_buffer is inert in torch)
    for step in range(3):
        _set_grads(ps, _grads(step))
        a.step()
    sd = a.state_dict()
    assert all(st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 3.0
               for st in sd["state"].values())
    ref = torch.optim.AdamW(qs, lr=1e-2)
    assert set(ref.param_groups[0]) <= set(a.param_groups[0])
    assert set(a.param_groups[0]) == set(ref.param_groups[0])
    with torch.no_grad():
        for p, q in zip(ps, qs):
            q.copy_(p)
    ref.load_state_dict(copy.deepcopy(sd))  # (load_state_dict keeps the tensors it is given)
    # and the other way round, into a fresh optimizer
    rs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    c = cdp.AdamW(rs, lr=1e-2)
    c.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert int(c.adam_step) == 3
    for opt, prm in ((a, ps), (ref, qs), (c, rs)):
        _set_grads(prm, _grads(3))
        opt.step()
    assert _close([p.detach() for p in ps], [q.detach() for q in qs])
    assert _close([p.detach() for p in rs], [q.detach() for q in qs])
    assert int(a.adam_step) == 4 and int(c.adam_step) == 4
    # disagreeing step counts
    bad = ref.state_dict()
    bad["state"][0]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="disagree"):
        c.load_state_dict(bad)


def test_constructor_validation():
    ps = _params()
    with pytest.raises(ValueError):
        cdp.AdamW(ps, amsgrad=True)
    with pytest.raises(ValueError):
        cdp.LAMB(ps, amsgrad=True)
    for kw in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1e-8),
               dict(weight_decay=-0.1), dict(max_grad_norm=-1.0), dict(ema_decay=1.5)):
        for cls in (cdp.AdamW, cdp.LAMB):
            with pytest.raises(ValueError):
                cls(ps, **kw)
    opt = cdp.LAMB(ps)
    assert opt.param_groups[0]["eps"] == 1e-6 and opt.param_groups[0]["exclude_bias_and_norm"] is True
    assert opt.bucket_steps([(0, 4)], None) is None
    with pytest.raises(ValueError):
        opt.set_adam_step(-1)


# ----------------------------------------------------------------------------- test 3
@pytest.mark.parametrize("cls", ["AdamW", "LAMB"])
def test_skip_nonfinite_and_clip(cls):
    ps = _params(dtype=torch.float32)
    sched = cdp.LRSchedule("cosine", total_steps=10)
    opt = getattr(cdp, cls)(ps, lr=1e-2, skip_nonfinite=True, max_grad_norm=0.05, ema_decay=0.9, lr_schedule=sched)
    for step in range(2):
        _set_grads(ps, _grads(step))
        opt.step()
    snap = lambda: ([p.detach().clone() for p in ps] + [opt.state[p][k].clone() for p in ps  # noqa: E731
                                                         for k in ("exp_avg", "exp_avg_sq", "ema_buffer")])
    before = snap()
    _set_grads(ps, _grads(2))
    ps[3].grad[5] = float("inf")
    opt.step()
    assert all(torch.equal(u, v) for u, v in zip(before, snap()))
    assert int(opt.adam_step) == 2 and opt.skipped_steps.item() == 1
    assert int(opt.schedule_step) == 3  # the schedule counts the iteration
    # the clip scales as _clip_reference does: a step on gradients pre-multiplied by the coefficient
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    twin = getattr(cdp, cls)(qs, lr=1e-2, lr_schedule=cdp.LRSchedule("cosine", total_steps=10))
    twin.load_state_dict({"state": {k: {kk: vv for kk, vv in st.items() if kk != "ema_buffer"}
                                    for k, st in copy.deepcopy(opt.state_dict()["state"]).items()},
                          "param_groups": twin.state_dict()["param_groups"]})
    twin.set_schedule_step(3)
    gs = _grads(3, scale=1.0)
    _set_grads(ps, gs)
    opt.step()
    coef = opt.clip_coef.item()
    assert 0.0 < coef < 1.0
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g.float()) for g in gs]))
    assert opt.grad_norm.item() == total.item()
    assert coef == torch.clamp(0.05 / (total + 1e-6), max=1.0).item()
    for q, g in zip(qs, gs):
        q.grad = g.float() * opt.clip_coef
    twin.step()
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(ps, qs))
    assert int(opt.adam_step) == 3 and opt.skipped_steps.item() == 1


# ----------------------------------------------------------------------------- test 4
@pytest.mark.parametrize("name", ["adamw", "lamb"])
def test_train_cli_runs_and_resumes_to_the_same_step(name, tmp_path):
    from cs744_distributed_data_parallel_amd import train

    def run(extra):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(["--iters", "2", "--batch-size", "8", "--synthetic-size", "80", "--device", "cpu", "--optimizer",
                        name, "--lr", "0.001", "--betas", "0.9", "0.99", "--adam-eps", "1e-7", "--ema-decay", "0.9",
                        "--checkpoint-dir", str(tmp_path)] + extra)
        return out.getvalue(), err.getvalue()

    out, _ = run(["--epochs", "1"])
    assert "Size of training set is 10" in out
    assert re.search(r"Test set: Average loss: \d+\.\d{4}, Accuracy: \d+/80 \(\d+%\)", out)
    first = torch.load(os.path.join(tmp_path, "ckpt_1.pt"), weights_only=True)["optimizer"]
    g = first["param_groups"][0]
    assert tuple(g["betas"]) == (0.9, 0.99) and g["eps"] == 1e-7 and g["weight_decay"] == 0.01
    assert {float(st["step"]) for st in first["state"].values()} == {2.0}
    assert all({"exp_avg", "exp_avg_sq", "ema_buffer"} <= set(st) for st in first["state"].values())
    out, _ = run(["--epochs", "2", "--resume"])
    assert "Resumed from" in out and "(epoch 1)" in out
    second = torch.load(os.path.join(tmp_path, "ckpt_2.pt"), weights_only=True)["optimizer"]
    assert {float(st["step"]) for st in second["state"].values()} == {4.0}  # continued from t = 2


def test_train_cli_weight_decay_default_stays_for_sgd(tmp_path):
    from cs744_distributed_data_parallel_amd import train

    with redirect_stdout(io.StringIO()), redirect_stderr(io.StringIO()):
        train.main(["--epochs", "1", "--iters", "1", "--batch-size", "8", "--synthetic-size", "80", "--device", "cpu",
                    "--checkpoint-dir", str(tmp_path)])
    g = torch.load(os.path.join(tmp_path, "ckpt_1.pt"), weights_only=True)["optimizer"]["param_groups"][0]
    assert g["weight_decay"] == 0.0001 and "betas" not in g
