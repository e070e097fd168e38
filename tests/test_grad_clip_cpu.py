"""Gradient-norm clipping and non-finite step skipping of the fused SGD, reference (CPU) paths:
parity with ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.SGD``, the skip semantics, the
state_dict contract, two gloo DDP ranks and the training CLI flags."""
import copy
import io
import os
import re
import sys
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest
import torch

import cs744_distributed_data_parallel_amd as cdp
from _dist_util import run_ranks


def _mlp():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(6, 9), torch.nn.Tanh(), torch.nn.Linear(9, 3))


def _set_grads(model, gen, scale):
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=gen) * scale


@pytest.mark.parametrize("kw", [dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.9, nesterov=True), dict()])
def test_clipped_sgd_matches_torch_clip_plus_sgd(kw):
    """Three steps with random gradients scaled so the clip is active in some steps and not in
    others; tolerance of test_sgd_matches_torch_reference."""
    a, b = _mlp(), _mlp()
    m = 1.0
    o1 = cdp.SGD(a.parameters(), lr=0.1, max_grad_norm=m, **kw)
    o2 = torch.optim.SGD(b.parameters(), lr=0.1, **kw)
    active = []
    for step, scale in enumerate([2.0, 1e-3, 0.5]):
        gen = torch.Generator().manual_seed(10 + step)
        _set_grads(a, gen, scale)
        gen = torch.Generator().manual_seed(10 + step)
        _set_grads(b, gen, scale)
        total = torch.nn.utils.clip_grad_norm_(b.parameters(), m)
        o1.step()
        o2.step()
        active.append(bool(total > m))
        assert torch.allclose(o1.grad_norm, total, rtol=1e-6)
        assert float(o1.clip_coef) == (float(torch.clamp(m / (total + 1e-6), max=1.0)))
        assert (float(o1.clip_coef) < 1.0) == active[-1]
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.allclose(p, q, atol=1e-7)
            assert torch.allclose(p.grad, q.grad, atol=1e-7)  # the reference path scales in place, as torch
    assert any(active) and not all(active)
    assert float(o1.skipped_steps) == 0


def test_skip_nonfinite_leaves_state_as_if_step_was_not_called():
    a, b = _mlp(), _mlp()
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)
    o1 = cdp.SGD(a.parameters(), skip_nonfinite=True, max_grad_norm=5.0, **kw)
    o2 = torch.optim.SGD(b.parameters(), **kw)

    def both(step, poison=False):
        for mdl in (a, b):
            _set_grads(mdl, torch.Generator().manual_seed(step), 0.3)
        if poison:
            next(iter(a.parameters())).grad[1, 2] = float("inf")
        o1.step()
        if not poison:
            torch.nn.utils.clip_grad_norm_(b.parameters(), 5.0)
            o2.step()  # torch's "step() not called" on the poisoned iteration

    both(0)
    before = [p.detach().clone() for p in a.parameters()]
    bufs = [o1.state[p]["momentum_buffer"].clone() for p in a.parameters()]
    both(1, poison=True)
    assert float(o1.skipped_steps) == 1
    assert not np.isfinite(float(o1.grad_norm))
    for p, p0, b0, q in zip(a.parameters(), before, bufs, b.parameters()):
        assert torch.equal(p, p0) and torch.equal(o1.state[p]["momentum_buffer"], b0)
        assert torch.allclose(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"], atol=1e-7)
    both(2)
    assert float(o1.skipped_steps) == 1
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, atol=1e-7)
        assert torch.allclose(o1.state[p]["momentum_buffer"], o2.state[q]["momentum_buffer"], atol=1e-7)


def test_skipped_first_step_leaves_no_momentum_state():
    a, b = _mlp(), _mlp()
    o1 = cdp.SGD(a.parameters(), lr=0.1, momentum=0.9, skip_nonfinite=True)
    o2 = torch.optim.SGD(b.parameters(), lr=0.1, momentum=0.9)
    _set_grads(a, torch.Generator().manual_seed(0), 1.0)
    next(iter(a.parameters())).grad[0, 0] = float("nan")
    o1.step()
    assert float(o1.skipped_steps) == 1
    assert all("momentum_buffer" not in o1.state[p] for p in a.parameters())
    for mdl in (a, b):
        _set_grads(mdl, torch.Generator().manual_seed(1), 1.0)
    o1.step()
    o2.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, atol=1e-7)


def test_skip_nonfinite_rejects_dampening_and_bad_max_norm():
    p = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError):
        cdp.SGD(p, lr=0.1, momentum=0.9, dampening=0.1, skip_nonfinite=True)
    with pytest.raises(ValueError):
        cdp.SGD(p, lr=0.1, max_grad_norm=-1.0)
    with pytest.raises(TypeError):
        cdp.SGD(p, 0.1, 0.9, 0.0, 0.0, False, 1.0)  # keyword-only
    o = cdp.SGD(p, lr=0.1)
    assert o.grad_norm is None and o.clip_coef is None and o.skipped_steps is None


def test_state_dict_keys_unchanged_with_clipping_on():
    def sd(**kw):
        m = torch.nn.Linear(4, 2)
        o = cdp.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, **kw)
        m(torch.ones(3, 4)).sum().backward()
        o.step()
        return o.state_dict()

    plain, clipped = sd(), sd(max_grad_norm=0.5, skip_nonfinite=True)
    assert set(plain) == set(clipped)
    assert set(plain["param_groups"][0]) == set(clipped["param_groups"][0])
    assert set(clipped["state"][0]) == {"momentum_buffer"}
    o2 = torch.optim.SGD(torch.nn.Linear(4, 2).parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    o2.load_state_dict(clipped)


def test_clip_grad_norm_function_delegates_on_cpu():
    a, b = _mlp(), _mlp()
    for mdl in (a, b):
        _set_grads(mdl, torch.Generator().manual_seed(3), 2.0)
    for kw in (dict(), dict(norm_type=float("inf"))):
        n1 = cdp.clip_grad_norm_(a.parameters(), 0.7, **kw)
        n2 = torch.nn.utils.clip_grad_norm_(b.parameters(), 0.7, **kw)
        assert torch.equal(n1, n2)
        for p, q in zip(a.parameters(), b.parameters()):
            assert torch.equal(p.grad, q.grad)


# ----------------------------------------------------------------------------- two gloo ranks
_B = 4  # per-rank batch
_MAXN = 0.05


def _batch(step, lo, hi):
    g = torch.Generator().manual_seed(1000 + step)
    x = torch.randn(2 * _B, 6, generator=g)
    y = torch.randn(2 * _B, 3, generator=g) * 3
    return x[lo:hi], y[lo:hi]


def _ddp_clipped(rank, world):
    import cs744_distributed_data_parallel_amd as cdp

    net = cdp.DistributedDataParallel(_mlp())
    opt = cdp.SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, max_grad_norm=_MAXN)
    coefs = []
    for step in range(3):
        x, y = _batch(step, rank * _B, (rank + 1) * _B)
        opt.zero_grad()
        torch.nn.functional.mse_loss(net(x), y).backward()
        opt.step()
        coefs.append(float(opt.clip_coef))
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).numpy(), coefs


def test_two_rank_ddp_with_max_grad_norm_matches_one_process():
    (f0, c0), (f1, c1) = run_ranks(_ddp_clipped, 2)
    np.testing.assert_allclose(f0, f1, rtol=0, atol=1e-6, err_msg="ranks diverged")
    assert min(c0) < 1.0  # the clip was active
    model = _mlp()
    opt = cdp.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, max_grad_norm=_MAXN)
    for step in range(3):
        x, y = _batch(step, 0, 2 * _B)
        opt.zero_grad()
        torch.nn.functional.mse_loss(model(x), y).backward()
        opt.step()
    ref = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    np.testing.assert_allclose(f0, ref, rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------- CLI
def test_train_cli_clip_flags_keep_the_reference_lines():
    from cs744_distributed_data_parallel_amd import train

    def run(extra):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(["--epochs", "1", "--iters", "2", "--batch-size", "8", "--synthetic-size", "80",
                        "--device", "cpu"] + extra)
        return out.getvalue(), err.getvalue()

    plain, _ = run([])
    clipped, err = run(["--clip-grad-norm", "1.0", "--skip-nonfinite"])
    strip = lambda s: [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", ln) for ln in s.splitlines()]  # noqa: E731
    assert strip(plain) == strip(clipped)
    assert "Size of training set is 10" in clipped
    assert re.search(r"Test set: Average loss: \d+\.\d{4}, Accuracy: \d+/80 \(\d+%\)", clipped)
    assert "grad norm" not in clipped


def test_train_cli_prints_the_grad_norm_to_stderr_every_window(capsys):
    from cs744_distributed_data_parallel_amd import train

    m = torch.nn.Linear(3, 2)
    opt = cdp.SGD(m.parameters(), lr=0.1, max_grad_norm=0.01)
    data = [(torch.randn(4, 3), torch.randint(0, 2, (4,))) for _ in range(20)]
    train.train_model(m, data, opt, torch.nn.CrossEntropyLoss(), max_iters=20)
    cap = capsys.readouterr()
    assert re.search(r"Training loss after 20 epochs is ", cap.out) and "grad norm" not in cap.out
    assert len(re.findall(r"grad norm in iter 20 is \d", cap.err)) == 1
