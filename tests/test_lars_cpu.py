"""cdp.LARS without a GPU: the pure-torch path against a small fp64 oracle of the formula, the
reduction to cdp.SGD for excluded parameters, the state_dict contract, validation and the CLI.

Bound of the oracle comparison. Every step is compared from the SAME fp32 state (the oracle reads the
optimizer's parameters, gradients and momentum before the step and evaluates one step exactly, in
fp64), so the bound is that of one pass through ``sgd_one`` (csrc/kernels/misc.hip), whose fp32
operations are, with u = 2^-24 the unit roundoff, each result r carrying at most u * |r| more error:

    q        one rounding of the fp64 value (the fp64 sums err by n * 2^-53, far below u): 2u |q| allowed
    gs_eff   (1 * 1) * q, exact products by one: e_q
    wd_eff   fl(wd) * q: the rounding of wd, of the product, and e_q: 4u |wd q|
    d        fma(w, wd_eff, g * gs_eff): |g| e_q + u |g q| + |w| e_wd + u |w wd q| + u |d|
             (the unfused form of the torch path has the one extra rounding counted here)
    buf      first: d. later: fma(d, 1 - damp, buf * m): roundings of m and 1 - damp, the product
             buf * m, the product d (1 - damp), the sum
    d_n      Nesterov: fma(buf, m, d): e_d + m e_buf + 2u |m buf| (rounding of m, product) + u |d_n|; else buf
    p        fma(d_n, -lr, p): lr e_dn + 2u |lr d_n| (rounding of lr, product) + u |p|

All magnitudes are evaluated by the oracle in fp64 per element; nothing is taken from the code
under test.
"""
import copy
import io
import re
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest
import torch

import cs744_distributed_data_parallel_amd as cdp

U = 2.0 ** -24


def _toy(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(
        torch.nn.Conv2d(3, 8, 3, padding=1), torch.nn.BatchNorm2d(8), torch.nn.ReLU(),
        torch.nn.Conv2d(8, 16, 3, padding=1), torch.nn.AdaptiveAvgPool2d(1), torch.nn.Flatten(),
        torch.nn.Linear(16, 10))


def _fwd_bwd(model, opt, step):
    g = torch.Generator().manual_seed(100 + step)
    x = torch.randn(4, 3, 8, 8, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    opt.zero_grad()
    torch.nn.functional.cross_entropy(model(x), y).backward()


def _oracle(w, g, buf, ndim, *, lr, m, damp, wd, eta, eps, nesterov, exclude):
    """One exact (fp64) LARS step of one tensor from fp32 inputs: (q, new w, new buf, bound on w,
    bound on buf), the bounds as derived in the module docstring."""
    w, g = w.astype(np.float64), g.astype(np.float64)
    adapt = ndim > 1 or not exclude
    if adapt:
        wn, gn = np.sqrt(np.sum(w * w)), np.sqrt(np.sum(g * g))
        q = 1.0 if (wn == 0 or gn == 0) else eta * wn / (gn + wd * wn + eps)
        wdw = wd
        e_q = 2 * U * abs(q)
    else:
        q, wdw, e_q = 1.0, 0.0, 0.0
    d = q * (g + wdw * w)
    e_wd = 4 * U * abs(wdw * q)
    e_d = np.abs(g) * e_q + U * np.abs(g * q) + np.abs(w) * e_wd + U * np.abs(w * wdw * q) + U * np.abs(d)
    if m != 0:
        if buf is None:
            nb, e_b = d.copy(), e_d
        else:
            b = buf.astype(np.float64)
            nb = m * b + (1 - damp) * d
            e_b = (2 * U * np.abs(m * b) + abs(1 - damp) * e_d + 2 * U * np.abs((1 - damp) * d) + U * np.abs(nb))
        if nesterov:
            dn = d + m * nb
            e_dn = e_d + m * e_b + 2 * U * np.abs(m * nb) + U * np.abs(dn)
        else:
            dn, e_dn = nb, e_b
    else:
        nb, e_b, dn, e_dn = None, None, d, e_d
    nw = w - lr * dn
    e_w = lr * e_dn + 2 * U * np.abs(lr * dn) + U * np.abs(nw)
    return q, nw, nb, e_w, e_b


VARIANTS = {
    "momentum": dict(momentum=0.9, weight_decay=1e-2),  # step 1 is the first-step rule, 2 and 3 the later one
    "nesterov": dict(momentum=0.9, weight_decay=1e-2, nesterov=True),
    "wd0": dict(momentum=0.9, weight_decay=0.0),
    "plain": dict(momentum=0.0, weight_decay=1e-2),
    "dampening": dict(momentum=0.8, dampening=0.25, weight_decay=1e-2),
}


@pytest.mark.parametrize("exclude", [True, False])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_three_steps_against_the_fp64_oracle(variant, exclude):
    hp = VARIANTS[variant]
    model = _toy()
    lr, eta, eps = 0.5, 0.02, 1e-8
    opt = cdp.LARS(model.parameters(), lr, trust_coefficient=eta, eps=eps, exclude_bias_and_norm=exclude, **hp)
    params = list(model.parameters())
    assert [tuple(p.shape) for p in params if p.dim() > 1] == [(8, 3, 3, 3), (16, 8, 3, 3), (10, 16)]
    worst = 0.0
    for step in range(3):
        _fwd_bwd(model, opt, step)
        before = []
        for p in params:
            b = opt.state[p].get("momentum_buffer")
            before.append((p.detach().numpy().copy(), p.grad.numpy().copy(), None if b is None else b.numpy().copy()))
        assert (before[0][2] is None) == (step == 0 or hp["momentum"] == 0)
        opt.step()
        ratios = opt.trust_ratios.numpy()
        for k, (p, (w, g, b)) in enumerate(zip(params, before)):
            q, nw, nb, e_w, e_b = _oracle(w, g, b, p.dim(), lr=lr, m=hp["momentum"], damp=hp.get("dampening", 0.0),
                                          wd=hp["weight_decay"], eta=eta, eps=eps, nesterov=hp.get("nesterov", False),
                                          exclude=exclude)
            adapted = p.dim() > 1 or not exclude
            if adapted:
                assert abs(float(ratios[k]) - q) <= 2 * U * abs(q), (step, k, ratios[k], q)
                assert q != 1.0 or not g.any() or not w.any()  # (BatchNorm's beta starts at zero)
            else:
                assert ratios[k] == 1.0
            err = np.abs(p.detach().numpy().astype(np.float64) - nw)
            worst = max(worst, float(np.max(err / e_w)))
            assert np.all(err <= e_w), (variant, step, k, float(np.max(err / e_w)))
            assert np.any(nw != w)
            if nb is not None:
                eb = np.abs(opt.state[p]["momentum_buffer"].numpy().astype(np.float64) - nb)
                assert np.all(eb <= e_b), (variant, step, k, float(np.max(eb / np.maximum(e_b, 1e-300))))
    print(f"{variant} exclude={exclude}: worst error / bound {worst:.3f}")


def test_excluded_parameters_get_no_weight_decay():
    model = _toy()
    opt = cdp.LARS(model.parameters(), 0.1, weight_decay=0.5, trust_coefficient=0.02)
    _fwd_bwd(model, opt, 0)
    bias = model[6].bias
    want = torch.add(bias.detach(), bias.grad, alpha=-0.1)  # as torch.optim.SGD without decay
    opt.step()
    assert torch.equal(bias.detach(), want)


def test_zero_weight_or_zero_gradient_gives_ratio_one():
    w0 = torch.nn.Parameter(torch.zeros(3, 4))
    w1 = torch.nn.Parameter(torch.ones(3, 4))
    opt = cdp.LARS([w0, w1], 0.1, weight_decay=0.1)
    w0.grad = torch.ones(3, 4)
    w1.grad = torch.zeros(3, 4)
    opt.step()
    assert opt.trust_ratios.tolist() == [1.0, 1.0]
    assert torch.equal(w0.detach(), torch.full((3, 4), -0.1))


@pytest.mark.parametrize("hp", [dict(momentum=0.9), dict(momentum=0.9, nesterov=True), dict()])
def test_one_dimensional_parameters_are_bitwise_sgd_without_decay(hp):
    def make():
        torch.manual_seed(3)
        return [torch.nn.Parameter(torch.randn(n)) for n in (1, 5, 64, 1027)]

    a, b = make(), make()
    lars = cdp.LARS(a, 0.1, weight_decay=1e-2, **hp)
    sgd = cdp.SGD(b, lr=0.1, weight_decay=0.0, **hp)
    for step in range(3):
        g = torch.Generator().manual_seed(step)
        for p, r in zip(a, b):
            p.grad = torch.randn(p.shape, generator=g)
            r.grad = p.grad.clone()
        lars.step()
        sgd.step()
        for p, r in zip(a, b):
            assert torch.equal(p, r)
            if hp:
                assert torch.equal(lars.state[p]["momentum_buffer"], sgd.state[r]["momentum_buffer"])
    assert lars.trust_ratios.tolist() == [1.0] * 4


def test_state_dict_round_trips_the_hyperparameters_and_continues_bitwise():
    m1 = _toy()
    o1 = cdp.LARS(m1.parameters(), 0.3, momentum=0.9, weight_decay=1e-3, trust_coefficient=0.05, eps=1e-6,
                  exclude_bias_and_norm=False)
    for step in range(2):
        _fwd_bwd(m1, o1, step)
        o1.step()
    sd = copy.deepcopy(o1.state_dict())
    g = sd["param_groups"][0]
    assert (g["trust_coefficient"], g["eps"], g["exclude_bias_and_norm"]) == (0.05, 1e-6, False)
    assert all(set(v) == {"momentum_buffer"} for v in sd["state"].values())
    m2 = _toy(seed=9)
    m2.load_state_dict(m1.state_dict())
    o2 = cdp.LARS(m2.parameters(), 0.1)  # other hyperparameters: all come from the state dict
    o2.load_state_dict(sd)
    g2 = o2.param_groups[0]
    assert (g2["trust_coefficient"], g2["eps"], g2["exclude_bias_and_norm"], g2["lr"]) == (0.05, 1e-6, False, 0.3)
    for step in range(2, 4):
        for m, o in ((m1, o1), (m2, o2)):
            _fwd_bwd(m, o, step)
            o.step()
        for p, r in zip(m1.parameters(), m2.parameters()):
            assert torch.equal(p, r)
            assert torch.equal(o1.state[p]["momentum_buffer"], o2.state[r]["momentum_buffer"])
        assert torch.equal(o1.trust_ratios, o2.trust_ratios)


def test_constructor_validation():
    p = [torch.nn.Parameter(torch.ones(2, 2))]
    with pytest.raises(ValueError, match="trust_coefficient"):
        cdp.LARS(p, 0.1, trust_coefficient=-1e-3)
    with pytest.raises(ValueError, match="eps"):
        cdp.LARS(p, 0.1, eps=-1.0)
    with pytest.raises(ValueError, match="learning rate"):
        cdp.LARS(p, -0.1)
    with pytest.raises(ValueError, match="Nesterov"):
        cdp.LARS(p, 0.1, nesterov=True)
    opt = cdp.LARS(p, 0.1)
    assert isinstance(opt, cdp.SGD) and isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert (g["trust_coefficient"], g["eps"], g["exclude_bias_and_norm"]) == (0.001, 1e-8, True)
    assert opt.bucket_steps([(0, 4)], None) is None


def test_train_cli_lars_keeps_the_reference_lines():
    from cs744_distributed_data_parallel_amd import train

    def run(extra):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(["--epochs", "1", "--iters", "2", "--batch-size", "8", "--synthetic-size", "80",
                        "--device", "cpu"] + extra)
        return out.getvalue(), err.getvalue()

    plain, _ = run([])
    lars, _ = run(["--optimizer", "lars", "--trust-coefficient", "0.01"])
    strip = lambda s: [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", ln) for ln in s.splitlines()]  # noqa: E731
    assert strip(plain) == strip(lars)
    assert "Size of training set is 10" in lars
    assert re.search(r"Test set: Average loss: \d+\.\d{4}, Accuracy: \d+/80 \(\d+%\)", lars)
    assert "trust ratio" not in lars


def test_train_loop_prints_the_trust_ratio_spread_to_stderr(capsys):
    from cs744_distributed_data_parallel_amd import train

    m = torch.nn.Linear(3, 2)
    opt = cdp.LARS(m.parameters(), 0.1, trust_coefficient=0.01)
    data = [(torch.randn(4, 3), torch.randint(0, 2, (4,))) for _ in range(20)]
    train.train_model(m, data, opt, torch.nn.CrossEntropyLoss(), max_iters=20)
    cap = capsys.readouterr()
    assert re.search(r"Training loss after 20 epochs is ", cap.out) and "trust ratio" not in cap.out
    assert len(re.findall(r"trust ratio in iter 20 is min \S+ max \S+", cap.err)) == 1
