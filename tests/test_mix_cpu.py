"""mixup / CutMix on the CPU path: the mixed batches of DeviceLoader, the two-target cross-entropy
fallback, CrossEntropyLoss with a MixTarget, the argument checks and the CLI flags."""
import io
import math
import re
from contextlib import redirect_stderr, redirect_stdout

import pytest
import torch
import torch.nn.functional as F

from _mix_util import CASES, MIX, check_default_arguments_change_nothing, check_mixed_batches, dataset


@pytest.mark.parametrize("B,H,W", CASES)
def test_cpu_mixed_batches_follow_the_unmixed_batch(B, H, W):
    check_mixed_batches(B, H, W, "cpu")


def test_cpu_default_mix_arguments_change_nothing():
    check_default_arguments_change_nothing("cpu")


def test_cpu_mix_leaves_the_crop_and_flip_draws_and_the_global_rng_alone():
    """The mix parameters come from a generator of their own: mode `none` batches equal the unmixed ones
    (checked above), the counter advances once per batch, and torch's default generator is untouched."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    ds = dataset(4, 8, 8, "cpu")
    ld = DeviceLoader(ds, 4, seed=2, **MIX)
    idx = torch.arange(len(ds))
    torch.manual_seed(77)
    want = torch.rand(3)
    torch.manual_seed(77)
    for k in range(3):
        assert int(ld._counter.item()) == k
        ld.batch(idx, 0, 4)
    assert torch.equal(torch.rand(3), want)
    # no padding and no nbatches: the counter still advances, so every batch has its own mix
    ds0 = dataset(4, 8, 8, "cpu")
    ds0.pad = 0
    l0 = DeviceLoader(ds0, 4, seed=2, mixup_alpha=1.0)
    lams = {l0.batch(idx, 0, 4)[1].lam.item() for _ in range(4)}
    assert int(l0._counter.item()) == 4 and len(lams) == 4
    # the iterator yields MixTargets too
    data, tgt = next(iter(ld))
    assert hasattr(tgt, "target_b") and data.shape[0] == 4


def _closed_form(z, a, b, lam, eps):
    """logsumexp(z) - (1 - eps) (lam z_a + (1 - lam) z_b) - (eps / C) sum z, and its gradient."""
    C = z.shape[1]
    lse = torch.logsumexp(z, 1)
    za, zb = z.gather(1, a[:, None])[:, 0], z.gather(1, b[:, None])[:, 0]
    loss = (lse - (1 - eps) * (lam * za + (1 - lam) * zb) - eps / C * z.sum(1)).mean()
    oa, ob = F.one_hot(a, C).to(z.dtype), F.one_hot(b, C).to(z.dtype)
    grad = (torch.softmax(z, 1) - (1 - eps) * (lam * oa + (1 - lam) * ob) - eps / C) / z.shape[0]
    return loss, grad


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [0.3, 1.0, 0.0])
def test_cross_entropy_fallback_matches_the_closed_form(eps, lam):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    g = torch.Generator().manual_seed(3)
    z = (3 * torch.randn(7, 10, generator=g, dtype=torch.float64)).requires_grad_()
    a = torch.randint(0, 10, (7,), generator=g)
    b = torch.randint(0, 10, (7,), generator=g)
    b[:2] = a[:2]  # rows whose two targets coincide: the weights add on one class
    for lam_arg in (lam, torch.tensor([lam], dtype=torch.float64)):
        z.grad = None
        loss = CF.cross_entropy(z, a, label_smoothing=eps, target_b=b, lam=lam_arg)
        assert loss.dim() == 0
        loss.backward()
        want, wgrad = _closed_form(z.detach(), a, b, lam, eps)
        assert abs(loss.item() - want.item()) < 1e-12
        assert (z.grad - wgrad).abs().max().item() < 1e-12


def test_bad_arguments_raise():
    from cs744_distributed_data_parallel_amd.data import DeviceLoader
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    ds = dataset(4, 8, 8, "cpu")
    for kw in (dict(mixup_alpha=-0.1), dict(cutmix_alpha=-1.0), dict(mix_prob=1.5), dict(mix_prob=-0.1),
               dict(mix_switch_prob=2.0), dict(mix_switch_prob=-0.5), dict(mixup_alpha=float("nan"))):
        with pytest.raises(ValueError):
            DeviceLoader(ds, 4, **kw)
    z = torch.randn(4, 10)
    t = torch.randint(0, 10, (4,))
    with pytest.raises(ValueError):
        CF.cross_entropy(z, t, target_b=t)
    with pytest.raises(ValueError):
        CF.cross_entropy(z, t, lam=0.5)
    with pytest.raises(ValueError):
        CF.cross_entropy(z, t, target_b=t, lam=1.5)
    with pytest.raises(ValueError):
        CF.cross_entropy(z, t, target_b=t, lam=torch.tensor([0.5, 0.5]))


def test_criterion_takes_a_mix_target():
    import cs744_distributed_data_parallel_amd as cdp

    g = torch.Generator().manual_seed(4)
    z = torch.randn(6, 10, generator=g, dtype=torch.float64).requires_grad_()
    a = torch.randint(0, 10, (6,), generator=g)
    info = torch.tensor([1, 0.25, 0.25, 0, 0, 0, 0, 0], dtype=torch.float32)
    tgt = cdp.MixTarget(a, a.flip(0), info[1:2], info)
    crit = cdp.CrossEntropyLoss(label_smoothing=0.1)
    loss = crit(z, tgt)
    want, wgrad = _closed_form(z.detach(), a, a.flip(0), 0.25, 0.1)
    loss.backward()
    assert abs(loss.item() - want.item()) < 1e-12 and (z.grad - wgrad).abs().max().item() < 1e-12
    # a plain tensor target is the criterion it always was
    assert torch.equal(crit(z, a), F.cross_entropy(z, a, label_smoothing=0.1))
    # unpacking a batch as (data, target) still works for a loop that never looks inside the target
    data, target = (torch.zeros(1), tgt)
    assert target is tgt


def _cli(extra):
    from cs744_distributed_data_parallel_amd import train

    out, err = io.StringIO(), io.StringIO()
    with redirect_stdout(out), redirect_stderr(err):
        train.main(["--device", "cpu", "--model", "vgg11", "--synthetic-size", "64", "--batch-size", "16",
                    "--iters", "2"] + extra)
    return out.getvalue(), err.getvalue()


def test_train_cli_mix_flags_keep_the_reference_lines():
    """Two iterations with mixing on: the run ends, every loss it prints is finite (the two-iteration run
    prints the test-set loss; a `Training loss` line comes with iteration 20), and stdout's line set is
    that of a run without the flags."""
    plain, _ = _cli([])
    mixed, _ = _cli(["--mixup-alpha", "0.2", "--cutmix-alpha", "1.0"])
    strip = lambda s: [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", ln) for ln in s.splitlines()]  # noqa: E731
    assert strip(plain) == strip(mixed)
    losses = [float(v) for v in re.findall(r"Training loss after \d+ \w+ is (?:tensor\()?(-?[\d.]+(?:e-?\d+)?|nan|inf)", mixed)]
    losses += [float(v) for v in re.findall(r"Average loss: (-?[\d.]+|nan|inf)", mixed)]
    assert losses and all(math.isfinite(v) for v in losses), mixed


def test_train_loop_prints_the_mix_line_on_stderr():
    """train_model over 20 mixed batches: stdout keeps the reference's lines, stderr gets one mix line."""
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.data import DeviceLoader
    from cs744_distributed_data_parallel_amd.train import train_model

    ds = dataset(4, 8, 8, "cpu")
    ld = DeviceLoader(ds, 1, seed=0, **MIX)  # 13 images: two passes make 20 iterations
    model = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(3 * 8 * 8, 10))
    opt = cdp.SGD(model.parameters(), lr=0.01)
    out, err = io.StringIO(), io.StringIO()

    class Twice:
        def __iter__(self):
            yield from ld
            yield from ld

    with redirect_stderr(err):
        train_model(model, Twice(), opt, cdp.CrossEntropyLoss(), max_iters=20, print_fn=lambda s: out.write(s + "\n"))
    lines = [ln for ln in err.getvalue().splitlines() if "mix in iter" in ln]
    assert len(lines) == 1 and re.fullmatch(r"\[cdp\] rank 0: mix in iter 20 is mode (none|mixup|cutmix) lam [\d.e-]+",
                                            lines[0]), err.getvalue()
    assert "mix" not in out.getvalue() and "Training loss after 20" in out.getvalue()
