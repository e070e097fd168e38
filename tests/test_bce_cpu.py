"""Binary cross-entropy over index and mixed targets, PyTorch composition (CPU): CF.binary_cross_entropy and
cdp.BinaryCrossEntropy against F.binary_cross_entropy_with_logits on the dense target in fp64, the lam = 1 and
target_b == target identities, the dense float target form, the argument checks and the CLI flags."""
import itertools

import pytest
import torch
import torch.nn.functional as F


def dense_target(t, C, eps=0.0, thr=None, tb=None, lam=None):
    """y = ((c == t_a ? wa : 0) + (c == t_b ? wb : 0)) + off in fp32, each step rounded on its own, then
    y > thr: timm's mixup_target + BinaryCrossEntropy target, written out with torch ops."""
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    lam = f(1.0) if lam is None else f(float(lam))
    on = f(1.0) - f(eps)
    off = f(eps) / C
    wa, wb = on * lam, on * (f(1.0) - lam)
    cls = torch.arange(C).unsqueeze(0)
    ya = torch.where(cls == t.cpu().unsqueeze(1), wa, f(0.0))
    yb = torch.where(cls == tb.cpu().unsqueeze(1), wb, f(0.0)) if tb is not None else torch.zeros_like(ya)
    y = (ya + yb) + off
    if thr is not None:
        y = (y > thr).float()
    return y


def ref_loss(z, y, sum_classes):
    l = F.binary_cross_entropy_with_logits(z.double(), y.double(), reduction="none")
    return l.sum(1).mean() if sum_classes else l.mean()


def _case(B=9, C=10):
    torch.manual_seed(5)
    return 3 * torch.randn(B, C), torch.randint(0, C, (B,))


CONFIGS = list(itertools.product([0.0, 0.1], [None, 0.2], [False, True], [None, 0.3, 0.9]))


@pytest.mark.parametrize("eps,thr,sum_classes,lam", CONFIGS)
def test_torch_path_matches_dense_fp64(eps, thr, sum_classes, lam):
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    z, t = _case()
    tb = t.flip(0) if lam is not None else None
    y = dense_target(t, z.shape[1], eps, thr, tb, lam)
    zr = z.double().requires_grad_()
    ref = ref_loss(zr, y, sum_classes)
    ref.backward()
    crit = cdp.BinaryCrossEntropy(eps, target_threshold=thr, sum_classes=sum_classes)
    for how in ("functional", "module"):
        a = z.clone().requires_grad_()
        if how == "functional":
            loss = CF.binary_cross_entropy(a, t, eps, thr, sum_classes, target_b=tb, lam=lam)
        elif lam is None:
            loss = crit(a, t)
        else:
            lam_t = torch.tensor([lam])
            loss = crit(a, cdp.MixTarget(t, tb, lam_t, torch.tensor([1.0, lam])))
        loss.backward()
        assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item())), how
        err = ((a.grad.double() - zr.grad).norm() / zr.grad.norm()).item()
        assert err < 1e-5, (how, err)


def test_identities():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    z, t = _case()
    for eps, thr in ((0.0, None), (0.1, None), (0.1, 0.2)):
        plain = CF.binary_cross_entropy(z, t, eps, thr)
        assert torch.equal(CF.binary_cross_entropy(z, t, eps, thr, target_b=t.flip(0), lam=1.0), plain)
        assert torch.equal(CF.binary_cross_entropy(z, t, eps, thr, target_b=t.flip(0), lam=torch.tensor([1.0])), plain)
    # the same class in both slots is the one-hot row for any lam (eps = 0, no threshold)
    assert torch.equal(CF.bce_dense_target(t, 10, target_b=t, lam=0.37), F.one_hot(t, 10).float())
    assert torch.equal(CF.binary_cross_entropy(z, t, target_b=t, lam=0.37), CF.binary_cross_entropy(z, t))
    # defaults spelled out
    assert torch.equal(CF.binary_cross_entropy(z, t, 0.1, target_threshold=None, sum_classes=False),
                       CF.binary_cross_entropy(z, t, 0.1))
    # a threshold of 0.2: lam = 0.9 leaves the partner (0.09 + off) negative, lam = 0.5 makes both positive
    thr = CF.binary_cross_entropy(z, t, 0.1, 0.2)
    assert torch.equal(CF.binary_cross_entropy(z, t, 0.1, 0.2, target_b=t.flip(0), lam=0.9), thr)
    assert not torch.equal(CF.binary_cross_entropy(z, t, 0.1, 0.2, target_b=t.flip(0), lam=0.5), thr)


def test_non_2d_logits_take_the_torch_path():
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    z, t = _case(12, 7)
    a = CF.binary_cross_entropy(z.reshape(3, 4, 7), t.reshape(3, 4), 0.1)
    assert torch.allclose(a, CF.binary_cross_entropy(z, t, 0.1))


@pytest.mark.parametrize("sum_classes", [False, True])
def test_dense_float_target(sum_classes):
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    z, _ = _case()
    torch.manual_seed(1)
    y = torch.rand_like(z)
    a = z.clone().requires_grad_()
    loss = CF.binary_cross_entropy(a, y, sum_classes=sum_classes)
    zr = z.double().requires_grad_()
    ref = ref_loss(zr, y, sum_classes)
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    loss.backward()
    ref.backward()
    assert ((a.grad.double() - zr.grad).norm() / zr.grad.norm()).item() < 1e-5
    # the threshold binarises a dense target too; the module hands a float target through
    crit = cdp.BinaryCrossEntropy(0.1, target_threshold=0.5, sum_classes=sum_classes)
    refb = ref_loss(z, (y > 0.5).float(), sum_classes)
    assert abs(crit(z, y).item() - refb.item()) <= 1e-5 * max(1.0, abs(refb.item()))
    with pytest.raises(ValueError):
        CF.binary_cross_entropy(z, y[:, :5])
    with pytest.raises(ValueError):
        CF.binary_cross_entropy(z, y, target_b=torch.zeros(9, dtype=torch.long), lam=0.5)


def test_value_errors():
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    z, t = _case()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            CF.binary_cross_entropy(z, t, label_smoothing=bad)
        with pytest.raises(ValueError):
            cdp.BinaryCrossEntropy(label_smoothing=bad)
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError):
            CF.binary_cross_entropy(z, t, target_threshold=bad)
        with pytest.raises(ValueError):
            cdp.BinaryCrossEntropy(target_threshold=bad)
    with pytest.raises(ValueError):
        CF.binary_cross_entropy(z, t, target_b=t)
    with pytest.raises(ValueError):
        CF.binary_cross_entropy(z, t, lam=0.5)
    with pytest.raises(ValueError):
        CF.binary_cross_entropy(z, t, target_b=t, lam=1.5)
    with pytest.raises(ValueError):
        CF.binary_cross_entropy(z, t, target_b=t, lam=torch.tensor([0.5, 0.5]))


def test_module_exports_and_repr():
    import cs744_distributed_data_parallel_amd as cdp

    assert cdp.BinaryCrossEntropy is cdp.ops.BinaryCrossEntropy
    assert cdp.ops.binary_cross_entropy is cdp.ops.functional.binary_cross_entropy
    assert repr(cdp.BinaryCrossEntropy()) == (
        "BinaryCrossEntropy(label_smoothing=0.0, target_threshold=None, sum_classes=False)")
    assert repr(cdp.BinaryCrossEntropy(0.1, target_threshold=0.2, sum_classes=True)) == (
        "BinaryCrossEntropy(label_smoothing=0.1, target_threshold=0.2, sum_classes=True)")


def test_cli_flags(capsys):
    from cs744_distributed_data_parallel_amd.train import parse_args

    a = parse_args([])
    assert a.loss == "ce" and a.bce_target_thresh is None and a.bce_sum_classes is False
    a = parse_args(["--loss", "bce", "--bce-target-thresh", "0.2", "--bce-sum-classes", "--label-smoothing", "0.1"])
    assert (a.loss, a.bce_target_thresh, a.bce_sum_classes, a.label_smoothing) == ("bce", 0.2, True, 0.1)
    for argv in (["--bce-target-thresh", "0.2"], ["--bce-sum-classes"], ["--loss", "ce", "--bce-sum-classes"],
                 ["--loss", "bce", "--bce-target-thresh", "1.0"], ["--loss", "hinge"]):
        with pytest.raises(SystemExit):
            parse_args(argv)
    capsys.readouterr()


def test_cli_trains_with_bce_on_the_cpu(capsys):
    """One tiny CPU epoch through the CLI with --loss bce: the reference's stdout lines, a finite test loss."""
    from cs744_distributed_data_parallel_amd.train import main

    main(["--device", "cpu", "--loss", "bce", "--bce-target-thresh", "0.2", "--label-smoothing", "0.1",
          "--mixup-alpha", "0.2", "--synthetic-size", "16", "--batch-size", "8", "--iters", "2"])
    out = capsys.readouterr().out
    assert "Training time after 1 epoch is" in out and "Test set: Average loss:" in out
