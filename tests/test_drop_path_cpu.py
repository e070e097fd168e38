"""Stochastic depth on the reference path: the per-block rate rule, the Python twin of the device draw
(`drop_path_scales`), the model's reference forward / backward against a hand-written loop over the blocks
in fp64, eval mode, the module's structure, `zero_init_residual` and the CLI flags."""
import io
import math
import re
from contextlib import redirect_stderr, redirect_stdout

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _cdp():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp


def _blocks(m):
    return [b for layer in (m.layer1, m.layer2, m.layer3, m.layer4) for b in layer]


def test_rates_follow_the_linear_rule():
    m = _cdp().resnet50(drop_path_rate=0.1)
    r = m.drop_path_rates
    assert len(r) == 16 and r[0] == 0.0 and r[-1] == 0.1
    steps = np.diff(np.asarray(r))
    assert np.allclose(steps, 0.1 / 15, rtol=0, atol=1e-15)
    assert _cdp().resnet18(drop_path_rate=0.0).drop_path_rates == [0.0] * 8


def test_twin_is_a_pure_function_with_distinct_draws():
    from cs744_distributed_data_parallel_amd.ops.functional import drop_path_scales

    rates = [0.5] * 6
    a = drop_path_scales(7, 3, rates, 48)
    assert a.dtype == torch.float32 and a.shape == (6, 48)
    assert torch.equal(a, drop_path_scales(7, 3, rates, 48))
    # a smaller batch or fewer blocks is a prefix: entry (i, b) depends on (seed, counter, i, b, p) alone
    assert torch.equal(a[:4, :5], drop_path_scales(7, 3, rates[:4], 5))
    # another counter, seed, block or image is another draw: at p = 0.5 two 48-image rows agree with
    # probability 2^-48
    assert not torch.equal(a, drop_path_scales(7, 4, rates, 48))
    assert not torch.equal(a, drop_path_scales(8, 3, rates, 48))
    for i in range(5):
        assert not torch.equal(a[i], a[i + 1])
    assert 0 < int((a[0] == 0).sum()) < 48  # images of one block differ
    # 64-bit keys: a seed or counter beyond 2^63 wraps like the device's unsigned arithmetic
    assert torch.equal(drop_path_scales(-1, 3, rates, 8), drop_path_scales((1 << 64) - 1, 3, rates, 8))


def test_twin_drops_at_the_rate_and_scales_exactly():
    from cs744_distributed_data_parallel_amd.ops.functional import drop_path_scales

    p = 0.2
    rows = torch.stack([drop_path_scales(11, t, [p], 64)[0] for t in range(64)])  # 64 steps x 64 images
    frac = (rows == 0).double().mean().item()
    bound = 5 * math.sqrt(p * (1 - p) / rows.numel())  # five binomial standard deviations, ~0.031
    print("dropped fraction", frac, "bound", bound)
    assert abs(frac - p) < bound
    keep = np.float32(1) / (np.float32(1) - np.float32(p))
    kept = rows[rows != 0]
    assert kept.numel() > 0 and (kept.numpy() == keep).all()
    # different rates in one table: each row has its own keep scale
    t = drop_path_scales(11, 0, [0.1, 0.25, 0.5], 64).numpy()
    for i, q in enumerate((0.1, 0.25, 0.5)):
        k = np.float32(1) / (np.float32(1) - np.float32(q))
        assert ((t[i] == 0) | (t[i] == k)).all()


def _hand_forward(m, x, table):
    """The model's training forward written out block by block, with the scales of `table` ([nb, B])."""
    rows = {i: k for k, i in enumerate(i for i, p in enumerate(m.drop_path_rates) if p > 0)}
    x = m.maxpool(F.relu(m.bn1(m.conv1(x))))
    for i, blk in enumerate(_blocks(m)):
        idt = x if blk.downsample is None else blk.downsample(x)
        out = F.relu(blk.bn1(blk.conv1(x)))
        out = blk.bn2(blk.conv2(out))
        if i in rows:
            out = out * table[rows[i]].double().view(-1, 1, 1, 1)
        x = F.relu(out + idt)
    return m.fc(torch.flatten(m.avgpool(x), 1))


def test_reference_path_matches_a_hand_composition():
    cdp = _cdp()
    torch.manual_seed(0)
    a = cdp.resnet18(num_classes=10, drop_path_rate=0.5, drop_path_seed=5, channels_last=False).double()
    b = cdp.resnet18(num_classes=10, drop_path_rate=0.5, drop_path_seed=5, channels_last=False).double()
    b.load_state_dict(a.state_dict())
    a.set_drop_path_step(3)
    x = torch.randn(2, 3, 64, 64, dtype=torch.float64)
    y = torch.tensor([1, 7])
    table = b.drop_path_schedule(3, 1, 2)[0]
    assert table.shape == (7, 2) and (table == 0).any() and (table != 0).any()
    assert int(a.drop_path_step) == 3
    out_a = a(x)
    assert int(a.drop_path_step) == 4  # one per training forward
    assert torch.equal(a.last_drop_scales, table)
    out_b = _hand_forward(b, x, table)
    assert torch.equal(out_a, out_b)
    F.cross_entropy(out_a, y).backward()
    F.cross_entropy(out_b, y).backward()
    for (n, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p.grad, q.grad, rtol=1e-12, atol=1e-14), n
    for (n, u), v in zip(a.named_buffers(), b.buffers()):
        assert torch.equal(u, v), n  # the running statistics are those of the unscaled BatchNorm
    # the first block never drops: its rate is 0 and it takes no scale
    assert a.drop_path_rates[0] == 0.0
    a.eval()
    with torch.no_grad():
        a(x)
    assert int(a.drop_path_step) == 4  # eval draws nothing


def test_eval_output_is_the_plain_models_bitwise():
    cdp = _cdp()
    torch.manual_seed(1)
    plain = cdp.resnet18(num_classes=10, channels_last=False).eval()
    dp = cdp.resnet18(num_classes=10, drop_path_rate=0.5, channels_last=False).eval()
    dp.load_state_dict(plain.state_dict())
    x = torch.randn(2, 3, 64, 64)
    with torch.no_grad():
        assert torch.equal(dp(x), plain(x))
    assert int(dp.drop_path_step) == 0 and dp.last_drop_scales is None


def test_structure_and_rate_validation():
    cdp = _cdp()
    plain = cdp.resnet18(num_classes=10)
    dp = cdp.resnet18(num_classes=10, drop_path_rate=0.3, zero_init_residual=True)
    assert list(dp.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in dp.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert [n for n, _ in dp.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert plain.drop_path_step is None and plain.last_drop_scales is None
    with pytest.raises(ValueError):
        plain.set_drop_path_step(1)
    with pytest.raises(ValueError):
        plain.drop_path_schedule(0, 1, 2)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError):
            cdp.resnet18(drop_path_rate=bad)
    # the attributes follow the module through _apply and keep their dtypes
    d = dp.double()
    assert d.drop_path_step.dtype == torch.int64 and d._dp_rates.dtype == torch.float32
    dp.set_drop_path_step(9)
    assert int(dp.drop_path_step) == 9
    assert dp.drop_path_schedule(9, 2, 3).shape == (2, 7, 3)


@pytest.mark.parametrize("name,last", [("resnet18", "bn2"), ("resnet50", "bn3")])
def test_zero_init_residual_zeroes_the_last_batchnorm_of_every_block(name, last):
    cdp = _cdp()
    torch.manual_seed(2)
    m = getattr(cdp, name)(num_classes=10, zero_init_residual=True, channels_last=False)
    zeroed = {f"{bn}.weight" for bn in (f"layer{l}.{i}.{last}" for l in range(1, 5) for i in range(len(getattr(m, f"layer{l}"))))}
    for n, p in m.named_parameters():
        if n in zeroed:
            assert (p == 0).all(), n
        elif n.endswith(".weight") and p.dim() == 1:
            assert (p == 1).all(), n  # every other BatchNorm keeps the normal initialisation
    assert zeroed <= {n for n, _ in m.named_parameters()}
    # at initialisation, in train mode, every block is its shortcut after the ReLU
    seen = []

    def hook(blk, inp, out):
        idt = inp[0] if blk.downsample is None else blk.downsample(inp[0])
        seen.append(torch.equal(out, F.relu(idt)))

    hs = [b.register_forward_hook(hook) for b in _blocks(m)]
    m.train()
    with torch.no_grad():
        m(torch.randn(2, 3, 32, 32))
    for h in hs:
        h.remove()
    assert len(seen) == len(_blocks(m)) and all(seen)


def test_train_cli_flags():
    from cs744_distributed_data_parallel_amd import train

    a = train.parse_args(["--model", "resnet18", "--drop-path", "0.05", "--zero-init-residual"])
    assert a.drop_path == 0.05 and a.zero_init_residual
    a = train.parse_args([])
    assert a.drop_path == 0.0 and not a.zero_init_residual
    for argv in (["--model", "vgg11", "--drop-path", "0.05"], ["--model", "vgg11", "--zero-init-residual"],
                 ["--model", "resnet18", "--drop-path", "1.0"]):
        with redirect_stderr(io.StringIO()), pytest.raises(SystemExit):
            train.parse_args(argv)

    def cli(extra):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(["--device", "cpu", "--model", "resnet18", "--synthetic-size", "40", "--batch-size", "2",
                        "--stored-size", "32", "--epochs", "1"] + extra)
        return out.getvalue(), err.getvalue()

    strip = lambda s: [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", ln) for ln in s.splitlines()]  # noqa: E731
    plain, perr = cli([])
    dropped, err = cli(["--drop-path", "0.5", "--zero-init-residual"])
    assert strip(plain) == strip(dropped)  # stdout keeps the reference's lines
    lines = [ln for ln in err.splitlines() if "drop path in iter" in ln]
    assert len(lines) == 1 and re.fullmatch(r"\[cdp\] rank 0: drop path in iter 20 dropped \d+ of 14 branches",
                                            lines[0]), err
    assert "drop path" not in perr and "drop path" not in dropped
