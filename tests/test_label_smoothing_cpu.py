"""Label smoothing and top-k accuracy, reference (CPU) paths: parity with ``F.cross_entropy``, the
argument checks, the rank rule of ``count_correct(topk=...)`` and the training CLI flags."""
import io
import re
from contextlib import redirect_stderr, redirect_stdout

import pytest
import torch
import torch.nn.functional as F

import cs744_distributed_data_parallel_amd as cdp
from cs744_distributed_data_parallel_amd.ops import functional as CF


def test_smoothed_loss_and_gradient_equal_torch():
    torch.manual_seed(0)
    z = (3 * torch.randn(7, 10)).requires_grad_()
    zr = z.detach().clone().requires_grad_()
    t = torch.randint(0, 10, (7,))
    ref = F.cross_entropy(zr, t, label_smoothing=0.1)
    ref.backward()
    for loss in (CF.cross_entropy(z, t, label_smoothing=0.1), cdp.CrossEntropyLoss(label_smoothing=0.1)(z, t)):
        assert torch.equal(loss, ref)
    z.grad = None
    cdp.CrossEntropyLoss(label_smoothing=0.1)(z, t).backward()
    assert torch.equal(z.grad, zr.grad)
    assert not torch.equal(ref, F.cross_entropy(zr, t))
    assert torch.equal(cdp.CrossEntropyLoss()(z, t), F.cross_entropy(zr, t))


@pytest.mark.parametrize("eps", [-0.1, 1.5])
def test_label_smoothing_outside_unit_interval_raises(eps):
    with pytest.raises(ValueError):
        cdp.CrossEntropyLoss(label_smoothing=eps)
    with pytest.raises(ValueError):
        CF.cross_entropy(torch.zeros(2, 3), torch.zeros(2, dtype=torch.long), label_smoothing=eps)


def test_extra_repr_shows_the_smoothing():
    assert "label_smoothing=0.1" in repr(cdp.CrossEntropyLoss(label_smoothing=0.1))
    assert cdp.CrossEntropyLoss().label_smoothing == 0.0
    cdp.CrossEntropyLoss(label_smoothing=0.0), cdp.CrossEntropyLoss(label_smoothing=1.0)  # the closed ends


def _rank_count(z, t, k):
    """The rank rule, row by row in plain Python."""
    n = 0
    for row, tt in zip(z.tolist(), t.tolist()):
        if not 0 <= tt < len(row) or row[tt] != row[tt]:
            continue
        rank = sum(1 for c, v in enumerate(row) if v > row[tt] or (v == row[tt] and c < tt))
        n += rank < k
    return n


def test_count_correct_topk_fallback_follows_the_rank_rule():
    torch.manual_seed(1)
    z = 3 * torch.randn(50, 10)
    z[::7] = z[::7].round()  # some ties
    t = torch.randint(0, 10, (50,))
    counts = []
    for k in (1, 2, 5, 10, 12):
        c = CF.count_correct(z, t, topk=k)
        assert c.dtype == torch.long and c.shape == (1,)
        assert int(c) == _rank_count(z, t, k)
        counts.append(int(c))
    assert counts == sorted(counts) and counts[-1] == 50 and counts[0] < counts[2]
    assert int(CF.count_correct(z, t)) == int(z.max(1)[1].eq(t).sum())
    out = torch.tensor([3])
    assert CF.count_correct(z, t, out, topk=5) is out and int(out) == 3 + counts[2]
    with pytest.raises(ValueError):
        CF.count_correct(z, t, topk=0)


def test_count_correct_topk_ties_go_to_the_lower_index():
    z = torch.zeros(4, 10)
    t = torch.tensor([0, 1, 4, 9])
    assert [int(CF.count_correct(z, t, topk=k)) for k in (1, 2, 5)] == [1, 2, 3]


def test_count_correct_topk_skips_bad_rows():
    z = torch.randn(3, 10)
    t = torch.tensor([-1, 2, 3])
    z[1, 2] = float("nan")
    z[2, 3] = 100.0
    assert int(CF.count_correct(z, t, topk=10)) == 1


def _cli(extra):
    from cs744_distributed_data_parallel_amd import train

    out, err = io.StringIO(), io.StringIO()
    with redirect_stdout(out), redirect_stderr(err):
        train.main(["--epochs", "1", "--iters", "2", "--batch-size", "8", "--synthetic-size", "80",
                    "--device", "cpu"] + extra)
    return out.getvalue(), err.getvalue()


def test_train_cli_smoothing_and_topk_keep_the_reference_lines():
    plain, plain_err = _cli([])
    smooth, err = _cli(["--label-smoothing", "0.1", "--eval-topk", "5"])
    strip = lambda s: [re.sub(r"-?\d+\.\d+(e-?\d+)?|\d+/80 \(\d+%\)", "#", ln) for ln in s.splitlines()]  # noqa: E731
    assert strip(plain) == strip(smooth)
    assert "top-" not in smooth and "top-" not in plain and "top-" not in plain_err
    m1 = re.search(r"Test set: Average loss: \d+\.\d{4}, Accuracy: (\d+)/80 \(\d+%\)", smooth)
    mk = re.findall(r"^\[cdp\] top-5 accuracy: (\d+)/80 \((\d+)%\)$", err, flags=re.M)
    assert m1 and len(mk) == 1
    assert int(mk[0][0]) >= int(m1.group(1))
    assert int(mk[0][1]) == round(100.0 * int(mk[0][0]) / 80)


def test_train_cli_eval_loss_is_unsmoothed(monkeypatch):
    """--label-smoothing reaches the training criterion only: test_model is given a plain one."""
    from cs744_distributed_data_parallel_amd import train

    seen = []
    real = train.test_model

    def spy(model, loader, criterion, **kw):
        seen.append((criterion.label_smoothing, kw.get("topk")))
        return real(model, loader, criterion, **kw)

    trained = []
    real_train = train.train_model

    def spy_train(model, loader, optimizer, criterion, *a, **kw):
        trained.append(criterion.label_smoothing)
        return real_train(model, loader, optimizer, criterion, *a, **kw)

    monkeypatch.setattr(train, "test_model", spy)
    monkeypatch.setattr(train, "train_model", spy_train)
    _cli(["--label-smoothing", "0.1", "--eval-topk", "3"])
    assert seen == [(0.0, 3)] and trained == [0.1]
