"""The non-finite comparers of _nonfinite_util.py on hand-made cases, and the reference semantics
that test_nonfinite_gpu.py relies on, pinned in float64 torch on the CPU: ReLU and max-pool
propagate NaN, the pool's backward sends the gradient to the last NaN of the window in scan order,
and a padding above half the kernel is refused."""
import math

import pytest
import torch
import torch.nn.functional as F

from _nonfinite_util import agree_loose, agree_strict

NAN, INF = math.nan, math.inf


def t(*v):
    return torch.tensor(v, dtype=torch.float64)


# ------------------------------------------------------------------------------ comparers
def test_strict_accepts():
    agree_strict(t(1.0, NAN, INF, -INF, 0.0), t(1.0 + 1e-9, NAN, INF, -INF, 0.0), 1e-8)
    agree_strict(t(1.0, NAN).float(), t(1.0, NAN), 0.0)  # any dtype, and a zero bound holds equality
    agree_strict(torch.tensor(NAN), torch.tensor(NAN), 0.0)  # 0-dim
    agree_strict(t(2.0, NAN), t(2.0, NAN), t(0.0, NAN))  # a bound that is NaN where ref is


@pytest.mark.parametrize("got,ref,what", [
    (t(1.0, 0.0), t(1.0, NAN), "NaN missing: 1 (first at (1,)"),
    (t(NAN, NAN, 3.0), t(1.0, 2.0, 3.0), "NaN not in the reference: 2 (first at (0,)"),
    (t(1.0, -INF), t(1.0, INF), "inf differs: 1 (first at (1,)"),
    (t(1.0, 3e38), t(1.0, INF), "inf differs: 1"),
    (t(1.0, NAN), t(1.0, INF), "NaN not in the reference: 1"),
    (t(INF, 1.0), t(3e38, 1.0), "inf not in the reference: 1 (first at (0,)"),
    (t(1.0, 2.1), t(1.0, 2.0), "above the bound: 1 (first at (1,)"),
])
def test_strict_rejects(got, ref, what):
    with pytest.raises(AssertionError) as e:
        agree_strict(got, ref, 1e-3, name="case")
    assert what in str(e.value) and str(e.value).startswith("case: ")


def test_strict_reports_every_kind_and_a_2d_index():
    got = torch.tensor([[1.0, 0.0, 5.0], [NAN, -INF, 6.0]], dtype=torch.float64)
    ref = torch.tensor([[1.0, NAN, 5.5], [4.0, INF, 6.0]], dtype=torch.float64)
    with pytest.raises(AssertionError) as e:
        agree_strict(got, ref, 0.1)
    m = str(e.value)
    for part in ("NaN missing: 1 (first at (0, 1)", "NaN not in the reference: 1 (first at (1, 0)",
                 "inf differs: 1 (first at (1, 1)", "above the bound: 1 (first at (0, 2)", "of 6 elements"):
        assert part in m, m


def test_loose_accepts():
    agree_loose(t(1.0, NAN, INF, NAN, -INF), t(1.0, INF, NAN, NAN, INF), 0.0)  # NaN against inf, inf against -inf
    agree_loose(t(1.0, 2.0), t(1.0, 2.0 + 1e-9), t(0.0, 1e-8))  # per-element bound


@pytest.mark.parametrize("got,ref,what", [
    (t(1.0, 0.0), t(1.0, NAN), "non-finite missing: 1 (first at (1,)"),
    (t(1.0, 3e38), t(1.0, INF), "non-finite missing: 1"),
    (t(INF, NAN, 1.0), t(0.0, 0.0, 1.0), "non-finite not in the reference: 2 (first at (0,)"),
    (t(1.0, 2.1), t(1.0, 2.0), "above the bound: 1 (first at (1,)"),
])
def test_loose_rejects(got, ref, what):
    with pytest.raises(AssertionError) as e:
        agree_loose(got, ref, 1e-3)
    assert what in str(e.value)


def test_shape_mismatch_is_rejected():
    for f in (agree_strict, agree_loose):
        with pytest.raises(AssertionError):
            f(t(1.0, 2.0), t(1.0), 1.0)


# ------------------------------------------------------------------------------ reference semantics
def test_relu_reference():
    for relu in (torch.relu, lambda v: v.clamp_min(0.0)):  # clamp_min is what the BatchNorm references use
        r = relu(t(NAN, -INF, INF, -0.0, -1.0, 2.0))
        assert math.isnan(r[0].item())
        assert r[1].item() == 0.0 and r[2].item() == INF and r[3].item() == 0.0
        assert r[4].item() == 0.0 and r[5].item() == 2.0


@pytest.mark.parametrize("pos", range(4))
@pytest.mark.parametrize("other", [1.0, INF], ids=["finite", "inf"])
def test_max_pool_reference_returns_nan_from_any_position(pos, other):
    w = [other, 5.0, -3.0, 0.5]
    w[pos] = NAN
    if other == INF and pos == 0:
        w[1] = INF
    x = torch.tensor(w, dtype=torch.float64).view(1, 1, 2, 2)
    assert math.isnan(F.max_pool2d(x, 2).item())
    x = x.clone().requires_grad_()
    F.max_pool2d(x, 2).backward(torch.ones(1, 1, 1, 1, dtype=torch.float64))
    want = [0.0] * 4
    want[pos] = 1.0
    assert x.grad.view(-1).tolist() == want


def test_max_pool_reference_backward_takes_last_nan_and_first_maximum():
    x = torch.tensor([[1.0, NAN, 7.0], [NAN, 2.0, NAN], [0.0, 1.0, 3.0]], dtype=torch.float64).view(1, 1, 3, 3)
    x.requires_grad_()
    y = F.max_pool2d(x, 3)
    assert math.isnan(y.item())
    y.backward(torch.ones_like(y))
    g = torch.zeros(3, 3, dtype=torch.float64)
    g[1, 2] = 1.0  # NaNs at scan positions 1, 3 and 5: the last one
    assert torch.equal(x.grad.view(3, 3), g)
    e = torch.full((1, 1, 2, 2), 4.0, dtype=torch.float64, requires_grad=True)  # all equal: the first tap
    F.max_pool2d(e, 2).sum().backward()
    assert e.grad.view(-1).tolist() == [1.0, 0.0, 0.0, 0.0]


def test_max_pool_reference_overlapping_windows():
    x = torch.zeros(1, 1, 1, 5, dtype=torch.float64)
    x[0, 0, 0, 2] = NAN
    y = F.max_pool2d(x, (1, 3), (1, 1), (0, 1))  # windows over columns [w - 1, w + 1]
    assert torch.isnan(y.view(-1)).tolist() == [False, True, True, True, False]


def test_max_pool_reference_refuses_padding_above_half_the_kernel():
    x = torch.zeros(1, 1, 4, 4, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="pad should be"):
        F.max_pool2d(x, 2, 2, 2)
    F.max_pool2d(x, 2, 2, 1)
    F.max_pool2d(x, 3, 2, 1)
