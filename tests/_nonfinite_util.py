"""Comparers for results that may hold NaN or inf (test_nonfinite_cpu.py, test_nonfinite_gpu.py).

The contract they check (README, "Non-finite values"):
  strict  forward activations: NaN exactly where the reference has NaN, +inf / -inf exactly where
          the reference has them, every other element within the bound
  loose   statistics and gradients: finite exactly where the reference is finite (NaN against inf
          is accepted: a sum of +inf and -inf terms may come out either way in another order),
          finite elements within the bound
Both raise an AssertionError that gives the count and the first index of each kind of disagreement."""
import numpy as np
import torch


def _prep(got, ref, bound):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert tuple(got.shape) == tuple(ref.shape), f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not torch.is_tensor(bound):
        bound = torch.tensor(float(bound), dtype=torch.float64)
    # (a bound such as U |ref| is NaN or inf where ref is; it is only read where both are finite)
    return got, ref, bound.detach().double().cpu().expand_as(ref)


def _describe(kind, bad, got, ref):
    n = int(bad.sum().item())
    if n == 0:
        return None
    flat = int(torch.nonzero(bad.reshape(-1))[0].item())
    idx = tuple(int(v) for v in np.unravel_index(flat, tuple(bad.shape))) if bad.dim() else ()
    return f"{kind}: {n} (first at {idx}: got {got.reshape(-1)[flat].item()!r}, ref {ref.reshape(-1)[flat].item()!r})"


def _finish(name, kinds, got, ref):
    msgs = [m for m in (_describe(k, b, got, ref) for k, b in kinds) if m]
    assert not msgs, f"{name}: " + "; ".join(msgs) + f" of {ref.numel()} elements"


def _over(got, ref, bound, where):
    """|got - ref| > bound (or not comparable) on `where`; elements outside it are not looked at."""
    z = torch.zeros_like(ref)
    err = (torch.where(where, got, z) - torch.where(where, ref, z)).abs()
    return where & ~(err <= torch.where(where, bound, z))


def agree_strict(got, ref, bound, name="strict"):
    got, ref, bound = _prep(got, ref, bound)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    rinf = torch.isinf(ref)
    both = ~gn & ~rn
    rest = both & ~rinf & torch.isfinite(got)
    _finish(name, [("NaN missing", rn & ~gn), ("NaN not in the reference", gn & ~rn),
                   ("inf differs", both & rinf & (got != ref)),
                   ("inf not in the reference", both & ~rinf & torch.isinf(got)),
                   ("above the bound", _over(got, ref, bound, rest))], got, ref)


def agree_loose(got, ref, bound, name="loose"):
    got, ref, bound = _prep(got, ref, bound)
    gf, rf = torch.isfinite(got), torch.isfinite(ref)
    _finish(name, [("non-finite missing", ~rf & gf), ("non-finite not in the reference", rf & ~gf),
                   ("above the bound", _over(got, ref, bound, gf & rf))], got, ref)
