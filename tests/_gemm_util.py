"""Helpers of the conv GEMM accuracy tests: test data with structured dynamic range, fp64
references computed once per (shape, data kind), the per-element fp32 dot-product bound, and the
bookkeeping needed to force a tile / split-K plan and prove that it is the one that ran."""
import functools
import types

import torch
import torch.nn.functional as F

ENGINES = ["f16x2", "x3", "f32"]           # fp32-class engines: all meet the fp32 bound
TILES = [(64, 64), (64, 128), (128, 64), (128, 128)]
TILE_256 = (256, 128)                      # x3 family only (conv); f16x2 with Cout % 4 == 0 only (wgrad)
SPLITK_ROWS_PER_PART = 32                  # rows per BN partial of the split-K reduction (RB, conv_igemm.hip)


def lib():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


def cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def make_data(kind, shape, gen):
    t = torch.randn(shape, generator=gen, dtype=torch.float64)
    if kind == "heavy":
        t = t * torch.exp(2.0 * torch.randn(shape, generator=gen, dtype=torch.float64))
    elif kind == "image_spread":  # image n scaled by 2^(-42 n / (N-1)): the last one by 2^-42
        n = shape[0]
        t = t * torch.pow(2.0, -42.0 * torch.arange(n, dtype=torch.float64) / max(1, n - 1)).view(-1, 1, 1, 1)
    elif kind == "channel_spread":  # channel c scaled by 2^(-(3c mod 43))
        t = t * torch.pow(2.0, -((3.0 * torch.arange(shape[1], dtype=torch.float64)) % 43)).view(1, -1, 1, 1)
    elif kind == "pixel_spread":  # inside every image, all pixels but the first 2^-40 below it
        s = torch.full(shape[2:], 2.0 ** -40, dtype=torch.float64)
        s[0, 0] = 1.0
        t = t * s.view(1, 1, *shape[2:])
    return t.float()


def fp32_bound(absref, K):
    """c (2^-22 + K 2^-24) sum_i |a_i||b_i| with c = 4: the fp32 dot-product bound of length K."""
    return 4.0 * (2.0 ** -22 + K * 2.0 ** -24) * absref + 1e-300


def bf16_bound(absref, K):
    """The bf16 fast mode rounds both operands to nearest bf16 (relative 2^-9 each), so every product
    is off by at most (1 + 2^-9)^2 - 1 = 2^-8 + 2^-18; the fp32 accumulation adds the fp32 bound."""
    return (2.0 ** -8 + 2.0 ** -18) * absref + fp32_bound(absref, K)


def check_ratio(got, ref, bound):
    err = (got.double().cpu() - ref).abs()
    return (err / bound).max().item()


def check_bound(name, got, ref, absref, K, extra=None, engine=None):
    """Assert |got - ref| <= bound per element; `extra` is added to the bound (e.g. an addend's
    rounding). NaN or inf anywhere fails (the ratio is then not <= 1)."""
    bound = bf16_bound(absref, K) if engine == "bf16" else fp32_bound(absref, K)
    if extra is not None:
        bound = bound + extra
    assert got.shape == ref.shape, f"{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    ratio = check_ratio(got, ref, bound)
    assert ratio <= 1.0, f"{name}: worst |err|/bound = {ratio:.3g} (K={K})"
    return ratio


@functools.lru_cache(maxsize=None)
def conv_case(shape, kind, wide_w=False):
    """Inputs (fp32, CPU) and exact fp64 results of one conv: y, dx, dw and the sum_i |a_i||b_i| of
    each of their elements. Computed once per (shape, data kind) and shared; callers must not modify
    any of it. wide_w: the last 64 input and output channels of w are 2^6 larger than the rest, so a
    weight row's |max| sits past its first 512 entries."""
    N, Ci, H, W, Co, k, s, p = shape
    gen = torch.Generator().manual_seed(7)
    x = make_data(kind, (N, Ci, H, W), gen)
    w = (torch.randn(Co, Ci, k, k, generator=gen) * (1.0 / (Ci * k * k) ** 0.5)).float()
    if wide_w:
        w[-64:] *= 64.0
        w[:, -64:] *= 64.0
    xd, wd = x.double(), w.double()
    y = F.conv2d(xd, wd, None, s, p)
    gy = make_data(kind, tuple(y.shape), gen)
    gyd = gy.double()
    xr = xd.clone().requires_grad_()
    wr = wd.clone().requires_grad_()
    F.conv2d(xr, wr, None, s, p).backward(gyd)
    abs_y = F.conv2d(xd.abs(), wd.abs(), None, s, p)
    xa = torch.zeros_like(xd, requires_grad=True)
    F.conv2d(xa, wd.abs(), None, s, p).backward(gyd.abs())
    wa = torch.zeros_like(wd, requires_grad=True)
    F.conv2d(xd.abs(), wa, None, s, p).backward(gyd.abs())
    c = types.SimpleNamespace(shape=shape, x=x, w=w, gy=gy, y=y.detach(), abs_y=abs_y, dx=xr.grad, abs_dx=xa.grad,
                              dw=wr.grad, abs_dw=wa.grad, P=y.shape[2], Q=y.shape[3])
    # the three GEMMs as (M, N, K) of plan_info: rows, output columns, reduction length
    c.fwd_mnk = (N * c.P * c.Q, Co, k * k * Ci)
    c.dgrad_mnk = (N * H * W, Ci, k * k * Co)       # stride 1; stride 2 runs per sub-pixel class
    c.wgrad_mnk = (N * c.P * c.Q, Co, k * k * Ci)   # plan_info("wgrad", reduction rows, Cout, Kdim)
    # the bound's K per kind, as in test_accuracy_gpu.py
    c.K_fwd, c.K_dgrad, c.K_wgrad = Ci * k * k, Co * k * k, N * c.P * c.Q
    return c


@functools.lru_cache(maxsize=None)
def conv_case_gpu(shape, kind, wide_w=False):
    """channels_last device copies of conv_case's inputs (read only)."""
    c = conv_case(shape, kind, wide_w)
    return cl(c.x.cuda()), cl(c.w.cuda()), cl(c.gy.cuda())


def ktiles(K):
    return (K + 31) // 32


def conv_tiles(engine):
    return TILES + ([TILE_256] if engine != "f32" else [])


def wgrad_tiles(engine, Cout):
    return TILES + ([TILE_256] if engine == "f16x2" and Cout % 4 == 0 else [])


def conv_splits(kt, engine=None):
    """(requested, effective) split-K counts over kt K-tiles: 1, 2, a count that does not divide kt
    (4 when it does not), kt - 1 (slices of 1 and 2 K-tiles) and a request past kt (clamped to kt:
    every slice one K-tile). Requests with the same effective count are listed once."""
    odd = next((n for n in [4] + list(range(3, kt)) if n < kt and kt % n), None)
    want = [(1, 1), (2, 2), (odd, odd), (kt - 1, kt - 1), (kt + 3, kt)]
    if engine == "bf16":
        want = [(1, 1), (kt + 3, kt)]
    out, seen = [], set()
    for req, eff in want:
        if req is None or eff < 1 or eff > kt or eff in seen:
            continue
        seen.add(eff)
        out.append((req, eff))
    return out


def wgrad_splits(M, engine=None):
    """(requested, effective) split counts of the weight gradient over ceil(M / 32) row steps."""
    steps = (M + 31) // 32
    want = [(1, 1), (steps + 3, steps)] if engine == "bf16" else [(1, 1), (3, 3), (steps + 3, steps)]
    out, seen = [], set()
    for req, eff in want:
        if eff > steps or eff in seen:
            continue
        seen.add(eff)
        out.append((req, eff))
    return out


def force(L, kind, bm, bn, splits, mnk, expect):
    """Force a plan and prove it: kind is 'conv', 'dgrad' or 'wgrad' (the data gradient shares the
    conv override). The planner's answer for the GEMM about to run must be exactly `expect`."""
    L.set_gemm_override("wgrad" if kind == "wgrad" else "conv", bm, bn, splits)
    got = list(L.plan_info(kind, *mnk))
    assert got == list(expect), f"{kind} {mnk}: forced ({bm}, {bn}, {splits}) but the plan is {got}, expected {list(expect)}"


def subpixel_classes(shape):
    """(Mc, Nout, Kc) of the stride-2 data gradient's sub-pixel class GEMMs that are launched
    (conv2d_dgrad_subpixel, csrc/runtime/ops.cpp); tap-less classes launch no GEMM here (Ci % 4 == 0)."""
    N, Ci, H, W, Co, k, s, p = shape
    assert s == 2
    out = []
    for ph in range(2):
        for pw in range(2):
            Hc, Wc = (H - ph + 1) // 2, (W - pw + 1) // 2
            kh0, kw0 = (ph + p) % 2, (pw + p) % 2
            nkh = (k - kh0 + 1) // 2 if kh0 < k else 0
            nkw = (k - kw0 + 1) // 2 if kw0 < k else 0
            if Hc > 0 and Wc > 0 and nkh * nkw > 0:
                out.append((N * Hc * Wc, Ci, nkh * nkw * Co))
    return out


def merge_bn_partials(part, rpp, M):
    """Chan merge in float64 of [nparts, C, 2] (mean, M2) partials over rpp-row groups -> mean, var."""
    cnt = torch.tensor([min(rpp, M - i * rpp) for i in range(part.shape[0])], dtype=torch.float64)
    pm, pq = part[..., 0].double().cpu(), part[..., 1].double().cpu()
    mean = (cnt[:, None] * pm).sum(0) / M
    m2 = pq.sum(0) + (cnt[:, None] * (pm - mean) ** 2).sum(0)
    return mean, m2 / M
