"""Helpers of the stem tests (test_stem_gpu.py): mirrors of the host's path selection (stem_ok,
stem_wgrad_blocks in csrc/kernels/stem.hip; conv_bn_act_fwd / conv_bn_act_bwd in
csrc/runtime/ops.cpp), test data on top of _gemm_util.conv_case, the float64 references of the
statistics and of the weight gradient with their derived bounds, and the child process that proves
the mirrors against the launch log (CDP_GEMM_LOG=1 is read once per process).

Bounds are in units of U = 2^-23 per fp32 rounding, as in _bn_util.py."""
import functools
import json
import types

import torch
import torch.nn.functional as F

from _bn_util import (EPS, EPS32, U, _unwin, bn_bwd_grid, bwd_ref, check_db, check_out, check_sums_and_dy,
                      momentum_factor, running_ref, sum_K)
from _gemm_util import check_bound, cl, conv_case, fp32_bound, lib

CO = 64            # the stem's output channels (stem_ok)
STEM_ROWS = 256    # rows of y per workgroup of stem_fwd_kernel, and per statistics partial
# gamma_258 = 258 u / (1 - 258 u), u = 2^-24: the relative error of a 256-term fp32 sum taken in any
# order, one division and one more rounding, without fp32_bound's safety factor. It enters the
# second-order terms of the M2 bound only; every first-order term goes through fp32_bound.
GAM = 260 * 2.0 ** -24


# ------------------------------------------------------------------------------ path mirrors
def stem_ok(Cin, KH=3, KW=3, stride=1, pad=1, Co=CO):
    return 1 <= Cin <= 4 and KH == 3 and KW == 3 and stride == 1 and pad == 1 and Co == 64


def stem_fwd_taken(Cin, training=True, residual=False, lazy_res=False, defer_apply=False, **conv):
    """conv_bn_act_fwd runs stem_fwd_kernel."""
    return stem_ok(Cin, **conv) and training and not residual and not lazy_res and not defer_apply


def stem_wgrad_taken(Cin, H, W, *, need_dx, pool, relu, has_bias, training=True, C=CO, w_cin=None, zout=False):
    """conv_bn_act_bwd runs stem_wgrad_kernel<Cin>. The host writes has_bias and the even map as
    fused_db = has_bias && !(pool && (H odd || W odd))."""
    w_cin = Cin if w_cin is None else w_cin
    even = H % 2 == 0 and W % 2 == 0
    return (not need_dx and training and pool and relu and not zout and has_bias and even and C == 64
            and stem_ok(Cin, Co=C) and Cin == w_cin)


def stem_wgrad_blocks(N, H, W):
    nwin = N * (H // 2) * (W // 2)
    return max(1, min((nwin + 63) // 64, 1024))


def stem_nparts(M):
    return (M + STEM_ROWS - 1) // STEM_ROWS


# ------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def stem_case(N, Cin, H, W, kind="normal"):
    """fp32 CPU inputs of one stem case (read only): x, w and the exact float64 conv from conv_case,
    the rest from a generator of its own. kind 'large_mean': bias 1024 in every channel, and output
    channel 32 with all-zero weights (y = 1024 exactly there: variance 0)."""
    cc = conv_case((N, Cin, H, W, CO, 3, 1, 1), "normal")
    gen = torch.Generator().manual_seed(4000 + Cin + 7 * N + 13 * H + 17 * W)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    c = types.SimpleNamespace(N=N, Cin=Cin, H=H, W=W, C=CO, M=N * H * W, kind=kind, x=cc.x, w=cc.w, y0=cc.y,
                              abs_y0=cc.abs_y)
    c.bias = r(CO)
    c.gamma = 0.5 + torch.rand(CO, generator=gen)
    c.beta, c.rm, c.rv = r(CO), r(CO), 0.5 + torch.rand(CO, generator=gen)
    c.gout_seed = 5000 + Cin + 7 * N + 13 * H + 17 * W
    if kind == "large_mean":
        c.bias = torch.full((CO,), 1024.0)
        c.w = cc.w.clone()
        c.w[32] = 0.0
        c.y0, c.abs_y0 = cc.y.clone(), cc.abs_y.clone()
        c.y0[:, 32] = 0.0
        c.abs_y0[:, 32] = 0.0
    return c


def stem_gout(c, pool):
    """The gradient at the block's output (CPU, fp32); drawn per call, the same values every time."""
    gen = torch.Generator().manual_seed(c.gout_seed + (1 if pool else 0))
    shp = (c.N, CO, c.H // 2, c.W // 2) if pool else (c.N, CO, c.H, c.W)
    return torch.randn(*shp, generator=gen)


def stem_case_gpu(c):
    return types.SimpleNamespace(x=cl(c.x.cuda()), w=cl(c.w.cuda()), bias=c.bias.cuda(), gamma=c.gamma.cuda(),
                                 beta=c.beta.cuda(), rm=c.rm.cuda(), rv=c.rv.cuda())


# ------------------------------------------------------------------------------ forward
def run_stem_fwd(L, c, g, *, bias, pool, relu, state=None, momentum=0.1):
    """conv_bn_act_fwd of a stem case in training mode (the path is asserted from the mirror first)."""
    assert stem_fwd_taken(c.Cin), "the mirror says this launch does not take stem_fwd_kernel"
    rm, rv, nbt = state if state is not None else (None, None, None)
    out, y, stats, xs, _, xa, wa, rmask = L.conv_bn_act_fwd(g.x, g.w, g.bias if bias else None, g.gamma, g.beta, rm, rv,
                                                            nbt, momentum, EPS, True, 1, 1, pool, relu, None)
    # the stem path saves x as it came (no channel padding) and returns no operand maxima
    assert tuple(xs.shape) == (c.N, c.Cin, c.H, c.W) and xa is None and wa is None and rmask is None
    return types.SimpleNamespace(out=out, y=y, stats=stats, xs=xs, bias=bias, pool=pool, relu=relu)


def check_y(wst, c, r):
    """y = conv(x) + b per element: the MFMA chain of 9 Cin products started from the bias."""
    assert tuple(r.y.shape) == (c.N, CO, c.H, c.W)  # nothing past M exists
    b = c.bias.double().view(1, -1, 1, 1) if r.bias else 0.0
    ref = c.y0 + b
    absref = c.abs_y0 + (c.bias.double().abs().view(1, -1, 1, 1) if r.bias else 0.0)
    wst.items.append(("y", check_bound("y", r.y, ref, absref, 9 * c.Cin + 1)))


def stats_ref(y):
    """float64 statistics of the returned y and the bounds of what stem_fwd_kernel + the float64
    finalize make of it. Per 256-row partial b (cnt_b rows): the kernel's mean pm_b is an fp32 sum
    and a division, |pm_b - tpm_b| <= d_b = GAM sum_b |y| / cnt_b; its M2 is the fp32 sum of
    fl(fl(y - pm_b)^2), within fp32_bound(Qk_b, 258) of Qk_b = sum_b (y - pm_b)^2 = Q_b + cnt_b
    (pm_b - tpm_b)^2. The finalize merges in float64 (Chan):
        mean_k = sum_b cnt_b pm_b / M                  |mean_k - mean| <= sum_b cnt_b d_b / M
        m2_k   = sum_b [pq_b + cnt_b (pm_b - mean_k)^2]
        m2_k - M2 = sum_b (pq_b - Qk_b) + M (mean - mean_k)^2 - 2 sum_b (pm_b - mean_k) cnt_b (tpm_b - pm_b)
    (the last term is the cross term that vanishes only for exact partial means). The asserted mean
    bound is the plain fp32_bound(sum |y|, 257) / M, which is larger than sum cnt_b d_b / M.
    Returns mean, var (biased), Bmean, Bvar: the bounds before the results' own rounding to fp32."""
    yd = y.double().cpu()
    N, C, H, W = yd.shape
    M = N * H * W
    ym = yd.permute(0, 2, 3, 1).reshape(M, C)
    mean = ym.mean(0)
    M2 = ((ym - mean) ** 2).sum(0)
    nb = stem_nparts(M)
    pad = torch.zeros(nb * STEM_ROWS - M, C, dtype=torch.float64)
    blk = torch.cat([ym, pad]).view(nb, STEM_ROWS, C)
    mask = (torch.arange(nb * STEM_ROWS) < M).view(nb, STEM_ROWS, 1).double()
    cnt = mask.sum(1)                                    # [nb, 1]
    A_b = blk.abs().sum(1)                               # [nb, C]
    tpm = blk.sum(1) / cnt
    Q_b = (((blk - tpm.unsqueeze(1)) ** 2) * mask).sum(1)
    d_b = GAM * A_b / cnt
    Bm = (cnt * d_b).sum(0) / M
    Bmean = fp32_bound(ym.abs().sum(0), STEM_ROWS + 1) / M
    assert (Bm <= Bmean).all()
    BM2 = (fp32_bound(Q_b + cnt * d_b ** 2, STEM_ROWS + 2).sum(0) + M * Bm ** 2
           + 2.0 * (((tpm - mean).abs() + d_b + Bm) * cnt * d_b).sum(0))
    return mean, M2 / M, Bmean, BM2 / M


def check_stem_stats(wst, c, r, state=None, state0=None, momentum=0.1):
    """stats = (mean, invstd, scale, shift) against the float64 statistics of the returned y, the
    bounds of mean and var (stats_ref) propagated as _bn_util.check_stats_train counts the roundings:
    mean 1, invstd 1, scale 2, shift 5 on |beta| + |mean scale|. invstd = (var + eps)^-1/2 falls
    with var and is convex: the var bound moves it by at most its rise at max(var - Bvar, 0).
    With state (rm, rv, nbt after the launch; state0 = rm, rv before it): the running statistics as
    _bn_util.running_ref, the statistics' bounds scaled by the momentum factor added."""
    mean, var, Bmean, Bvar = stats_ref(r.y)
    st = r.stats.double().cpu()
    g, bt = c.gamma.double(), c.beta.double()
    invstd = 1.0 / torch.sqrt(var + EPS32)
    Dinv = 1.0 / torch.sqrt((var - Bvar).clamp_min(0.0) + EPS32) - invstd
    scale = g * invstd
    Bmean_r = Bmean + U * (mean.abs() + Bmean)
    Bscale = g.abs() * Dinv + 2 * U * g.abs() * (invstd + Dinv)
    wst.add("mean", st[0], mean, Bmean_r)
    wst.add("invstd", st[1], invstd, Dinv + U * (invstd + Dinv))
    wst.add("scale", st[2], scale, Bscale)
    wst.add("shift", st[3], bt - mean * scale,
            (mean.abs() + Bmean_r) * Bscale + scale.abs() * Bmean_r
            + 5 * U * (bt.abs() + (mean.abs() + Bmean_r) * (scale.abs() + Bscale)))
    if state is not None:
        f32 = momentum_factor(momentum, 0)
        rmr, rmb, rvr, rvb = running_ref(f32, state0[0], state0[1], mean, var, c.M)
        unb = c.M / (c.M - 1) if c.M > 1 else 1.0
        wst.add("running_mean", state[0], rmr, rmb + float(f32) * Bmean)
        wst.add("running_var", state[1], rvr, rvb + float(f32) * Bvar * unb)
        assert int(state[2].item()) == 1, "num_batches_tracked must advance by one"


def check_stem_out(wst, c, r):
    check_out(wst, r, c, r.pool, r.relu)


# ------------------------------------------------------------------------------ backward
def run_stem_bwd(L, c, g, r, gout, *, need_dx, has_bias, expect_stem):
    """conv_bn_act_bwd behind run_stem_fwd's r; the weight-gradient path is asserted from the mirror
    (expect_stem says what the case is about) before the launch."""
    taken = stem_wgrad_taken(c.Cin, c.H, c.W, need_dx=need_dx, pool=r.pool, relu=r.relu, has_bias=has_bias)
    assert taken == expect_stem, f"the mirror says stem_wgrad_kernel is {'taken' if taken else 'not taken'}"
    assert has_bias == r.bias
    res = L.conv_bn_act_bwd(cl(gout.cuda()), r.xs, g.w, r.y, r.stats, 1, 1, r.pool, r.relu, need_dx, has_bias, None,
                            True)
    dx, dw, db, dgamma, dbeta = res[:5]
    assert (dx is not None) == need_dx
    return types.SimpleNamespace(dx=dx, dw=dw, db=db, dgamma=dgamma, dbeta=dbeta, stem=taken)


def check_stem_bwd(wst, c, r, b, gout):
    """dbeta, dgamma, db at _bn_util's bounds (the statistics reduction is bn_bwd_reduce +
    chan_finalize, or the fused finalize, on every path), then dw -- and dx where it was asked for --
    against dy_ref = sc (dz - S0 / M - xhat S1 / M) correlated with x (with W) in float64:
        dw  fp32_bound(sum |dy_ref| |x|, M) + sum (dy bound) |x| + sum over ambiguous windows |sc| |g| |x|
        dx  fp32_bound(sum |dy_ref| |w|, 9 64) + the same two sums against |w|
    The dy bound is check_sums_and_dy's; the stem kernel multiplies the sums by fl(1 / M) where
    bn_bwd_apply divides: one more rounding on |k1| + |xhat k2|. An ambiguous window carries its |g|
    on all four pixels here: wherever the kernel routes it, dy differs from the reference by at
    most |sc| |g| on two of them. Returns the reference (its n_amb, n_total)."""
    pool, relu = r.pool, r.relu
    ref = bwd_ref(r.y, r.stats, gout, pool, relu)
    nparts = bn_bwd_grid(c.N, c.H, c.W, CO, pool)
    K = sum_K(ref, nparts)
    dyr, dyb, B0, B1 = check_sums_and_dy(wst, ref, None, b.dbeta, b.dgamma, K)
    check_db(wst, ref, b.db, dyr, dyb, B0, B1, K, True, r.bias, pool, nparts)
    if b.stem:
        k1, k2 = ref.S0.view(1, -1, 1, 1) / ref.M, ref.S1.view(1, -1, 1, 1) / ref.M
        dyb = dyb + U * ref.sc.abs() * (k1.abs() + (ref.xh * k2).abs())
    gd = gout.double().abs()
    gfull = _unwin(gd.unsqueeze(-1).expand(-1, -1, -1, -1, 4).contiguous(), c.H, c.W) if pool else gd
    extra = dyb + ref.amb * ref.sc.abs() * gfull
    xd = c.x.double()
    wshape = (CO, c.Cin, 3, 3)
    dwr = torch.nn.grad.conv2d_weight(xd, wshape, dyr, padding=1)
    dwb = torch.nn.grad.conv2d_weight(xd.abs(), wshape, fp32_bound(dyr.abs(), ref.M) + extra, padding=1)
    assert b.dw.is_contiguous(memory_format=torch.channels_last)
    wst.add("dw", b.dw, dwr, dwb)
    if b.dx is not None:
        wd = c.w.double()
        dxr = F.conv_transpose2d(dyr, wd, padding=1)
        dxb = F.conv_transpose2d(fp32_bound(dyr.abs(), 9 * CO) + extra, wd.abs(), padding=1)
        wst.add("dx", b.dx, dxr, dxb)
    return ref


# ------------------------------------------------------------------------------ launch-log child
# (name, (N, Cin, H, W), forward kwargs, backward kwargs or None); forward kwargs: bias, pool, relu and
# the fallbacks' training / residual; backward kwargs: need_dx
LOG_CASES = (
    [(f"stem-cin{ci}", (3, ci, 10, 6), dict(bias=True, pool=True, relu=True), dict(need_dx=False)) for ci in (1, 2, 3, 4)]
    + [("stem-tail", (1, 3, 1, 257), dict(bias=False, pool=False, relu=True), None),
       ("stem-blocks", (2, 3, 18, 14), dict(bias=True, pool=True, relu=True), dict(need_dx=False)),
       ("stem-one-window", (1, 1, 2, 2), dict(bias=True, pool=True, relu=True), dict(need_dx=False)),
       ("fwd-eval", (3, 3, 10, 6), dict(bias=True, pool=True, relu=True, training=False), None),
       ("fwd-residual", (3, 3, 10, 6), dict(bias=True, pool=False, relu=True, residual=True), None),
       ("odd-map", (2, 3, 7, 9), dict(bias=True, pool=True, relu=True), dict(need_dx=False)),
       ("no-bias", (3, 3, 10, 6), dict(bias=False, pool=True, relu=True), dict(need_dx=False)),
       ("need-dx-cin3", (3, 3, 10, 6), dict(bias=True, pool=True, relu=True), dict(need_dx=True)),
       ("need-dx-cin4", (3, 4, 10, 6), dict(bias=True, pool=True, relu=True), dict(need_dx=True)),
       ("no-relu", (3, 3, 10, 6), dict(bias=True, pool=True, relu=False), dict(need_dx=False)),
       ("no-pool", (3, 3, 10, 6), dict(bias=True, pool=False, relu=True), dict(need_dx=False))])


def log_expectation(shape, fkw, bkw):
    """What the mirrors say of one LOG_CASES entry: the stem_fwd record or None, the stem_wgrad
    record or None."""
    N, Cin, H, W = shape
    training, residual = fkw.get("training", True), fkw.get("residual", False)
    fwd = ["stem_fwd", N * H * W, CO, 9 * Cin, 256, 64, 1] if stem_fwd_taken(Cin, training, residual) else None
    wg = None
    if bkw is not None and stem_wgrad_taken(Cin, H, W, need_dx=bkw["need_dx"], pool=fkw["pool"], relu=fkw["relu"],
                                            has_bias=fkw["bias"], training=training):
        wg = ["stem_wgrad", CO, 9 * Cin, N * H * W, 64, 36, stem_wgrad_blocks(N, H, W)]
    return fwd, wg


def log_child():
    """Runs in a fresh process with CDP_GEMM_LOG=1: forward and backward of LOG_CASES, one JSON line
    of [name, forward records, backward records]."""
    L = lib()
    out = []
    for name, shape, fkw, bkw in LOG_CASES:
        c = stem_case(*shape)
        g = stem_case_gpu(c)
        training = fkw.get("training", True)
        res = cl(torch.randn(c.N, CO, c.H, c.W).cuda()) if fkw.get("residual") else None
        L.gemm_log(True)
        r = L.conv_bn_act_fwd(g.x, g.w, g.bias if fkw["bias"] else None, g.gamma, g.beta, g.rm.clone(), g.rv.clone(),
                              torch.zeros((), dtype=torch.long, device="cuda"), 0.1, EPS, training, 1, 1, fkw["pool"],
                              fkw["relu"], res)
        torch.cuda.synchronize()
        frec = [list(t) for t in L.gemm_log(True)]
        brec = None
        if bkw is not None:
            gout = cl(stem_gout(c, fkw["pool"]).cuda())
            L.conv_bn_act_bwd(gout, r[3], g.w, r[1], r[2], 1, 1, fkw["pool"], fkw["relu"], bkw["need_dx"], fkw["bias"],
                              None, training, x_amax=r[5], w_amax=r[6])
            torch.cuda.synchronize()
            brec = [list(t) for t in L.gemm_log(True)]
        out.append([name, frec, brec])
    print("STEM_LOG " + json.dumps(out))
