"""Helpers of the BatchNorm stage tests (test_bn_stages_gpu.py, test_nonfinite_gpu.py): test data, the exact pass-through
conv that hands the BatchNorm kernels a chosen input and returns their dy, mirrors of the host's
path selection (bn_bwd_grid, bn_fin_act_ok, bn_bwd_fin_apply_ok, chan_finalize_launch in
csrc/kernels/bn.hip and conv_bn_act_fwd / conv_bn_act_bwd in csrc/runtime/ops.cpp), float64
references computed on the CPU and the derived error bounds.

Every bound is in units of U = 2^-23, the issue's allowance per fp32 rounding (round to nearest is
2^-24, so one rounding uses half of it)."""
import functools
import types

import torch
import torch.nn.functional as F

from _gemm_util import cl, force, fp32_bound, lib, merge_bn_partials  # noqa: F401  (re-exported)

U = 2.0 ** -23
EPS = 1e-5
EPS32 = float(torch.tensor(EPS, dtype=torch.float32))  # what the kernels add: (float)eps
AMBIG = 2.0 ** -20      # routing decisions closer than this (relative) are not held per element
AMBIG_CAP = 1e-5        # share of a case's elements that may be excluded that way
TINY = 1e-300
FIN_MAXP, FIN_MAXP16 = 128, 512  # bn.hip
BWD_REDUCE_ROWS = 32             # RBD, bwd_fuse.hip: rows of dX per BN partial of bwd_reduce_kernel


# ------------------------------------------------------------------------------ path mirrors
def bn_bwd_grid(N, H, W, C, pool):
    """bn_bwd_grid (bn.hip): workgroups, and so partial rows, of the backward statistics reduction."""
    C4 = C // 4
    lanes = min(C4, 256)
    ppb = 256 // lanes
    npix = N * ((H // 2) * (W // 2) if pool else H * W)
    rows = (npix + ppb - 1) // ppb
    b = (rows + 1) // 2
    if b < 256:
        b = min(rows, 256)
    return max(1, min(b, 1024))


def fwd_path(nparts, C, fin_env=None, residual=False, training=True):
    """Kernels of the forward BatchNorm: bn_fin_act<64>, bn_fin_act<16>, or bn_finalize (eval:
    bn_eval_stats) followed by bn_act_fwd. fin_env is the value of CDP_BN_FIN_ACT (None: unset)."""
    if not training:
        return "eval+act"
    if fin_env != "0" and not residual and nparts <= FIN_MAXP16 and C % 64 == 0:
        return "fin_act16" if nparts > 32 else "fin_act64"
    return "finalize+act"


def act_qmode(C):
    """bn_act_fwd_launch: 1 = one channel quad per thread, 2 = two alternating quads, 0 = any C."""
    C4 = C // 4
    return 1 if C4 <= 256 and 256 % C4 == 0 else 2 if C4 == 512 else 0


def bwd_path(nparts, N, C, H, W, pool, has_bias, fin_env=None, training=True, zout=False):
    """Kernels after the backward statistics reduction: bn_bwd_fin_apply, or chan_finalize /
    chan_finalize8 followed by bn_bwd_apply. fin_env is the value of CDP_BN_BWD_FIN (None: unset)."""
    odd = pool and (H % 2 == 1 or W % 2 == 1)
    if (fin_env != "0" and training and not zout and nparts <= FIN_MAXP and C % 64 == 0 and not odd
            and (N <= 64 or fin_env == "1")):
        return "fin_apply"
    return "finalize8+apply" if C >= 256 and 512 < nparts <= 1024 else "finalize+apply"


def set_env(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


# ------------------------------------------------------------------------------ data
@functools.lru_cache(maxsize=None)
def bn_case(C, N, H, W, kind="normal"):
    """fp32 CPU inputs of one BatchNorm case (read only). kind 'large_mean': mean 1024, sigma 1 and
    one constant channel (variance 0)."""
    gen = torch.Generator().manual_seed(1000 + C + 7 * N + 13 * H + 17 * W)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    x = r(N, C, H, W)
    if kind == "large_mean":
        x = x + 1024.0
        x[:, C // 2] = 1024.0
    c = types.SimpleNamespace(C=C, N=N, H=H, W=W, M=N * H * W, kind=kind, x=x)
    c.gamma = 0.5 + torch.rand(C, generator=gen)
    c.beta, c.bias = r(C), r(C)
    c.rm, c.rv = r(C), 0.5 + torch.rand(C, generator=gen)
    c.gout = {False: r(N, C, H, W), True: r(N, C, max(1, H // 2), max(1, W // 2))}
    c.res = r(N, C, H, W)
    return c


@functools.lru_cache(maxsize=None)
def bn_case_gpu(C, N, H, W, kind="normal"):
    c = bn_case(C, N, H, W, kind)
    g = types.SimpleNamespace(x=cl(c.x.cuda()), gamma=c.gamma.cuda(), beta=c.beta.cuda(), bias=c.bias.cuda(),
                              rm=c.rm.cuda(), rv=c.rv.cuda(), res=cl(c.res.cuda()),
                              gout={k: cl(v.cuda()) for k, v in c.gout.items()})
    return g


@functools.lru_cache(maxsize=None)
def eye_w(C):
    """The identity as a 1x1 conv weight: y = x (+ b) and dx = dy exactly under the f32 engine."""
    return cl(torch.eye(C, device="cuda").view(C, C, 1, 1))


def new_state(g):
    """Fresh running statistics and num_batches_tracked of a BatchNorm2d (nonzero starting values)."""
    return g.rm.clone(), g.rv.clone(), torch.zeros((), dtype=torch.long, device="cuda")


def run_fwd(L, c, g, *, bias, pool, relu, training=True, affine=True, state=None, momentum=0.1, residual=False,
            x=None):
    """conv_bn_act_fwd through the pass-through conv under the forced 64x64 tile (one statistics
    partial per 64 rows), and the statistics partials of the same launch from conv2d_fwd."""
    M, C = c.M, c.C
    force(L, "conv", 64, 64, 1, (M, C, C), (64, 64, 1))
    w = eye_w(C)
    b = g.bias if bias else None
    xin = g.x if x is None else x
    rm, rv, nbt = state if state is not None else (None, None, None)
    out, y, stats, xs, _, xa, wa, rmask = L.conv_bn_act_fwd(
        xin, w, b, g.gamma if affine else None, g.beta if affine else None, rm, rv, nbt, momentum, EPS, training,
        1, 0, pool, relu, g.res if residual else None)
    r = types.SimpleNamespace(out=out, y=y, stats=stats, xs=xs, xa=xa, wa=wa, rmask=rmask, w=w, nparts=(M + 63) // 64)
    y2, part, rpp = L.conv2d_fwd(xin, w, b, 1, 0, True)
    assert torch.equal(y2, y), "conv2d_fwd and conv_bn_act_fwd disagree on y (same plan, same inputs)"
    assert int(rpp.item()) == 64 and tuple(part.shape) == (r.nparts, C, 2)
    r.mean, r.var = merge_bn_partials(part, 64, M)  # float64 Chan merge: mean, biased variance
    # the pass-through precondition: y is x, or fl(x + b)
    xc = (c.x if x is None else x.cpu())
    want = xc + c.bias.view(1, -1, 1, 1) if bias else xc
    assert torch.equal(y.cpu(), want), "pass-through conv: y != fl(x + b)"
    return r


def run_fwd_nonfinite(L, c, g, *, x, b, want_y, pool, relu, training=True, state=None, res=None, drop_scale=None):
    """run_fwd for inputs that hold NaN or inf (test_nonfinite_gpu.py): x, the conv bias b (or None),
    the residual res (or None) and the stochastic-depth scales are device tensors given by the caller,
    want_y (CPU) is what the pass-through conv must return for them. Through w = I an element x[n, k,
    h, w] that is not finite makes every channel of its pixel non-finite (0 * NaN and 0 * inf are
    NaN), so the precondition is not y == fl(x + b) but: NaN exactly where want_y has it, the same
    inf where want_y has one, and bit-equal values everywhere else."""
    from _nonfinite_util import agree_strict

    M, C = c.M, c.C
    force(L, "conv", 64, 64, 1, (M, C, C), (64, 64, 1))
    w = eye_w(C)
    rm, rv, nbt = state if state is not None else (None, None, None)
    kw = {} if drop_scale is None else {"drop_scale": drop_scale}
    out, y, stats, xs, _, xa, wa, rmask = L.conv_bn_act_fwd(x, w, b, g.gamma, g.beta, rm, rv, nbt, 0.1, EPS, training,
                                                            1, 0, pool, relu, res, **kw)
    r = types.SimpleNamespace(out=out, y=y, stats=stats, xs=xs, xa=xa, wa=wa, rmask=rmask, w=w, nparts=(M + 63) // 64)
    y2, part, rpp = L.conv2d_fwd(x, w, b, 1, 0, True)
    agree_strict(y, want_y, 0.0, name="pass-through conv, y against fl(x + b)")
    agree_strict(y2, want_y, 0.0, name="pass-through conv2d_fwd, y against fl(x + b)")
    assert int(rpp.item()) == 64 and tuple(part.shape) == (r.nparts, C, 2)
    r.mean, r.var = merge_bn_partials(part, 64, M)  # non-finite in the channels whose y is
    return r


_dgrad_checked = set()


def assert_dgrad_passthrough(L, c, g):
    """dx = dy exactly through the identity weight (once per shape): the block's returned dx is then
    the BatchNorm backward's dy, bit for bit."""
    key = (c.C, c.N, c.H, c.W)
    if key in _dgrad_checked:
        return
    t = g.gout[False]
    got = L.conv2d_dgrad(t, eye_w(c.C), [c.N, c.C, c.H, c.W], 1, 0)
    assert torch.equal(got, t), "pass-through conv: dgrad(dy, I) != dy"
    _dgrad_checked.add(key)


# ------------------------------------------------------------------------------ checks
def ratio(got, ref, bound):
    """max |got - ref| / bound; NaN or inf anywhere gives a ratio that is not <= 1."""
    return ((got.double().cpu() - ref).abs() / (bound + TINY)).max().item()


class Worst:
    """Collects error/bound ratios of one test, asserts each, prints the worst."""

    def __init__(self, name):
        self.name, self.items = name, []

    def add(self, what, got, ref, bound):
        assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
        r = ratio(got, ref, bound)
        self.items.append((what, r))
        return r

    def finish(self):
        print(f"\n[{self.name}] " + " ".join(f"{k}={v:.3g}" for k, v in self.items))
        bad = [(k, v) for k, v in self.items if not v <= 1.0]
        assert not bad, f"{self.name}: error/bound above 1: {bad}"
        return max(v for _, v in self.items) if self.items else 0.0


def _cv(t):
    return t.view(1, -1, 1, 1)


def check_stats_train(wst, r, c, affine=True):
    """stats = (mean, invstd, scale, shift) against the float64 merge of the launch's own partials:
    U per fp32 rounding in the quantity's formula -- mean 1, invstd 1, scale = g * invstd 2,
    shift = beta - (float)mean * scale 5 (mean 1, scale 2, product 1, difference 1), the last on
    |beta| + |mean * scale|."""
    st = r.stats.double().cpu()
    g = c.gamma.double() if affine else torch.ones(c.C, dtype=torch.float64)
    bt = c.beta.double() if affine else torch.zeros(c.C, dtype=torch.float64)
    invstd = 1.0 / torch.sqrt(r.var + EPS32)
    scale = g * invstd
    wst.add("mean", st[0], r.mean, U * r.mean.abs())
    wst.add("invstd", st[1], invstd, U * invstd)
    wst.add("scale", st[2], scale, 2 * U * scale.abs())
    wst.add("shift", st[3], bt - r.mean * scale, 5 * U * (bt.abs() + (r.mean * scale).abs()))


def check_stats_eval(wst, r, c, affine=True):
    """bn_eval_stats_kernel, all fp32: invstd = 1 / sqrtf(rv + eps) 3 roundings, scale 4,
    shift = b - rm * g * invstd 6 on |b| + |rm * scale|; mean is rm itself."""
    st = r.stats.double().cpu()
    g = c.gamma.double() if affine else torch.ones(c.C, dtype=torch.float64)
    bt = c.beta.double() if affine else torch.zeros(c.C, dtype=torch.float64)
    rm, rv = c.rm.double(), c.rv.double()
    invstd = 1.0 / torch.sqrt(rv + EPS32)
    assert torch.equal(r.stats[0].cpu(), c.rm)
    wst.add("invstd", st[1], invstd, 3 * U * invstd)
    wst.add("scale", st[2], g * invstd, 4 * U * (g * invstd).abs())
    wst.add("shift", st[3], bt - rm * g * invstd, 6 * U * (bt.abs() + (rm * g * invstd).abs()))


def check_out(wst, r, c, pool, relu, residual=False):
    """out against y and the returned stats in float64: one fmaf, one rounding; max and ReLU are
    monotone and add none. Residual: two roundings, U (|bn| + |res| + |sum|) before the ReLU, which
    does not grow an error."""
    st = r.stats.double().cpu()
    z = r.y.double().cpu() * _cv(st[2]) + _cv(st[3])
    if residual:
        res = c.res.double()
        bound = U * (z.abs() + res.abs() + (z + res).abs())
        z = z + res
    if relu:
        z = z.clamp_min(0.0)
    if pool:
        z = F.max_pool2d(z, 2)
    if not residual:
        bound = U * z.abs()
    wst.add("out", r.out, z, bound)
    return z


def running_ref(f32, rm0, rv0, mean, var, M):
    """One running-statistics update in float64 from the fp32 factor f32 (a 0-dim fp32 tensor):
    (1 - f) rm + f mean and the unbiased variance, with the bound 2^-22 (|(1 - f) rm| + |f mean|)."""
    f = float(f32)
    omf = float(torch.tensor(1.0, dtype=torch.float32) - f32)
    unb = var * M / (M - 1) if M > 1 else var
    a, b = omf * rm0.double().cpu(), f * mean
    a2, b2 = omf * rv0.double().cpu(), f * unb
    return a + b, 2.0 ** -22 * (a.abs() + b.abs()), a2 + b2, 2.0 ** -22 * (a2.abs() + b2.abs())


def momentum_factor(momentum, nbt_before):
    """The kernel's fp32 factor: momentum itself, or 1 / (count + 1) for momentum=None (passed as -1)."""
    if momentum >= 0:
        return torch.tensor(momentum, dtype=torch.float32)
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(nbt_before + 1), dtype=torch.float32)


# ------------------------------------------------------------------------------ backward reference
def _win(t):
    """[N, C, H, W] -> [N, C, H/2, W/2, 4] windows in scan order (0,0), (0,1), (1,0), (1,1)."""
    N, C, H, W = t.shape
    Ho, Wo = H // 2, W // 2
    return t[:, :, :2 * Ho, :2 * Wo].reshape(N, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, Ho, Wo, 4)


def _unwin(t, H, W):
    """Inverse of _win onto a zero [N, C, H, W] map (odd borders stay zero)."""
    N, C, Ho, Wo, _ = t.shape
    out = torch.zeros(N, C, H, W, dtype=t.dtype)
    out[:, :, :2 * Ho, :2 * Wo] = t.reshape(N, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, 2 * Ho, 2 * Wo)
    return out


def bwd_ref(y, stats, gout, pool, relu, route_from=None):
    """float64 BatchNorm backward quantities from y, the kernel's own fp32 stats and gout (all given
    as CPU tensors, converted here). Routing (ReLU, first-max-wins 2x2 pool) is decided from
    z = y * scale + shift in float64; with route_from (a residual block's output) from its sign.
    Returns dz, xhat, the per-channel sums S0 = sum dz, S1 = sum dz xhat, S2 = sum xhat, the sums of
    the terms' magnitudes A0..A2, the mask of elements whose routing is ambiguous and the slack
    (sum |g|, sum |g| |xhat| over them) that they add to the bounds of S0 and S1."""
    yd, st, gd = y.double().cpu(), stats.double().cpu(), gout.double().cpu()
    mu, is_, sc, sh = (_cv(st[i]) for i in range(4))
    N, C, H, W = yd.shape
    p = yd * sc
    z = p + sh
    xh = (yd - mu) * is_
    amb = torch.zeros_like(z, dtype=torch.bool)
    gfull = torch.zeros_like(z)  # |g| that an element's routing decides
    if route_from is not None:
        dz = torch.where(route_from.double().cpu() > 0, gd, torch.zeros_like(gd))
    elif not pool:
        dz = gd if not relu else torch.where(z > 0, gd, torch.zeros_like(gd))
        if relu:
            amb = z.abs() < AMBIG * (p.abs() + sh.abs())
        gfull = gd.abs()
    else:
        zw, pw = _win(z), _win(p)
        mx, arg = zw.max(-1)
        top = zw.topk(2, -1).values
        wamb = (top[..., 0] - top[..., 1]) < AMBIG * top[..., 0].abs()
        gg = gd
        if relu:
            gg = torch.where(mx > 0, gd, torch.zeros_like(gd))
            pmx = pw.gather(-1, arg.unsqueeze(-1)).squeeze(-1)
            wamb = wamb | (mx.abs() < AMBIG * (pmx.abs() + sh.abs()))
        dz = _unwin(F.one_hot(arg, 4).double() * gg.unsqueeze(-1), H, W)
        amb = _unwin(wamb.unsqueeze(-1).expand(-1, -1, -1, -1, 4).double(), H, W) > 0
        gfull = _unwin(gd.abs().unsqueeze(-1).expand(-1, -1, -1, -1, 4).contiguous(), H, W)
    t1 = dz * xh
    dims = (0, 2, 3)
    ref = types.SimpleNamespace(dz=dz, xh=xh, sc=sc, amb=amb, N=N, C=C, H=H, W=W, M=N * H * W, pool=pool)
    ref.S0, ref.S1, ref.S2 = dz.sum(dims), t1.sum(dims), xh.sum(dims)
    ref.A0, ref.A1, ref.A2 = dz.abs().sum(dims), t1.abs().sum(dims), xh.abs().sum(dims)
    ga = gfull * amb
    # a pooled window counts its |g| once for S0 (all four elements carry it here: 4x, an upper bound)
    ref.slack0, ref.slack1 = ga.sum(dims), (ga * xh.abs()).sum(dims)
    if pool:  # the gradient may land on any element of an ambiguous window: the window's largest |xhat|
        xm = _unwin(_win(xh.abs()).amax(-1, keepdim=True).expand(-1, -1, -1, -1, 4).contiguous(), H, W)
        ref.slack1 = (ga * xm).sum(dims)
    ref.n_amb, ref.n_total = int(amb.sum().item()), amb.numel()
    assert ref.n_amb <= AMBIG_CAP * ref.n_total, f"ambiguous routing: {ref.n_amb} of {ref.n_total} above the cap"
    return ref


def sum_K(ref, nparts):
    """Elements one partial sums in fp32: ceil(rows / nparts), x 4 under pooling."""
    rows = ref.N * ((ref.H // 2) * (ref.W // 2) if ref.pool else ref.H * ref.W)
    return -(-rows // nparts) * (4 if ref.pool else 1)


def check_sums_and_dy(wst, ref, dy, dbeta, dgamma, K, sums=None):
    """dbeta, dgamma and dy. sums = None: the kernels reduced dz themselves, and the sums are held
    to fp32_bound(sum |terms|, K) plus the ambiguous elements' slack. sums = (S0, S1, B0, B1): the
    partials were given, S their float64 sum and B its bound. dy per element:
    |sc| [2^-21 (|dz| + |k1| + |xhat k2|) + B0 / M + |xhat| B1 / M], ambiguous elements excluded."""
    if sums is None:
        S0, S1 = ref.S0, ref.S1
        B0, B1 = fp32_bound(ref.A0, K) + ref.slack0, fp32_bound(ref.A1, K) + ref.slack1
    else:
        S0, S1, B0, B1 = sums
    wst.add("dbeta", dbeta, S0, B0)
    wst.add("dgamma", dgamma, S1, B1)
    k1, k2 = _cv(S0) / ref.M, _cv(S1) / ref.M
    dyr = ref.sc * (ref.dz - k1 - ref.xh * k2)
    bound = ref.sc.abs() * (2.0 ** -21 * (ref.dz.abs() + k1.abs() + (ref.xh * k2).abs())
                            + _cv(B0) / ref.M + ref.xh.abs() * _cv(B1) / ref.M)
    got = dy.double().cpu()
    assert torch.isfinite(got).all()
    got = torch.where(ref.amb, dyr, got)
    wst.add("dy", got, dyr, bound)
    return dyr, bound, B0, B1


def split_rows(S, nparts, gen):
    """A float64 per-channel sum S [C] as nparts fp32 rows [nparts, C] of uneven size and mixed sign
    whose sum is S up to the rows' fp32 rounding."""
    C = S.shape[0]
    if nparts == 1:
        return S.float().view(1, C)
    a = torch.randn(nparts - 1, C, generator=gen, dtype=torch.float64) * torch.exp(
        torch.randn(nparts - 1, C, generator=gen, dtype=torch.float64))
    scale = S.abs() + S.abs().mean() + 1e-3
    rows = (a * scale).float()
    last = (S - rows.double().sum(0)).float().view(1, C)
    return torch.cat([rows, last], 0)
