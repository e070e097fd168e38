"""NaN and inf through the forward kernels, against float64 torch (whose ops carry the semantics
pinned by test_nonfinite_cpu.py).

The contract (README, "Non-finite values"; comparers in _nonfinite_util.py)
  strict  forward activations: NaN exactly where the reference has NaN, the same inf where it has
          one, every other element within the bound the finite tests hold it to
  loose   statistics and gradients: finite exactly where the reference is finite, finite elements
          within their bound (a sum over +inf and -inf may come out NaN or inf by its order)

Parts
  BatchNorm apply   bn_fin_act<64>, bn_fin_act<16>, bn_finalize + bn_act_fwd (qmode 0, 1, 2), eval,
                    plain residual (poison in y, in the residual), stochastic depth, through the
                    pass-through harness of _bn_util.py (f32 engine, w = I, forced 64x64 tile; the
                    path asserted before the launch). Injection: a whole channel through the conv
                    bias (training), single elements of x (eval: every channel of the pixel becomes
                    non-finite through w = I). out strict at the finite tests' bound, stats and the
                    running statistics loose against the float64 statistics of y itself, clean
                    channels at check_stats_train's and running_ref's bounds; the residual pass mask
                    bit for bit; the f16x2 act max exact on the images and channels without a
                    non-finite output.
  max-pool          maxpool_fwd_kernel / maxpool_bwd_kernel at (2, 8, 9, 11), (k, s, p) = (2, 2, 0),
                    (3, 2, 1), (3, 1, 1): NaN at a first, a middle and a last tap, in border windows,
                    under overlapping windows, before and after +inf; the gradient on the last NaN.
                    (A window of these shapes has k - p = 2 rows in range at a border, never one: the
                    NaN sits in the first and in the last in-range row of a border window.)
  conv GEMMs        conv2d_fwd / dgrad / wgrad of f16x2, x3, f32 and bf16 at the planner's tile with
                    one NaN or +inf in image 0 of the activation operand: the affected outputs are
                    those whose receptive field holds it (counted), every other output meets the
                    finite bound against the unpoisoned reference.
  models            VGG-11 and ResNet-18 training steps on a batch with one NaN pixel (NaN loss,
                    non-finite running means and gradient norm, skip_nonfinite skips), VGG-11 eval
                    (NaN stays in its image), one block's backward with a poisoned gradient.

Seen on an MI355X. With relu_nan / max_nan (common.h) and the isnan term of maxpool_fwd_kernel all
222 cases pass (5 s). On the kernels from before (fmaxf ReLU and pools, `v > m` max-pool) 105 of
them fail, every one where a NaN meets a ReLU or a pool position other than the first:
  training, whole channel     every ReLU case of every apply kernel ("NaN missing", got 0.0 for the
                              whole channel); the linear cases pass, pooled ones too (all four
                              window elements are NaN, and fmaxf(NaN, NaN) is NaN)
  eval, single pixels         every ReLU case, and every pooled linear case (a window with one NaN
                              returned its largest finite value, e.g. 70.4 and 198.9 beside the 100)
  residual, stochastic depth  poison in y: all; in the residual: NaN only (+inf and -inf pass)
  act max                     its clean parts cannot be chosen, the poisoned outputs being 0
  max-pool                    all three (k, s, p): 5, 20 and 40 NaN outputs missing
  models                      VGG-11 and ResNet-18 train on with finite losses (3.10 and 2.31), eval
                              logits of the poisoned image finite
  conv GEMMs, block backward with a poisoned gradient: all pass, before as after
"""
import math

import pytest
import torch
import torch.nn.functional as F

from _bn_util import (EPS, EPS32, U, Worst, _cv, _win, act_qmode, bn_case, bn_case_gpu, check_stats_eval, cl,
                      fwd_path, lib, momentum_factor, new_state, running_ref, run_fwd_nonfinite, set_env)
from _gemm_util import bf16_bound, conv_case, conv_case_gpu, fp32_bound
from _nonfinite_util import agree_loose, agree_strict

pytestmark = pytest.mark.gpu

NAN, INF = math.nan, math.inf
S10 = (3, 10, 10)
VALS = [pytest.param(NAN, id="nan"), pytest.param(INF, id="pinf"), pytest.param(-INF, id="ninf")]
POOL_RELU = [pytest.param(p, r, id=f"{'pool' if p else 'nopool'}-{'relu' if r else 'lin'}")
             for p in (False, True) for r in (True, False)]


@pytest.fixture
def L():
    """The native library on the f32 engine; engine and both overrides restored afterwards."""
    lb = lib()
    orig = lb.get_conv_gemm()
    try:
        lb.set_conv_gemm("f32")
        yield lb
    finally:
        lb.set_conv_gemm(orig)
        lb.set_gemm_override("conv", 0, 0, 0)
        lb.set_gemm_override("wgrad", 0, 0, 0)


def _nonfinite(t):
    return ~torch.isfinite(t)


# ------------------------------------------------------------------------------ BatchNorm apply: helpers
def _bias_poison(c, g, ch, v):
    """Channel ch of y poisoned through the conv bias: x, b (device) and the expected y (CPU, fp32)."""
    b = c.bias.clone()
    b[ch] = v
    return g.x, b.cuda(), c.x + b.view(1, -1, 1, 1)


def _pixel_poison(c, pts, bias):
    """Single elements x[n, k, h, w] = v: the expected y has v in channel k of the pixel (v + b is v
    for an inf, NaN for a NaN) and NaN in its other channels (0 * v through w = I). A finite v fills
    the pixel's every channel instead (a chosen finite neighbour)."""
    x = c.x.clone()
    for n, k, h, w, v in pts:
        if math.isfinite(v):
            x[n, :, h, w] = v
    b = c.bias if bias else torch.zeros(c.C)
    want = x + b.view(1, -1, 1, 1)
    for n, k, h, w, v in pts:
        if not math.isfinite(v):
            x[n, k, h, w] = v
            want[n, :, h, w] = NAN
            want[n, k, h, w] = v
    return cl(x.cuda()), (c.bias.cuda() if bias else None), want


def _out_ref(r, pool, relu, res=None, ds=None):
    """check_out's reference and bound: float64 from the returned y and the returned fp32 stats;
    one fmaf rounding, U |ref|; with a residual U (|bn| + |res| + |sum|) before the ReLU (a
    stochastic-depth scale: |scale bn| in place of |bn|, its rounding is within the same sum)."""
    st = r.stats.double().cpu()
    z = r.y.double().cpu() * _cv(st[2]) + _cv(st[3])
    if ds is not None:
        z = z * ds.double().cpu().view(-1, 1, 1, 1)
    bound = None
    if res is not None:
        rd = res.double().cpu()
        bound = U * (z.abs() + rd.abs() + (z + rd).abs())
        z = z + rd
    if relu:
        z = z.clamp_min(0.0)
    if pool:
        z = F.max_pool2d(z, 2)
    if bound is None:
        bound = U * z.abs()
    return z, bound


def _check_stats_loose(r, c, state, rm0, rv0, poisoned):
    """stats and the running statistics against the float64 statistics of y itself in the poisoned
    channels (all non-finite there) and the merge of the launch's own partials in the clean ones, at
    check_stats_train's and running_ref's bounds."""
    C = c.C
    clean = torch.ones(C, dtype=torch.bool)
    clean[list(poisoned)] = False
    y64 = r.y.double().cpu()
    mean = torch.where(clean, r.mean, y64.mean((0, 2, 3)))
    var = torch.where(clean, r.var, y64.var((0, 2, 3), unbiased=False))
    g, bt = c.gamma.double(), c.beta.double()
    invstd = 1.0 / torch.sqrt(var + EPS32)
    scale = g * invstd
    shift = bt - mean * scale
    st = r.stats.double().cpu()
    for name, ref in (("mean", mean), ("invstd", invstd), ("scale", scale), ("shift", shift)):
        assert torch.isfinite(ref[clean]).all() and _nonfinite(ref[~clean]).all(), name
    agree_loose(st[0], mean, U * mean.abs(), "mean")
    agree_loose(st[1], invstd, U * invstd, "invstd")
    agree_loose(st[2], scale, 2 * U * scale.abs(), "scale")
    agree_loose(st[3], shift, 5 * U * (bt.abs() + (mean * scale).abs()), "shift")
    rmr, rmb, rvr, rvb = running_ref(momentum_factor(0.1, 0), rm0, rv0, mean, var, c.M)
    assert _nonfinite(rmr[~clean]).all() and _nonfinite(rvr[~clean]).all()
    agree_loose(state[0], rmr, rmb, "running_mean")
    agree_loose(state[1], rvr, rvb, "running_var")
    assert int(state[2].item()) == 1


def _train_channel(L, monkeypatch, C, shp, pool, relu, v, fin_env, path, qmode=None):
    N, H, W = shp
    set_env(monkeypatch, "CDP_BN_FIN_ACT", fin_env)
    c, g = bn_case(C, N, H, W), bn_case_gpu(C, N, H, W)
    nparts = (c.M + 63) // 64
    assert fwd_path(nparts, C, fin_env) == path
    if qmode is not None:
        assert act_qmode(C) == qmode
    ch = C // 2 + 1
    x, b, want = _bias_poison(c, g, ch, v)
    state = new_state(g)
    rm0, rv0 = state[0].clone(), state[1].clone()
    r = run_fwd_nonfinite(L, c, g, x=x, b=b, want_y=want, pool=pool, relu=relu, state=state)
    _check_stats_loose(r, c, state, rm0, rv0, [ch])
    ref, bound = _out_ref(r, pool, relu)
    # the poisoned channel's statistics are non-finite, so its every output is NaN; the others are clean
    assert torch.isnan(ref[:, ch]).all() and torch.isfinite(ref).sum().item() == ref.numel() - ref[:, ch].numel()
    agree_strict(r.out, ref, bound, "out")


@pytest.mark.parametrize("v", VALS)
@pytest.mark.parametrize("pool,relu", POOL_RELU)
def test_train_fin_act64(L, monkeypatch, pool, relu, v):
    """C = 64, 300 rows, 5 partials -> bn_fin_act<64>."""
    _train_channel(L, monkeypatch, 64, S10, pool, relu, v, None, "fin_act64")


@pytest.mark.parametrize("v", VALS)
@pytest.mark.parametrize("pool,relu", POOL_RELU)
def test_train_fin_act16(L, monkeypatch, pool, relu, v):
    """C = 128, 2,420 rows, 38 partials -> bn_fin_act<16>."""
    _train_channel(L, monkeypatch, 128, (5, 22, 22), pool, relu, v, None, "fin_act16")


@pytest.mark.parametrize("v", VALS)
@pytest.mark.parametrize("pool,relu", POOL_RELU)
@pytest.mark.parametrize("C,shp,qmode,fin_env", [(12, S10, 0, None), (96, S10, 0, None), (32, S10, 1, None),
                                                 (2048, (2, 4, 4), 2, "0")], ids=["C12", "C96", "C32", "C2048"])
def test_train_finalize_act(L, monkeypatch, C, shp, qmode, fin_env, pool, relu, v):
    """bn_finalize + bn_act_fwd in qmode 0 (C = 12, 96), 1 (C = 32) and 2 (C = 2048, forced with
    CDP_BN_FIN_ACT=0, where the fused kernel would run)."""
    _train_channel(L, monkeypatch, C, shp, pool, relu, v, fin_env, "finalize+act", qmode)


# ------------------------------------------------------------------------------ BatchNorm apply: eval
def _eval_points(C, v):
    """Poisoned elements of a (3, C, 10, 10) input: v at each of the four positions of a 2x2 window
    (four windows), a finite 100 beside the first (larger than every clean value), and +inf in
    another channel beside two of them, once after the poisoned pixel in scan order and once before
    it (in that channel the poisoned pixel is NaN)."""
    k, k2 = 1, C - 2
    return k, k2, [(0, k, 1, 0, 100.0),                       # finite neighbour of the first window, position (1, 0)
                   (0, k, 0, 0, v), (0, k, 0, 3, v), (0, k, 3, 4, v), (1, k, 5, 7, v),  # positions (0,0) (0,1) (1,0) (1,1)
                   (0, k2, 3, 5, INF),                        # +inf after the NaN of window (1, 2) of image 0
                   (1, k2, 4, 6, INF)]                        # +inf before the NaN of window (2, 3) of image 1


@pytest.mark.parametrize("v", VALS)
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("pool,relu", POOL_RELU)
@pytest.mark.parametrize("C", [64, 12])
def test_eval_single_pixels(L, C, pool, relu, bias, v):
    """bn_eval_stats + bn_act_fwd (qmode 1 and 0). The statistics do not depend on y, so the poison
    stays in its pixels: NaN at every window position, beside a larger finite value, before and
    after +inf; -inf through the ReLU is exactly 0 and pools to a finite value."""
    c, g = bn_case(C, *S10), bn_case_gpu(C, *S10)
    assert fwd_path(5, C, None, training=False) == "eval+act"
    k, k2, pts = _eval_points(C, v)
    x, b, want = _pixel_poison(c, pts, bias)
    # the injected pattern, read off the expected y
    nanw, infw = _win(torch.isnan(want).double()), _win((want == INF).double())
    for pos in range(4):
        assert ((nanw[..., pos] == 1) & (nanw.sum(-1) == 1)).any(), f"no window with its only NaN at position {pos}"
    # window (0, 0) of image 0, a channel other than k: NaN at (0, 0), beside it a value above every clean one
    assert math.isnan(want[0, 0, 0, 0].item()) and want[0, 0, 1, 0].item() > (c.x.abs().max() + c.bias.abs().max()).item()
    both = (nanw.sum(-1) >= 1) & (infw.sum(-1) >= 1)
    first_nan = torch.where(nanw == 1, torch.arange(4.0), torch.full((4,), 9.0)).amin(-1)
    first_inf = torch.where(infw == 1, torch.arange(4.0), torch.full((4,), 9.0)).amin(-1)
    assert (both & (first_nan < first_inf)).any() and (both & (first_inf < first_nan)).any()
    state = new_state(g)
    r = run_fwd_nonfinite(L, c, g, x=x, b=b, want_y=want, pool=pool, relu=relu, training=False, state=state)
    wst = Worst("eval")
    check_stats_eval(wst, r, c)
    wst.finish()
    assert torch.equal(state[0], g.rm) and torch.equal(state[1], g.rv) and int(state[2].item()) == 0
    ref, bound = _out_ref(r, pool, relu)
    agree_strict(r.out, ref, bound, "out")
    out = r.out.cpu()
    # what must be non-finite is: every poisoned pixel's (window's) every channel but, for an inf, its own
    n_bad = _nonfinite(ref).sum().item()
    assert n_bad >= 4 * (C - 1), n_bad
    if v == -INF:  # (gamma > 0, so the scale is positive and z = -inf)
        if relu and not pool:
            for n, kk, h, w, _ in pts[1:5]:
                assert out[n, kk, h, w].item() == 0.0 and not math.copysign(1.0, out[n, kk, h, w].item()) < 0
        if pool:  # window (0, 0) of image 0 holds -inf (or its ReLU's 0) and three finite values
            assert math.isfinite(out[0, k, 0, 0].item())
            if relu:
                assert out[0, k, 0, 0].item() > 0.0  # the finite 100 of the same window


# ------------------------------------------------------------------------------ BatchNorm apply: residual
def _rmask_check(r, C):
    if r.rmask is not None:  # CDP_RES_MASK is read once per process
        o = (r.out.permute(0, 2, 3, 1).reshape(-1, C // 4, 4) > 0).to(torch.int32)
        want = (o * torch.tensor([1, 2, 4, 8], device=o.device, dtype=torch.int32)).sum(-1).to(torch.uint8).reshape(-1)
        assert torch.equal(r.rmask.reshape(-1), want), "rmask disagrees with out > 0"


@pytest.mark.parametrize("v", VALS)
@pytest.mark.parametrize("where", ["y", "res"])
@pytest.mark.parametrize("C", [64, 96])
def test_residual(L, monkeypatch, C, where, v):
    """Plain residual block (bn_finalize + bn_act_fwd, unpooled, ReLU, pass mask): the poison in y
    (a whole channel, through the bias) or in single elements of the residual."""
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    c, g = bn_case(C, *S10), bn_case_gpu(C, *S10)
    assert fwd_path(5, C, None, residual=True) == "finalize+act"
    state = new_state(g)
    rm0, rv0 = state[0].clone(), state[1].clone()
    if where == "y":
        ch = C // 2 + 1
        x, b, want = _bias_poison(c, g, ch, v)
        res = g.res
        poisoned = [ch]
    else:
        x, b, want = g.x, g.bias, c.x + c.bias.view(1, -1, 1, 1)
        rs = c.res.clone()
        spots = [(0, 0, 0, 0), (1, C // 2, 4, 7), (2, C - 1, 9, 9), (2, 5, 9, 0)]
        for s in spots:
            rs[s] = v
        res = cl(rs.cuda())
        poisoned = []
    r = run_fwd_nonfinite(L, c, g, x=x, b=b, want_y=want, pool=False, relu=True, state=state, res=res)
    _check_stats_loose(r, c, state, rm0, rv0, poisoned)
    ref, bound = _out_ref(r, False, True, res=res)
    agree_strict(r.out, ref, bound, "out")
    _rmask_check(r, C)
    if where == "res":
        got = [r.out[s].item() for s in spots]
        if v == -INF:
            assert got == [0.0] * 4
        elif v == INF:
            assert got == [INF] * 4
        else:
            assert all(math.isnan(t) for t in got)
        assert _nonfinite(ref).sum().item() == (0 if v == -INF else 4)


@pytest.mark.parametrize("v", VALS)
def test_stochastic_depth_dropped_image_keeps_the_nan(L, monkeypatch, v):
    """drop_scale = (0, 1.25, 0): in the dropped images the branch is 0 * bn(y), which is NaN where
    bn(y) is not finite (as in torch), so the poisoned channel is NaN in every image and the others are
    the shortcut."""
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    C = 64
    c, g = bn_case(C, *S10), bn_case_gpu(C, *S10)
    ch = 7
    x, b, want = _bias_poison(c, g, ch, v)
    ds = torch.tensor([0.0, 1.25, 0.0], device="cuda")
    state = new_state(g)
    rm0, rv0 = state[0].clone(), state[1].clone()
    r = run_fwd_nonfinite(L, c, g, x=x, b=b, want_y=want, pool=False, relu=True, state=state, res=g.res, drop_scale=ds)
    _check_stats_loose(r, c, state, rm0, rv0, [ch])
    ref, bound = _out_ref(r, False, True, res=g.res, ds=ds)
    assert torch.isnan(ref[:, ch]).all() and _nonfinite(ref).sum().item() == ref[:, ch].numel()
    agree_strict(r.out, ref, bound, "out")
    _rmask_check(r, C)
    clean = [k for k in range(C) if k != ch]
    for img in (0, 2):
        assert torch.equal(r.out[img, clean], F.relu(g.res[img, clean]))


# ------------------------------------------------------------------------------ act max (f16x2)
@pytest.mark.parametrize("v", [pytest.param(NAN, id="nan"), pytest.param(INF, id="pinf")])
@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("Co", [64, 96], ids=["fin_act", "qmode0"])
@pytest.mark.parametrize("mode", ["train-channel", "eval-pixel"])
def test_act_max_exact_on_clean_parts(mode, Co, pool, v):
    """f16x2 engine, a real 3x3 conv: the block's returned per-image / per-channel |max| equals the
    maxima of out, bit for bit, for the images and channels that hold no non-finite output."""
    lb = lib()
    orig = lb.get_conv_gemm()
    try:
        lb.set_conv_gemm("f16x2")
        K = lb.act_max_copies()
        N, HW = 4, 8
        gen = torch.Generator().manual_seed(Co + pool)
        x = torch.randn(N, 64, HW, HW, generator=gen)
        w = cl((torch.randn(Co, 64, 3, 3, generator=gen) * 0.05).cuda())
        b = torch.randn(Co, generator=gen)
        gm, be = (torch.rand(Co, generator=gen) + 0.5).cuda(), torch.randn(Co, generator=gen).cuda()
        training = mode == "train-channel"
        if training:
            b[3] = v
            rm = rv = nbt = None
        else:
            x[0, 5, 3, 4] = v
            rm, rv = torch.randn(Co, generator=gen).cuda(), (torch.rand(Co, generator=gen) + 0.5).cuda()
            nbt = torch.zeros((), dtype=torch.long, device="cuda")
        out, _, _, _, amax, _, _, _ = lb.conv_bn_act_fwd(cl(x.cuda()), w, b.cuda(), gm, be, rm, rv, nbt, 0.1, EPS,
                                                         training, 1, 1, pool, True, None)
        torch.cuda.synchronize()
    finally:
        lb.set_conv_gemm(orig)
    bad = _nonfinite(out)
    img_clean, ch_clean = ~bad.any(1).any(1).any(1), ~bad.any(0).any(1).any(1)
    if training:
        assert ch_clean.sum().item() == Co - 1 and not ch_clean[3] and not img_clean.any()
    else:
        assert img_clean.tolist() == [False, True, True, True]
    img = amax[:N].view(torch.float32)
    chm = amax[N:N + K * Co].view(torch.float32).view(K, Co).amax(0)
    assert torch.equal(img[img_clean], out.abs().amax(dim=(1, 2, 3))[img_clean])
    assert torch.equal(chm[ch_clean], out.abs().amax(dim=(0, 2, 3))[ch_clean])


# ------------------------------------------------------------------------------ standalone max-pool
def _rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


def _pool_input(k, s, p):
    """(2, 8, 9, 11) with one placement per (image, channel) plane; a window (ho, wo) has its tap
    (dh, dw) at input (ho s - p + dh, wo s - p + dw)."""
    N, C, H, W = 2, 8, 9, 11
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(11 + k + s + p))
    at = lambda ho, wo, dh, dw: (ho * s - p + dh, wo * s - p + dw)  # noqa: E731
    mid = (0, 1) if k == 2 else (1, 1)
    x[(0, 0) + at(1, 1, 0, 0)] = NAN                      # first tap
    x[(0, 1) + at(2, 3, *mid)] = NAN                      # a middle tap
    x[(0, 2) + at(1, 2, k - 1, k - 1)] = NAN              # last tap
    x[(0, 3) + at(0, 0, p, p)] = NAN                      # border window (p > 0): its first in-range row and column
    x[0, 4, (Ho - 1) * s - p + min(k - 1, H - 1 - ((Ho - 1) * s - p)), 2] = NAN  # last window row's last in-range row
    x[0, 5, 3, 5] = NAN                                   # interior: under every window that overlaps it
    h, w = at(1, 1, 0, 0)                                 # two NaNs in one window: the gradient takes the last
    x[0, 6, h, w] = NAN
    x[0, 6, h + k - 1, w + k - 2] = NAN
    x[0, 7, h, w] = INF                                   # +inf, then NaN
    x[0, 7, h, w + 1] = NAN
    x[1, 0, h, w] = NAN                                   # NaN, then +inf
    x[1, 0, h + k - 1, w + k - 1] = INF
    x[1, 1] = 0.25                                        # all-equal windows: the first tap takes the gradient
    x[1, 2, h, w + 1] = -INF                              # -inf is a value like another
    return x, (Ho, Wo)


@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (3, 2, 1), (3, 1, 1)])
def test_max_pool_forward_and_backward(k, s, p):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    x, (Ho, Wo) = _pool_input(k, s, p)
    xn = cl(x.cuda()).requires_grad_()
    xr = x.double().requires_grad_()
    y = CF.max_pool2d(xn, k, s, p)
    ref = F.max_pool2d(xr, k, s, p)
    assert tuple(y.shape) == (2, 8, Ho, Wo)
    nan_out = torch.isnan(ref.detach())
    per_plane = nan_out.sum((2, 3))
    assert (per_plane[0] >= 1).all() and per_plane[1, 0] >= 1 and per_plane[1, 1:].sum() == 0
    if s < k:  # the interior NaN sits under several windows
        assert per_plane[0, 5].item() == (4 if s == 2 else 9)
    agree_strict(y, ref.detach(), 0.0, "max-pool forward")  # a maximum rounds nothing
    gen = torch.Generator().manual_seed(5)
    gy = torch.randn(tuple(y.shape), generator=gen)
    y.backward(cl(gy.cuda()))
    ref.backward(gy.double())
    assert torch.isfinite(xr.grad).all()
    assert _rel_err(xn.grad, xr.grad) < 1e-6
    # the plane with two NaNs in its first window: all of that window's gradient is on the later one
    h, w = 1 * s - p, 1 * s - p
    assert xr.grad[0, 6, h, w].item() == 0.0 or s < k
    assert xn.grad[0, 6, h + k - 1, w + k - 2].item() != 0.0
    # all-equal plane: the gradient is where torch puts it (first tap), nowhere else
    assert torch.equal(xn.grad[1, 1].cpu() != 0, xr.grad[1, 1] != 0)


def test_max_pool_refuses_padding_above_half_the_kernel():
    """A window could lie entirely in the padding and would have no tap to return; ATen refuses the
    same (test_nonfinite_cpu.py)."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    x = cl(torch.randn(2, 8, 9, 11, device="cuda"))
    for k, s, p in [(2, 2, 2), (3, 2, 2), (3, 1, 3)]:
        with pytest.raises(RuntimeError, match="pad should be"):
            lib().maxpool2d_fwd(x, k, s, p)
        with pytest.raises(RuntimeError, match="pad should be"):
            CF.max_pool2d(x, k, s, p)
    lib().maxpool2d_fwd(x, 2, 2, 1)
    lib().maxpool2d_fwd(x, 3, 2, 1)


# ------------------------------------------------------------------------------ conv GEMMs
S2 = (2, 12, 11, 13, 20, 3, 1, 1)
S3 = (2, 7, 9, 9, 10, 3, 1, 1)


@pytest.fixture
def Lany():
    lb = lib()
    orig = lb.get_conv_gemm()
    try:
        yield lb
    finally:
        lb.set_conv_gemm(orig)


def _span(i, n):
    """Outputs of a 3x3, stride 1, pad 1 conv (or of its transpose) that read input index i of n."""
    return [j for j in (i - 1, i, i + 1) if 0 <= j < n]


@pytest.mark.parametrize("v", [pytest.param(NAN, id="nan"), pytest.param(INF, id="pinf")])
@pytest.mark.parametrize("op", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("engine", ["f16x2", "x3", "f32", "bf16"])
@pytest.mark.parametrize("sid,shape", [("S2", S2), ("S3", S3)])
def test_gemm_with_one_poisoned_activation(Lany, sid, shape, engine, op, v):
    """One element of image 0 of the activation operand (x for the forward and the weight gradient,
    dy for the data gradient) is NaN or +inf, on the top border row. The outputs whose receptive field
    holds it are non-finite, as in float64, and are counted; all others meet the finite bound against
    the unpoisoned float64 reference. Only f16x2 with inf may leave clean outputs unheld: the
    poisoned image's (weight gradient: channel's) |max| is inf, its scale falls back to 1, so image 0
    (the channel's slice of dw) is not held; with NaN nothing is left out."""
    N, Ci, H, W, Co, k, s, p = shape
    c = conv_case(shape, "normal")
    xc, wc, gyc = conv_case_gpu(shape, "normal")
    L = Lany
    L.set_conv_gemm(engine)
    wd = c.w.double()
    h0, w0, chan = 0, 5, 3
    if op == "fwd":
        xp = c.x.clone()
        xp[0, chan, h0, w0] = v
        got = L.conv2d_fwd(cl(xp.cuda()), wc, None, 1, 1, False)[0]
        refp = F.conv2d(xp.double(), wd, None, 1, 1)
        ref, absref, K = c.y, c.abs_y, c.K_fwd
        count = len(_span(h0, H)) * len(_span(w0, W)) * Co
        own = torch.zeros_like(ref, dtype=torch.bool)
        own[0] = True
    elif op == "dgrad":
        gp = c.gy.clone()
        gp[0, chan, h0, w0] = v
        got = L.conv2d_dgrad(cl(gp.cuda()), wc, list(c.x.shape), 1, 1)
        refp = torch.nn.grad.conv2d_input(list(c.x.shape), wd, gp.double(), 1, 1)
        ref, absref, K = c.dx, c.abs_dx, c.K_dgrad
        count = len(_span(h0, H)) * len(_span(w0, W)) * Ci
        own = torch.zeros_like(ref, dtype=torch.bool)
        own[0] = True
    else:
        xp = c.x.clone()
        xp[0, chan, h0, w0] = v
        got = L.conv2d_wgrad(gyc, cl(xp.cuda()), list(c.w.shape), 1, 1)
        refp = torch.nn.grad.conv2d_weight(xp.double(), list(c.w.shape), c.gy.double(), 1, 1)
        ref, absref, K = c.dw, c.abs_dw, c.K_wgrad
        # tap (kh, kw) reads x[h0, w0] for the output pixel (h0 - kh + 1, w0 - kw + 1)
        count = sum(1 for kh in range(3) for kw in range(3) if 0 <= h0 - kh + 1 < c.P and 0 <= w0 - kw + 1 < c.Q) * Co
        own = torch.zeros_like(ref, dtype=torch.bool)
        own[:, chan] = True
    affected = _nonfinite(refp)
    assert affected.sum().item() == count and (affected & ~own).sum().item() == 0
    g = got.double().cpu()
    assert tuple(g.shape) == tuple(ref.shape)
    agree_loose(g[affected], refp[affected], 0.0, f"{op}: affected outputs")
    unheld = own & ~affected if (engine == "f16x2" and v == INF) else torch.zeros_like(own)
    held = ~affected & ~unheld
    if engine == "f16x2" and v == INF:
        assert held.sum().item() == ref.numel() - own.sum().item()
    else:
        assert held.sum().item() == ref.numel() - count
    bound = bf16_bound(absref, K) if engine == "bf16" else fp32_bound(absref, K)
    agree_loose(g[held], ref[held], bound[held], f"{op}: clean outputs")
    assert torch.isfinite(g[held]).all()


# ------------------------------------------------------------------------------ models
def _bns(m):
    return [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)]


def _training_step_on_a_nan_pixel(make, x, y):
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(0)
    ref = make(channels_last=False)  # the torch backend on the CPU: what "NaN is expected" means
    model = make().cuda()
    model.load_state_dict({k: v.cuda() for k, v in ref.state_dict().items()})
    loss_r = F.cross_entropy(ref(x), y)
    loss_r.backward()
    assert math.isnan(loss_r.item())
    assert len(_bns(ref)) >= 8 and all(_nonfinite(b.running_mean).all() for b in _bns(ref))
    assert not math.isfinite(torch.cat([p.grad.reshape(-1) for p in ref.parameters()]).norm().item())

    opt = cdp.SGD(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4, skip_nonfinite=True)
    before = [p.detach().clone() for p in model.parameters()]
    opt.zero_grad()
    loss = cdp.CrossEntropyLoss()(model(x.cuda()), y.cuda())
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert math.isnan(loss.item()), loss.item()
    finite_rm = [i for i, b in enumerate(_bns(model)) if not _nonfinite(b.running_mean).all()]
    assert len(_bns(model)) == len(_bns(ref)) and not finite_rm, f"BatchNorms with a finite running_mean: {finite_rm}"
    assert not math.isfinite(float(opt.grad_norm))
    assert int(opt.skipped_steps) == 1
    for (n, p), b in zip(model.named_parameters(), before):
        assert torch.equal(p.detach(), b), n


def test_vgg11_training_step_on_a_nan_pixel():
    import cs744_distributed_data_parallel_amd as cdp

    gen = torch.Generator().manual_seed(3)
    x = torch.randn(4, 3, 32, 32, generator=gen)
    x[2, 1, 13, 20] = NAN
    _training_step_on_a_nan_pixel(cdp.VGG11, x, torch.randint(0, 10, (4,), generator=gen))


def test_resnet18_training_step_on_a_nan_pixel():
    """Basic blocks: the stem's standalone max-pool and the residual ReLU carry the NaN."""
    import cs744_distributed_data_parallel_amd as cdp

    gen = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 64, 64, generator=gen)
    x[1, 0, 30, 41] = NAN
    _training_step_on_a_nan_pixel(lambda **kw: cdp.resnet18(num_classes=10, **kw), x,
                                  torch.randint(0, 10, (2,), generator=gen))


def test_vgg11_eval_nan_stays_in_its_image():
    """Eval mode with clean BatchNorm statistics (one clean training forward) and a NaN pixel in
    image 0: its logits are all NaN, the other images' logits are those of the clean batch within
    test_vgg11_eval_matches_reference's tolerance. On an MI355X (f16x2 engine) they were bitwise
    equal: every forward scale is per image, and no kernel mixes images in eval mode."""
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    gen = torch.Generator().manual_seed(8)
    model(torch.randn(16, 3, 32, 32, generator=gen).cuda())
    model.eval()
    assert all(torch.isfinite(b.running_mean).all() and torch.isfinite(b.running_var).all() for b in _bns(model))
    x = torch.randn(4, 3, 32, 32, generator=gen)
    xp = x.clone()
    xp[0, 2, 16, 15] = NAN
    with torch.no_grad():
        clean = model(x.cuda()).double().cpu()
        got = model(xp.cuda()).double().cpu()
    assert torch.isfinite(clean).all()
    assert torch.isnan(got[0]).all(), got[0]
    assert torch.isfinite(got[1:]).all()
    d = (got[1:] - clean[1:]).abs().max().item()
    print(f"\n[vgg11 eval] images 1-3 against the clean forward: max |diff| = {d:.3g}, "
          f"bitwise equal: {torch.equal(got[1:], clean[1:])}")
    assert d < 1e-3 * clean.abs().max().item()


def _pair(ci, co, gen):
    conv = torch.nn.Conv2d(ci, co, 3, 1, 1, bias=True)
    bn = torch.nn.BatchNorm2d(co)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(co, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(co, generator=gen) * 0.5)
        bn.running_mean.copy_(torch.randn(co, generator=gen) * 0.3)
        bn.running_var.copy_(torch.rand(co, generator=gen) + 0.5)
    return conv, bn


GRAD_TOL = 5e-4  # of the tensor's largest finite reference value: the block gradients' tolerance in test_drop_path_gpu.py


@pytest.mark.parametrize("v", [pytest.param(NAN, id="nan"), pytest.param(INF, id="pinf")])
@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("engine", ["f32", "f16x2"])
def test_block_backward_with_a_poisoned_gradient(Lany, engine, training, pool, v):
    """conv_bn_act_bwd of a finite forward (3x3 conv 16 -> 32, BatchNorm, ReLU, [pool]) with one NaN
    or +inf in gout, against torch autograd in float64. Training: the element's channel loses its
    sums, so its whole dy is non-finite. Eval: the BatchNorm is a fixed affine map and the poison goes
    only where the routing sends it -- one element of dz, its 3x3 neighbourhood of dx, its channel's
    row of dw, dgamma and dbeta."""
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    Lany.set_conv_gemm(engine)
    Ci, Co, N, H, W = 16, 32, 2, 8, 8
    gen = torch.Generator().manual_seed(21)
    conv_r, bn_r = _pair(Ci, Co, gen)
    conv_r, bn_r = conv_r.double(), bn_r.double()
    conv, bn = _pair(Ci, Co, gen)
    conv.load_state_dict(conv_r.state_dict())
    bn.load_state_dict(bn_r.state_dict())
    conv, bn = conv.float().cuda(), bn.float().cuda()
    conv.weight.data = cl(conv.weight.data)
    bn.train(training)
    bn_r.train(training)
    x = torch.randn(N, Ci, H, W, generator=gen)
    xn = cl(x.cuda()).requires_grad_()
    xr = x.double().requires_grad_()
    out = CF.conv_bn_act(xn, conv, bn, relu=True, pool=pool)
    z = F.relu(bn_r(conv_r(xr)))
    z.retain_grad()
    ref = F.max_pool2d(z, 2) if pool else z
    assert torch.isfinite(out).all()
    # a gradient element whose output is well above 0 (its ReLU passes in fp32 as in float64)
    cand = (ref.detach() > 0.25).nonzero()
    n, ch, ho, wo = (int(t) for t in cand[len(cand) // 2])
    gout = torch.randn(tuple(ref.shape), generator=gen)
    gout[n, ch, ho, wo] = v
    out.backward(cl(gout.cuda()))
    ref.backward(gout.double())
    pairs = {"dx": (xn.grad, xr.grad), "dw": (conv.weight.grad, conv_r.weight.grad),
             "dgamma": (bn.weight.grad, bn_r.weight.grad), "dbeta": (bn.bias.grad, bn_r.bias.grad)}
    routed = _nonfinite(z.grad)  # the gradient behind the pool, before the ReLU and the BatchNorm
    assert routed.sum().item() == 1 and routed[n, ch].any()
    if training:
        assert _nonfinite(xr.grad).all()
    else:
        _, _, h, w = (int(t) for t in routed.nonzero()[0])
        assert _nonfinite(xr.grad).sum().item() == len(_span(h, H)) * len(_span(w, W)) * Ci
        assert _nonfinite(xr.grad[1 - n]).sum().item() == 0
    for name in ("dw", "dgamma", "dbeta"):  # both modes: only the element's channel
        bad = _nonfinite(pairs[name][1])
        assert bad[ch].any() and bad.sum().item() == bad[ch].sum().item(), name
    for name, (got, want) in pairs.items():
        fin = torch.isfinite(want)
        scale = want[fin].abs().max().item() if fin.any() else 0.0
        agree_loose(got, want, GRAD_TOL * scale, name)
