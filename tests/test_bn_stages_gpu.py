"""Each BatchNorm kernel of csrc/kernels/bn.hip, and the BatchNorm job of bwd_fuse.hip, against
float64 through the fused block ops (conv_bn_act_fwd / conv_bn_act_bwd), one stage at a time.

Method (tests/_bn_util.py). The conv of the block is an exact pass-through: f32 engine, 1x1,
w = I, so y = x (or fl(x + b)) and dx = dy bit for bit -- both asserted. That gives full control of
the BatchNorm input and exposes dy. Forward references come from the returned y and the statistics
partials of the same launch (conv2d_fwd under the same forced 64x64 tile, one partial per 64 rows);
backward references from y, the kernel's own fp32 stats and gout. Partial counts are forced through
the tile (forward), predicted by a mirror of bn_bwd_grid (backward) or given as part_in, and every
test asserts the kernels it is about from those counts before it launches.

Covered paths
  forward   bn_fin_act<64> (<= 32 partials), bn_fin_act<16> (33..512, the 512 edge), bn_finalize
            (one batch, and the looped batch past 2,048 partials) + bn_act_fwd in qmode 0, 1 and 2,
            pooled and unpooled, C / 4 > 256, the 513-partial edge, large mean with a constant
            channel, eval statistics, affine=False, track_running_stats=False, plain residual with
            its ReLU pass mask, momentum=None (cumulative average)
  backward  bn_bwd_reduce (PS 2 and 3, pooled and unpooled, one to four channel-quad passes),
            bn_bwd_fin_apply, chan_finalize (batch and tail loop), chan_finalize8 (with a channel
            tail), bn_bwd_apply (odd pooled border, separate bias pass, residual by output and by
            mask, dres), eval backward (dbmode 2), bwd_reduce_kernel's BN partials (pooled and
            unpooled, PS 2 and 3, with and without ReLU, dgrad splits 1 -- in place -- and 3)
Left out: the stem kernels, stochastic depth and the deferred downsample BatchNorm (own tests),
act-max values (own tests), timing.

Bounds (U = 2^-23 per fp32 rounding; derived, see _bn_util.py)
  stats     mean U, invstd U, scale 2 U, shift 5 U (|beta| + |mean scale|); eval: 3, 4 and 6 U
  out       U |ref|; residual U (|bn| + |res| + |sum|)
  running   2^-22 (|(1 - f) rm| + |f mean|); num_batches_tracked advances by one
  sums      fp32_bound(sum |terms|, K), K = ceil(rows / nparts) (x 4 pooled); given partials:
            U |sum| (+ 2^-45 sum |rows| for the float64 order)
  dy        |sc| [2^-21 (|dz| + |k1| + |xhat k2|) + B0 / M + |xhat| B1 / M]
  db        training: 0 within |sc| fp32_bound(sum |xhat|, K) (|S1| + B1) / M; eval: sc S0 at
            |sc| B0 + U |ref|; odd pooled map: sum dy at the summed dy bounds + fp32_bound
Routing closer than 2^-20 relative is excluded per element and added to the sums' bounds; the
share is asserted <= 1e-5 per case.

Worst error / bound ratios seen on an MI355X (each test prints its own)
  forward   mean 0.49, invstd 0.50, scale 0.46, shift 0.24, out 0.50 (one rounding is half of U),
            running_mean 0.46, running_var 0.42; eval invstd 0.25, scale 0.24, shift 0.18;
            residual out 0.46
  backward  dbeta 0.050, dgamma 0.13, dy 0.21 (eval dy 0.50), db 0.48 (C = 4096, 32 rows),
            db eval 0.007, db over an odd pooled map 0.003
  part_in   dbeta 0.50, dgamma 0.49, dy 0.38, db 0.48
  prev_*    dx 0.003, sum dz 0.003, sum dz xhat 0.005, sum xhat 0.005
  momentum=None: before the fix in bn.hip (cma_arrive) running_mean was 1.4e6 bounds off at
  C = 4096 from the second call on (factor 1 / (k + 2) in channels whose workgroup started after
  channel 0's had finished); with it 0.40.
Ambiguous routing: 0 of 9.2 M elements over all backward cases (cap 1e-5).
"""
import pytest
import torch
import torch.nn.functional as F

from _bn_util import (BWD_REDUCE_ROWS, EPS, U, Worst, act_qmode, assert_dgrad_passthrough, bn_bwd_grid, bn_case,
                      bn_case_gpu, bwd_path, bwd_ref, check_out, check_stats_eval, check_stats_train,
                      check_sums_and_dy, cl, force, fp32_bound, fwd_path, lib, momentum_factor, new_state,
                      running_ref, run_fwd, set_env, split_rows, sum_K, _cv)

pytestmark = pytest.mark.gpu

S10 = (3, 10, 10)
_DEFAULT_ENGINE = []  # the engine the process started with (set by the L fixture)
SWEEP = [pytest.param(b, p, r, id=f"{'bias' if b else 'nobias'}-{'pool' if p else 'nopool'}-{'relu' if r else 'lin'}")
         for b in (False, True) for p in (False, True) for r in (True, False)]


@pytest.fixture
def L():
    """The native library on the f32 engine; engine and both overrides restored afterwards."""
    lb = lib()
    orig = lb.get_conv_gemm()
    _DEFAULT_ENGINE[:] = [orig]
    try:
        lb.set_conv_gemm("f32")
        yield lb
    finally:
        lb.set_conv_gemm(orig)
        lb.set_gemm_override("conv", 0, 0, 0)
        lb.set_gemm_override("wgrad", 0, 0, 0)


# ------------------------------------------------------------------------------ forward, training
def _fwd_train(L, monkeypatch, name, C, shp, bias, pool, relu, fin_env, path, nparts, qmode=None, kind="normal"):
    N, H, W = shp
    set_env(monkeypatch, "CDP_BN_FIN_ACT", fin_env)
    c, g = bn_case(C, N, H, W, kind), bn_case_gpu(C, N, H, W, kind)
    assert (c.M + 63) // 64 == nparts
    assert fwd_path(nparts, C, fin_env) == path
    if qmode is not None:
        assert act_qmode(C) == qmode
    state = new_state(g)
    rm0, rv0 = state[0].clone(), state[1].clone()
    r = run_fwd(L, c, g, bias=bias, pool=pool, relu=relu, state=state)
    wst = Worst(name)
    check_stats_train(wst, r, c)
    check_out(wst, r, c, pool, relu)
    rmr, rmb, rvr, rvb = running_ref(momentum_factor(0.1, 0), rm0, rv0, r.mean, r.var, c.M)
    wst.add("running_mean", state[0], rmr, rmb)
    wst.add("running_var", state[1], rvr, rvb)
    assert int(state[2].item()) == 1
    wst.finish()


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
def test_F1_fin_act64(L, monkeypatch, bias, pool, relu):
    """C = 64, 300 rows: 5 partials, the last of 44 rows -> bn_fin_act<64>."""
    _fwd_train(L, monkeypatch, "F1", 64, S10, bias, pool, relu, None, "fin_act64", 5)


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
def test_F2_fin_act16(L, monkeypatch, bias, pool, relu):
    """C = 128, 2,420 rows: 38 partials -> bn_fin_act<16>."""
    _fwd_train(L, monkeypatch, "F2", 128, (5, 22, 22), bias, pool, relu, None, "fin_act16", 38)


@pytest.mark.parametrize("shp,nparts,path", [((8, 64, 64), 512, "fin_act16"), ((9, 57, 64), 513, "finalize+act")],
                         ids=["512-fused", "513-unfused"])
def test_F2_fused_partial_limit(L, monkeypatch, shp, nparts, path):
    """The last fused partial count and the first that takes bn_finalize."""
    _fwd_train(L, monkeypatch, "F2-edge", 64, shp, False, False, True, None, path, nparts)


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
@pytest.mark.parametrize("C,qmode", [(12, 0), (96, 0), (32, 1)])
def test_F3_finalize_act_by_channel_count(L, monkeypatch, C, qmode, bias, pool, relu):
    """C % 64 != 0: bn_finalize + bn_act_fwd, qmode 0 (C = 12, 96) and 1 (C = 32)."""
    _fwd_train(L, monkeypatch, "F3", C, S10, bias, pool, relu, None, "finalize+act", 5, qmode)


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
@pytest.mark.parametrize("C,shp,qmode", [(2048, (2, 4, 4), 2), (64, S10, 1)], ids=["C2048", "C64"])
def test_F4_two_launch_forced(L, monkeypatch, C, shp, qmode, bias, pool, relu):
    """CDP_BN_FIN_ACT=0: bn_finalize + bn_act_fwd where the fused kernel would run; C = 2048 is
    qmode 2 with C / 4 > 256. C = 64 meets the bounds that test_F1 holds the fused path to."""
    _fwd_train(L, monkeypatch, "F4", C, shp, bias, pool, relu, "0", "finalize+act", (shp[0] * shp[1] * shp[2] + 63) // 64,
               qmode)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_F5_finalize_looped_batch(L, monkeypatch, bias):
    """2,059 partials: eleven past the 2,048 that bn_finalize holds in registers."""
    _fwd_train(L, monkeypatch, "F5", 4, (9, 121, 121), bias, False, True, None, "finalize+act", 2059, 1)


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
@pytest.mark.parametrize("C,path", [(64, "fin_act64"), (12, "finalize+act"), (96, "finalize+act"), (32, "finalize+act")])
def test_F6_large_mean(L, monkeypatch, C, path, bias, pool, relu):
    """Mean 1024, sigma 1, one constant channel (var = 0, invstd = eps^-1/2): the same bounds."""
    _fwd_train(L, monkeypatch, "F6", C, S10, bias, pool, relu, None, path, 5, kind="large_mean")


# ------------------------------------------------------------------------------ forward, other
@pytest.mark.parametrize("bias,pool,relu", SWEEP)
@pytest.mark.parametrize("C", [64, 12, 96, 32])
def test_forward_eval(L, C, bias, pool, relu):
    c, g = bn_case(C, *S10), bn_case_gpu(C, *S10)
    state = new_state(g)
    r = run_fwd(L, c, g, bias=bias, pool=pool, relu=relu, training=False, state=state)
    wst = Worst("eval")
    check_stats_eval(wst, r, c)
    check_out(wst, r, c, pool, relu)
    assert torch.equal(state[0], g.rm) and torch.equal(state[1], g.rv) and int(state[2].item()) == 0
    wst.finish()


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
def test_forward_affine_false(L, monkeypatch, bias, pool, relu):
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    c, g = bn_case(64, *S10), bn_case_gpu(64, *S10)
    r = run_fwd(L, c, g, bias=bias, pool=pool, relu=relu, affine=False, state=new_state(g))
    wst = Worst("affine=False")
    check_stats_train(wst, r, c, affine=False)
    check_out(wst, r, c, pool, relu)
    wst.finish()


@pytest.mark.parametrize("fin_env", [None, "0"], ids=["fused", "two-launch"])
@pytest.mark.parametrize("bias,pool,relu", SWEEP)
def test_forward_no_running_stats(L, monkeypatch, bias, pool, relu, fin_env):
    set_env(monkeypatch, "CDP_BN_FIN_ACT", fin_env)
    c, g = bn_case(64, *S10), bn_case_gpu(64, *S10)
    r = run_fwd(L, c, g, bias=bias, pool=pool, relu=relu, state=None)
    wst = Worst("track_running_stats=False")
    check_stats_train(wst, r, c)
    check_out(wst, r, c, pool, relu)
    wst.finish()


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("C", [64, 96])
def test_forward_residual(L, monkeypatch, C, bias):
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    c, g = bn_case(C, *S10), bn_case_gpu(C, *S10)
    assert fwd_path(5, C, None, residual=True) == "finalize+act"
    r = run_fwd(L, c, g, bias=bias, pool=False, relu=True, state=new_state(g), residual=True)
    wst = Worst("residual")
    check_stats_train(wst, r, c)
    check_out(wst, r, c, False, True, residual=True)
    wst.finish()
    if r.rmask is not None:  # CDP_RES_MASK is read once per process
        o = (r.out.permute(0, 2, 3, 1).reshape(-1, C // 4, 4) > 0).to(torch.int32)
        want = (o * torch.tensor([1, 2, 4, 8], device=o.device, dtype=torch.int32)).sum(-1).to(torch.uint8).reshape(-1)
        assert torch.equal(r.rmask.reshape(-1), want)


# ------------------------------------------------------------------------------ momentum=None
@pytest.mark.parametrize("C,shp,fin_env,path", [(4096, (2, 2, 2), "0", "finalize+act"), (512, (2, 2, 2), None, "fin_act64"),
                                                (512, (5, 22, 22), None, "fin_act16")],
                         ids=["C4096-finalize", "C512-fin_act64", "C512-fin_act16"])
def test_momentum_none_is_cumulative_average(L, monkeypatch, C, shp, fin_env, path):
    """BatchNorm2d(momentum=None): three calls with different inputs must leave the running
    statistics at the average of the three batches' statistics, every channel with the factor
    1 / (k + 1) of the count from before its launch. (a) one workgroup per channel, more than fit
    on the device at once; (b) the fused kernels. A factor taken after the count's increment is
    1 / (k + 2): off by O(1) relative."""
    N, H, W = shp
    set_env(monkeypatch, "CDP_BN_FIN_ACT", fin_env)
    c, g = bn_case(C, N, H, W), bn_case_gpu(C, N, H, W)
    nparts = (c.M + 63) // 64
    assert fwd_path(nparts, C, fin_env) == path
    state = new_state(g)
    wst = Worst("momentum=None")
    means, unbs = [], []
    erm = torch.zeros(C, dtype=torch.float64)  # accumulated bound against the float64 average
    erv = torch.zeros(C, dtype=torch.float64)
    for k in range(3):
        xk = cl((g.x * (1.0 + k) + 0.5 * k).contiguous())
        rm0, rv0 = state[0].clone(), state[1].clone()
        r = run_fwd(L, c, g, bias=False, pool=False, relu=True, state=state, momentum=-1.0, x=xk)
        f32 = momentum_factor(-1.0, k)
        rmr, rmb, rvr, rvb = running_ref(f32, rm0, rv0, r.mean, r.var, c.M)
        wst.add(f"running_mean[{k}]", state[0], rmr, rmb)
        wst.add(f"running_var[{k}]", state[1], rvr, rvb)
        assert int(state[2].item()) == k + 1
        means.append(r.mean)
        unbs.append(r.var * c.M / (c.M - 1))
        erm, erv = (1.0 - float(f32)) * erm + rmb, (1.0 - float(f32)) * erv + rvb
    # (the fp32 factors 1/2 and 1/3 against the exact ones: U on every term)
    wst.add("running_mean", state[0], sum(means) / 3.0, erm + U * sum(m.abs() for m in means))
    wst.add("running_var", state[1], sum(unbs) / 3.0, erv + U * sum(unbs))
    assert int(state[2].item()) == 3
    wst.finish()


# ------------------------------------------------------------------------------ backward
def _db_check(wst, ref, db, dyr, dybound, B0, B1, K, training, has_bias, pool, nblk):
    if not has_bias:
        assert db is None
        return
    sc = ref.sc.view(-1)
    odd = pool and (ref.H % 2 == 1 or ref.W % 2 == 1)
    if odd:  # bn_bwd_apply's partial sums of dy, finalized by chan_finalize
        npix = ref.N * (ref.H // 2) * (ref.W // 2)
        Kdb = 4 * -(-npix // nblk) + -(-ref.M // nblk)
        # (an ambiguous element's dy may differ by |sc| |g|: slack0)
        bound = dybound.sum((0, 2, 3)) + fp32_bound(dyr.abs().sum((0, 2, 3)), Kdb) + sc.abs() * ref.slack0
        wst.add("db(sum dy)", db, dyr.sum((0, 2, 3)), bound)
    elif training:  # -scale S2 S1 / M with S2 = sum xhat: exactly 0
        bound = sc.abs() * fp32_bound(ref.A2, K) * (ref.S1.abs() + B1) / ref.M
        wst.add("db(0)", db, torch.zeros_like(ref.S0), bound)
    else:
        wst.add("db(eval)", db, sc * ref.S0, sc.abs() * B0 + U * (sc * ref.S0).abs())


def _bwd(L, monkeypatch, name, C, shp, bias, pool, relu, fin_env, path, training=True, nparts_range=None):
    N, H, W = shp
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    set_env(monkeypatch, "CDP_BN_BWD_FIN", fin_env)
    nparts = bn_bwd_grid(N, H, W, C, pool)
    if nparts_range is not None:
        assert nparts_range[0] < nparts <= nparts_range[1], nparts
    assert bwd_path(nparts, N, C, H, W, pool, bias, fin_env, training) == path
    c, g = bn_case(C, N, H, W), bn_case_gpu(C, N, H, W)
    assert_dgrad_passthrough(L, c, g)
    r = run_fwd(L, c, g, bias=bias, pool=pool, relu=relu, training=training, state=new_state(g))
    res = L.conv_bn_act_bwd(g.gout[pool], r.xs, r.w, r.y, r.stats, 1, 0, pool, relu, True, bias, None, training)
    dx, _, db, dgamma, dbeta = res[:5]
    ref = bwd_ref(r.y, r.stats, c.gout[pool], pool, relu)
    K = sum_K(ref, nparts)
    wst = Worst(f"{name} nparts={nparts} ambiguous={ref.n_amb}/{ref.n_total}")
    if training:
        dyr, dyb, B0, B1 = check_sums_and_dy(wst, ref, dx, dbeta, dgamma, K)
    else:  # a fixed affine map: dy = scale dz; dgamma with the running statistics
        B0, B1 = fp32_bound(ref.A0, K) + ref.slack0, fp32_bound(ref.A1, K) + ref.slack1
        wst.add("dbeta", dbeta, ref.S0, B0)
        wst.add("dgamma", dgamma, ref.S1, B1)
        dyr = ref.sc * ref.dz
        dyb = U * dyr.abs()
        wst.add("dy", torch.where(ref.amb, dyr, dx.double().cpu()), dyr, dyb)
    _db_check(wst, ref, db, dyr, dyb, B0, B1, K, training, bias, pool, nparts)
    wst.finish()


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
def test_B1_fin_apply(L, monkeypatch, bias, pool, relu):
    """C = 64, (3, ., 10, 10): 19 partials (5 pooled) -> bn_bwd_reduce + bn_bwd_fin_apply."""
    _bwd(L, monkeypatch, "B1", 64, S10, bias, pool, relu, None, "fin_apply", nparts_range=(0, 128))


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
@pytest.mark.parametrize("C,fin_env", [(64, "0"), (12, None), (96, None)])
def test_B2_reduce_finalize_apply(L, monkeypatch, C, fin_env, bias, pool, relu):
    """bn_bwd_reduce + chan_finalize + bn_bwd_apply: forced at C = 64, the only path at C % 64 != 0."""
    _bwd(L, monkeypatch, "B2", C, S10, bias, pool, relu, fin_env, "finalize+apply", nparts_range=(0, 512))


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("C", [64, 12])
def test_B2_odd_pooled_map(L, monkeypatch, C, bias, relu):
    """(2, ., 7, 9) pooled: the border outside every window gets dz = 0, and the bias gradient takes
    the separate partial pass over dy."""
    _bwd(L, monkeypatch, "B2-odd", C, (2, 7, 9), bias, True, relu, None, "finalize+apply")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_B3_chan_finalize8(L, monkeypatch, bias, relu):
    """C = 256, 5,120 rows: 640 partials -> chan_finalize8."""
    _bwd(L, monkeypatch, "B3", 256, (5, 32, 32), bias, False, relu, None, "finalize8+apply", nparts_range=(512, 1024))


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
@pytest.mark.parametrize("C,fin_env,path", [(2048, None, "fin_apply"), (2048, "0", "finalize+apply"),
                                            (4096, None, "fin_apply"), (4096, "0", "finalize+apply")])
def test_B4_channel_quads_beyond_one_pass(L, monkeypatch, C, fin_env, path, bias, pool, relu):
    """C / 4 = 512 and 1,024: bn_bwd_reduce (and, unfused, bn_bwd_apply) walk two and four passes
    of 256 channel quads."""
    _bwd(L, monkeypatch, "B4", C, (2, 4, 4), bias, pool, relu, fin_env, path, nparts_range=(0, 128))


@pytest.mark.parametrize("bias,pool,relu", SWEEP)
def test_B5_eval_backward(L, monkeypatch, bias, pool, relu):
    _bwd(L, monkeypatch, "B5", 64, S10, bias, pool, relu, None, "finalize+apply", training=False)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_B5_eval_backward_odd_pooled_map(L, monkeypatch, bias, relu):
    _bwd(L, monkeypatch, "B5-odd", 64, (2, 7, 9), bias, True, relu, None, "finalize+apply", training=False)


@pytest.mark.parametrize("by", ["out", "mask"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_B6_residual(L, monkeypatch, bias, by):
    """A residual block's backward: the ReLU routed by the block's output or by its pass mask, and
    dres = dz."""
    C = 64
    N, H, W = S10
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    set_env(monkeypatch, "CDP_BN_BWD_FIN", None)
    nparts = bn_bwd_grid(N, H, W, C, False)
    assert bwd_path(nparts, N, C, H, W, False, bias, None, True, zout=True) == "finalize+apply"
    c, g = bn_case(C, N, H, W), bn_case_gpu(C, N, H, W)
    assert_dgrad_passthrough(L, c, g)
    r = run_fwd(L, c, g, bias=bias, pool=False, relu=True, state=new_state(g), residual=True)
    if by == "mask" and r.rmask is None:
        pytest.skip("this process runs without the residual ReLU mask (CDP_RES_MASK=0)")
    zout = r.out if by == "out" else r.rmask
    res = L.conv_bn_act_bwd(g.gout[False], r.xs, r.w, r.y, r.stats, 1, 0, False, True, True, bias, zout, True)
    dx, _, db, dgamma, dbeta, dres = res[:6]
    ref = bwd_ref(r.y, r.stats, c.gout[False], False, True, route_from=r.out)
    K = sum_K(ref, nparts)
    wst = Worst(f"B6-{by}")
    dyr, dyb, B0, B1 = check_sums_and_dy(wst, ref, dx, dbeta, dgamma, K)
    _db_check(wst, ref, db, dyr, dyb, B0, B1, K, True, bias, False, nparts)
    assert torch.equal(dres.cpu(), ref.dz.float()), "dres != dz"
    wst.finish()


# ------------------------------------------------------------------------------ synthetic part_in
def _synthetic(L, monkeypatch, C, nparts, ps, pool, fin_env, path):
    N, H, W = S10
    bias = ps == 3
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    set_env(monkeypatch, "CDP_BN_BWD_FIN", fin_env)
    assert bwd_path(nparts, N, C, H, W, pool, bias, fin_env) == path
    c, g = bn_case(C, N, H, W), bn_case_gpu(C, N, H, W)
    assert_dgrad_passthrough(L, c, g)
    r = run_fwd(L, c, g, bias=bias, pool=pool, relu=True, state=new_state(g))
    ref = bwd_ref(r.y, r.stats, c.gout[pool], pool, True)
    gen = torch.Generator().manual_seed(100 * nparts + ps)
    cols = [split_rows(s, nparts, gen) for s in (ref.S0, ref.S1, ref.S2)[:ps]]
    part = torch.stack(cols, -1).contiguous()
    assert tuple(part.shape) == (nparts, C, ps)
    pd = part.double()
    S, noise = pd.sum(0), 2.0 ** -45 * pd.abs().sum(0)  # [C, ps]; the float64 merge's order
    B = U * S.abs() + noise
    res = L.conv_bn_act_bwd(g.gout[pool], r.xs, r.w, r.y, r.stats, 1, 0, pool, True, True, bias, None, True,
                            part_in=part.cuda())
    dx, _, db, dgamma, dbeta = res[:5]
    wst = Worst(f"part_in C={C} nparts={nparts} ps={ps}")
    check_sums_and_dy(wst, ref, dx, dbeta, dgamma, None, sums=(S[:, 0], S[:, 1], B[:, 0], B[:, 1]))
    if ps == 3:
        sc = ref.sc.view(-1)
        dbr = -sc * S[:, 2] * S[:, 1] / ref.M
        wst.add("db", db, dbr, U * dbr.abs() + sc.abs() * (noise[:, 2] * S[:, 1].abs() + S[:, 2].abs() * noise[:, 1]) / ref.M)
    wst.finish()


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ps", [2, 3])
@pytest.mark.parametrize("nparts", [1, 5, 127, 128])
def test_part_in_fused_merge(L, monkeypatch, nparts, ps, pool):
    """bn_bwd_fin_apply merges any [nparts <= 128, C, ps] partials as their float64 sum."""
    _synthetic(L, monkeypatch, 64, nparts, ps, pool, "1", "fin_apply")


@pytest.mark.parametrize("pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("ps", [2, 3])
@pytest.mark.parametrize("nparts", [129, 1024, 1025, 2500])
def test_part_in_chan_finalize(L, monkeypatch, nparts, ps, pool):
    """chan_finalize: one batch of loads up to 1,024 partials, its tail loop past them."""
    _synthetic(L, monkeypatch, 64, nparts, ps, pool, "1", "finalize+apply")


@pytest.mark.parametrize("ps", [2, 3])
@pytest.mark.parametrize("nparts", [513, 1000])
def test_part_in_chan_finalize8(L, monkeypatch, nparts, ps):
    """C = 260: 33 blocks of 8 channels, the last with 4."""
    _synthetic(L, monkeypatch, 260, nparts, ps, False, None, "finalize8+apply")


# ------------------------------------------------------------------------------ prev_* (bwd_reduce_kernel)
@pytest.mark.parametrize("prev_relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("prev_ps", [2, 3])
@pytest.mark.parametrize("prev_pool", [False, True], ids=["nopool", "pool"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("engine", ["f32", "default"])
def test_prev_bn_partials_of_bwd_reduce(L, monkeypatch, engine, splits, prev_pool, prev_ps, prev_relu):
    """A real 3x3 conv (96 -> 64 channels) over a dX of (3, 96, 10, 10): 300 rows, so the last of the
    10 partials holds 12, and the second 64-column block is partial. The BN job's partials, summed
    in float64, against the sums formed from the returned dx, prev_y and prev_stats; dx itself
    against the float64 data gradient (splits = 1 reads it back in place and must leave it intact)."""
    set_env(monkeypatch, "CDP_BN_FIN_ACT", None)
    set_env(monkeypatch, "CDP_BN_BWD_FIN", None)
    Ci, Co, N, H, W = 96, 64, 3, 10, 10
    gen = torch.Generator().manual_seed(31 + 2 * prev_pool)
    pH, pW = (2 * H, 2 * W) if prev_pool else (H, W)
    prev_y = torch.randn(N, Ci, pH, pW, generator=gen)
    pg, pb = 0.5 + torch.rand(Ci, generator=gen), torch.randn(Ci, generator=gen)
    mu = prev_y.mean((0, 2, 3))
    istd = 1.0 / torch.sqrt(prev_y.var((0, 2, 3), unbiased=False) + EPS)
    prev_stats = torch.stack([mu, istd, pg * istd, pb - mu * pg * istd]).contiguous()
    x = prev_y * _cv(prev_stats[2]) + _cv(prev_stats[3])
    x = F.relu(x) if prev_relu else x
    x = F.max_pool2d(x, 2) if prev_pool else x
    w = torch.randn(Co, Ci, 3, 3, generator=gen) / (9 * Ci) ** 0.5
    gamma, beta, bias = 0.5 + torch.rand(Co, generator=gen), torch.randn(Co, generator=gen), torch.randn(Co, generator=gen)
    gout = torch.randn(N, Co, H, W, generator=gen)
    if engine != "f32":
        L.set_conv_gemm(_DEFAULT_ENGINE[0])
    xg, wg = cl(x.cuda()), cl(w.cuda())
    out, y, stats, xs, _, xa, wa, _ = L.conv_bn_act_fwd(xg, wg, bias.cuda(), gamma.cuda(), beta.cuda(), None, None, None,
                                                        0.1, EPS, True, 1, 1, False, True, None)
    force(L, "dgrad", 64, 64, splits, (N * H * W, Ci, 9 * Co), (64, 64, splits))
    res = L.conv_bn_act_bwd(cl(gout.cuda()), xs, wg, y, stats, 1, 1, False, True, True, True, None, True, None, None,
                            None, None, None, xa, wa, None, None, cl(prev_y.cuda()), prev_stats.cuda(), prev_pool,
                            prev_relu, prev_ps)
    dx, prev_part = res[0], res[6]
    if prev_part is None:
        import os
        if os.environ.get("CDP_BWD_FUSE", "1")[:1] == "0":
            pytest.skip("this process runs with CDP_BWD_FUSE=0")
    assert prev_part is not None, "prev_part not returned although the fused backward reduction is on"
    nrow = (N * H * W + BWD_REDUCE_ROWS - 1) // BWD_REDUCE_ROWS
    assert tuple(prev_part.shape) == (nrow, Ci, prev_ps)
    wst = Worst(f"prev {engine} s{splits}")
    # this block's dy in float64, then dx through the conv's data gradient
    ref = bwd_ref(y, stats, gout, False, True)
    K = sum_K(ref, bn_bwd_grid(N, H, W, Co, False))
    B0, B1 = fp32_bound(ref.A0, K) + ref.slack0, fp32_bound(ref.A1, K) + ref.slack1
    k1, k2 = _cv(ref.S0) / ref.M, _cv(ref.S1) / ref.M
    dyr = ref.sc * (ref.dz - k1 - ref.xh * k2)
    dyb = ref.sc.abs() * (2.0 ** -21 * (ref.dz.abs() + k1.abs() + (ref.xh * k2).abs()) + _cv(B0) / ref.M
                          + ref.xh.abs() * _cv(B1) / ref.M) + ref.amb * ref.sc.abs() * gout.double().abs()
    wd = w.double()
    dxr = F.conv_transpose2d(dyr, wd, padding=1)
    dxa = F.conv_transpose2d(dyr.abs(), wd.abs(), padding=1)
    wst.add("dx", dx, dxr, fp32_bound(dxa, 9 * Co) + F.conv_transpose2d(dyb, wd.abs(), padding=1))
    # the previous block's statistics sums over the returned dx
    pref = bwd_ref(prev_y, prev_stats, dx, prev_pool, prev_relu)
    Kp = BWD_REDUCE_ROWS * (4 if prev_pool else 1)
    got = prev_part.double().cpu().sum(0)
    wst.add("sum dz", got[:, 0], pref.S0, fp32_bound(pref.A0, Kp) + pref.slack0)
    wst.add("sum dz xhat", got[:, 1], pref.S1, fp32_bound(pref.A1, Kp) + pref.slack1)
    if prev_ps == 3:
        wst.add("sum xhat", got[:, 2], pref.S2, fp32_bound(pref.A2, Kp))
    wst.finish()
