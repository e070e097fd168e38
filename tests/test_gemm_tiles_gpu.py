"""Every conv GEMM tile and split-K count, forced through set_gemm_override, against fp64 at shapes
with M, N and K tails.

The planner (plan_gemm / plan_wgrad, csrc/runtime/ops.cpp) picks one tile and split count per shape,
so the rest of the suite sees one instantiation per (engine, kind). Here the plan is forced, proved
through plan_info before every launch, and each output element is held to the fp32 dot-product bound
of tests/test_accuracy_gpu.py (c = 4, the same K per kind):

    |y - y_fp64| <= 4 (2^-22 + K 2^-24) sum_i |a_i||b_i|

with the fp64 references computed once per (shape, data kind) on the CPU (tests/_gemm_util.py). The
bf16 fast mode rounds both operands to bf16, relative 2^-9 each, so its bound is
(2^-8 + 2^-18) sum|a||b| plus the fp32 bound: derived, not measured.

Covered instantiations
  engines   f32 (conv_igemm.hip, wgrad_kernel), x3 (NP = 3), f16x2 (NP = 2), bf16 (NP = 1)
  conv      64x64, 64x128, 128x64, 128x128 for every engine, 256x128 for x3 / f16x2 / bf16; forward and
            transposed-gather data gradient; MODE 0 (S1, S4, S5), MODE 1 (S2), MODE 2 (S3); split-K
            counts 1, 2, one that does not divide the K-tiles, K-tiles - 1 (slices of 1 and 2 K-tiles
            behind the two-stage prefetch) and a request past the K-tiles (clamped: every slice one
            K-tile); bf16 at 1 and the clamp only
  wgrad     the four tiles for every engine, fast (S1, S2) and generic (S3) paths, the 512-thread
            256x128 f16x2 tile (S1, S2); splits 1, 3 and a request past the 32-row steps (clamped)
  stride 2  every x3 / f16x2 tile at splits 1 and 3 over the sub-pixel class GEMMs (S4), with the row
            remap in the kernel (splits 1) and in the reduction (splits 3), with and without an addend
  epilogue  bias, BN partials (single-row last partial, output mean 1024), in-place addend, weight
            gradient into out= (accumulating or not), bitwise determinism under split-K: per tile
            at splits 1 and 4 (conv) / 3 (wgrad) on S1 for f16x2, x3 and f32

Left out, because the host normalises them to a configuration already listed (plan_gemm /
plan_wgrad) -- the kernels do not exist:
  * conv 256x128 with the f32 engine: becomes 128x128 (conv_igemm.hip has no 256-row tile)
  * wgrad 256x128 with any engine but f16x2, or with Cout % 4 != 0 (S3): becomes 128x128
    (wgrad_launch has the 512-thread tile for the pipelined f16x2 fast path only)
  * 256 rows with 64 columns: set_gemm_override refuses it
  * split counts past the K-tiles / row steps run as the clamp; no slice is ever empty
test_overrides_normalise_as_documented pins these.

Shapes (N, Ci, H, W, Co, k, stride, pad), gather mode and weight-gradient path read from
conv_x3_launch / conv_igemm_launch / wgrad_launch:
  S1 (3, 96, 10, 10, 160, 3, 1, 1)  fwd M 300 N 160 K 864 (27 K-tiles), dgrad M 300 N 96 K 1440 (45):
     C % 32 == 0 and Kdim % 32 == 0 both ways -> MODE 0. wgrad Cout 160, Kdim 864, 10 row steps (the
     last 12 rows): C % 4 == Cout % 4 == 0 -> fast path (f16x2: the pipelined kernel, and 256x128).
     P Q = 100, so 128- and 256-row tiles span images (f16x2's per-image A scale is looked up per row).
  S2 (2, 12, 11, 13, 20, 3, 1, 1)   fwd M 286 N 20 K 108 (4 K-tiles, the last 12 wide), dgrad N 12
     K 180 (6, the last 20 wide): C % 4 == 0 but not % 32 -> MODE 1, K-runs of 8 straddle taps, every
     FastDiv divisor (13, 143, 12 / 20, 3) not a power of two. wgrad: fast path, 9 row steps.
  S3 (2, 7, 9, 9, 10, 3, 1, 1)      fwd M 162 N 10 K 63, dgrad N 7 K 90 (gather source C = Co = 10):
     MODE 2 both ways. conv2d_fwd does not pad channels (only the fused block forward does, which
     would make Ci 8 and take MODE 1). Nout % 4 != 0: narrow epilogue and the scalar splitk_reduce
     kernel. wgrad: generic (non-fast) path, un-pipelined for f16x2, 6 row steps.
  S4 (2, 64, 15, 15, 128, 3, 2, 1) and (2, 128, 14, 14, 256, 1, 2, 0): stride-2 data gradient as
     sub-pixel class GEMMs, gather source C = Co, Kc a multiple of 128 -> MODE 0; the 1x1 case has
     three tap-less classes.
  S5 (2, 576, 5, 5, 576, 1, 1, 0)   f16x2 only: 18 > 16 per-row |max| partials of W (fwd) and W^T
     (dgrad), MODE 0; the largest weights sit in the last 64 channels, past the first 16 partials.
"""
import pytest
import torch

from _gemm_util import (ENGINES, SPLITK_ROWS_PER_PART, check_bound, cl, conv_case, conv_case_gpu, conv_splits,
                        conv_tiles, force, ktiles, lib, merge_bn_partials, subpixel_classes, wgrad_splits,
                        wgrad_tiles)

pytestmark = pytest.mark.gpu

S1 = (3, 96, 10, 10, 160, 3, 1, 1)
S2 = (2, 12, 11, 13, 20, 3, 1, 1)
S3 = (2, 7, 9, 9, 10, 3, 1, 1)
S4 = [(2, 64, 15, 15, 128, 3, 2, 1), (2, 128, 14, 14, 256, 1, 2, 0)]
S5 = (2, 576, 5, 5, 576, 1, 1, 0)
S1_ROW1 = (257, 96, 1, 1, 160, 1, 1, 0)  # M = 257: the last BN partial of every tile (and of 32) is one row
SHAPES = {"S1": S1, "S2": S2, "S3": S3}
ALL_ENGINES = ENGINES + ["bf16"]


def _mnk(shape, gemm):
    N, Ci, H, W, Co, k, s, p = shape
    P, Q = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    if gemm == "dgrad":
        return (N * H * W, Ci, k * k * Co)
    return (N * P * Q, Co, k * k * Ci)  # fwd (M, N, K) and wgrad (rows, Cout, Kdim)


@pytest.fixture
def L():
    """The native library with the engine saved; engine and both overrides restored afterwards."""
    lb = lib()
    orig = lb.get_conv_gemm()
    try:
        yield lb
    finally:
        lb.set_conv_gemm(orig)
        lb.set_gemm_override("conv", 0, 0, 0)
        lb.set_gemm_override("wgrad", 0, 0, 0)


def _conv_sweep():
    out = []
    for sid, shape in SHAPES.items():
        for engine in ALL_ENGINES:
            for gemm in ("fwd", "dgrad"):
                kt = ktiles(_mnk(shape, gemm)[2])
                for bm, bn in conv_tiles(engine):
                    for req, eff in conv_splits(kt, engine):
                        for kind in ("normal", "image_spread"):
                            out.append(pytest.param(sid, engine, gemm, bm, bn, req, eff, kind,
                                                    id=f"{sid}-{engine}-{gemm}-{bm}x{bn}-s{req}-{kind}"))
    return out


@pytest.mark.parametrize("sid,engine,gemm,bm,bn,req,eff,kind", _conv_sweep())
def test_conv_tile_split_meets_bound(L, sid, engine, gemm, bm, bn, req, eff, kind):
    shape = SHAPES[sid]
    c = conv_case(shape, kind)
    xc, wc, gyc = conv_case_gpu(shape, kind)
    L.set_conv_gemm(engine)
    if gemm == "fwd":
        force(L, "conv", bm, bn, req, c.fwd_mnk, (bm, bn, eff))
        got = L.conv2d_fwd(xc, wc, None, shape[6], shape[7], False)[0]
        check_bound("fwd", got, c.y, c.abs_y, c.K_fwd, engine=engine)
    else:
        force(L, "dgrad", bm, bn, req, c.dgrad_mnk, (bm, bn, eff))
        got = L.conv2d_dgrad(gyc, wc, list(c.x.shape), shape[6], shape[7])
        check_bound("dgrad", got, c.dx, c.abs_dx, c.K_dgrad, engine=engine)


def _wgrad_sweep():
    out = []
    for sid, shape in SHAPES.items():
        M, Cout, _ = _mnk(shape, "wgrad")
        for engine in ALL_ENGINES:
            for bm, bn in wgrad_tiles(engine, Cout):
                for req, eff in wgrad_splits(M, engine):
                    for kind in ("normal", "image_spread") + (("channel_spread",) if sid == "S1" else ()):
                        out.append(pytest.param(sid, engine, bm, bn, req, eff, kind,
                                                id=f"{sid}-{engine}-{bm}x{bn}-s{req}-{kind}"))
    return out


@pytest.mark.parametrize("sid,engine,bm,bn,req,eff,kind", _wgrad_sweep())
def test_wgrad_tile_split_meets_bound(L, sid, engine, bm, bn, req, eff, kind):
    shape = SHAPES[sid]
    c = conv_case(shape, kind)
    xc, wc, gyc = conv_case_gpu(shape, kind)
    L.set_conv_gemm(engine)
    force(L, "wgrad", bm, bn, req, c.wgrad_mnk, (bm, bn, eff))
    got = L.conv2d_wgrad(gyc, xc, list(c.w.shape), shape[6], shape[7])
    check_bound("wgrad", got, c.dw, c.abs_dw, c.K_wgrad, engine=engine)


# ------------------------------------------------------------------------------ S4: stride 2
@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("bm,bn", conv_tiles("x3"), ids=lambda v: str(v))
@pytest.mark.parametrize("engine", ["f16x2", "x3"])
@pytest.mark.parametrize("shape", S4, ids=["3x3s2", "1x1s2"])
def test_stride2_dgrad_subpixel_classes(L, shape, engine, bm, bn, splits, addend):
    c = conv_case(shape, "normal")
    _, wc, gyc = conv_case_gpu(shape, "normal")
    L.set_conv_gemm(engine)
    L.set_gemm_override("conv", bm, bn, splits)
    classes = subpixel_classes(shape)
    assert len(classes) == (4 if shape[5] == 3 else 1)
    for Mc, Nout, Kc in classes:  # every class GEMM runs the forced tile (all have >= 4 K-tiles)
        assert list(L.plan_info("dgrad", Mc, Nout, Kc)) == [bm, bn, splits], (Mc, Nout, Kc)
    if addend:
        base = cl(torch.randn(c.x.shape, generator=torch.Generator().manual_seed(5)))
        acc = base.cuda()
        got = L.conv2d_dgrad(gyc, wc, list(c.x.shape), 2, shape[7], acc)
        assert got.data_ptr() == acc.data_ptr()
        check_bound("dgrad+addend", got, c.dx + base.double(), c.abs_dx, c.K_dgrad, extra=2.0 ** -23 * base.double().abs())
    else:
        got = L.conv2d_dgrad(gyc, wc, list(c.x.shape), 2, shape[7])
        check_bound("dgrad", got, c.dx, c.abs_dx, c.K_dgrad)


# ------------------------------------------------------------------------------ S5: wide weights
@pytest.mark.parametrize("tile", [None, (128, 64, 1), (64, 128, 4)], ids=["planner", "128x64-s1", "64x128-s4"])
def test_f16x2_wide_weight_row_maxima(L, tile):
    """576 input and output channels: 18 per-row |max| partials, two past the 16 that conv_x3_body
    loads up front. The largest weights sit in the last 64 channels (2^6 above the rest), so a scale
    taken from the first 16 partials alone would overflow fp16."""
    c = conv_case(S5, "normal", True)
    xc, wc, gyc = conv_case_gpu(S5, "normal", True)
    L.set_conv_gemm("f16x2")
    if tile is not None:
        force(L, "conv", *tile, c.fwd_mnk, tile)
        force(L, "dgrad", *tile, c.dgrad_mnk, tile)
    y = L.conv2d_fwd(xc, wc, None, 1, 0, False)[0]
    dx = L.conv2d_dgrad(gyc, wc, list(c.x.shape), 1, 0)
    check_bound("fwd", y, c.y, c.abs_y, c.K_fwd)
    check_bound("dgrad", dx, c.dx, c.abs_dx, c.K_dgrad)


# ------------------------------------------------------------------------------ ride-alongs on S1
def _ride(splits_gt1):
    return [pytest.param(e, bm, bn, s, id=f"{e}-{bm}x{bn}-s{s}") for e in ENGINES for bm, bn in conv_tiles(e)
            for s in (1, splits_gt1)]


def _ride_wgrad():
    return [pytest.param(e, bm, bn, s, id=f"{e}-{bm}x{bn}-s{s}") for e in ENGINES
            for bm, bn in wgrad_tiles(e, S1[4]) for s in (1, 3)]


def _bias(Co, offset=0.0):
    return torch.randn(Co, generator=torch.Generator().manual_seed(13)) + offset


@pytest.mark.parametrize("engine,bm,bn,splits", _ride(4))
def test_forward_bias(L, engine, bm, bn, splits):
    """The bias is one more term of every output's sum: |b| joins sum |a||b| (splits > 1: added by
    the split-K reduction, else by the GEMM epilogue)."""
    c = conv_case(S1, "normal")
    xc, wc, _ = conv_case_gpu(S1, "normal")
    b = _bias(S1[4])
    L.set_conv_gemm(engine)
    force(L, "conv", bm, bn, splits, c.fwd_mnk, (bm, bn, splits))
    y = L.conv2d_fwd(xc, wc, b.cuda(), 1, 1, False)[0]
    bd = b.double().view(1, -1, 1, 1)
    check_bound("fwd+bias", y, c.y + bd, c.abs_y + bd.abs(), c.K_fwd)


def _bn_stats(L, shape, engine, bm, bn, splits, bias):
    c = conv_case(shape, "normal")
    xc, wc, _ = conv_case_gpu(shape, "normal")
    L.set_conv_gemm(engine)
    force(L, "conv", bm, bn, splits, c.fwd_mnk, (bm, bn, splits))
    y, part, rpp = L.conv2d_fwd(xc, wc, None if bias is None else bias.cuda(), shape[6], shape[7], True)
    rpp, M = int(rpp.item()), c.fwd_mnk[0]
    assert rpp == (bm if splits == 1 else SPLITK_ROWS_PER_PART)
    assert tuple(part.shape) == ((M + rpp - 1) // rpp, shape[4], 2)
    mean, var = merge_bn_partials(part, rpp, M)
    yd = y.double().cpu()  # the kernel's own output: the statistics apart from the GEMM's rounding
    return yd, rpp, mean, var, yd.mean((0, 2, 3)), yd.var((0, 2, 3), unbiased=False)


@pytest.mark.parametrize("shape", [S1, S1_ROW1], ids=["S1", "M257"])
@pytest.mark.parametrize("engine,bm,bn,splits", _ride(2))
def test_bn_partials_match_own_output(L, shape, engine, bm, bn, splits):
    """BN partials (mean, M2 per rpp-row group) merged in float64 against the float64 statistics of
    the returned y. M257 is a 1x1 conv over 257 one-pixel images: 257 = 1 mod 256, 128, 64 and 32, so
    the last partial of every layout holds a single row."""
    _, _, mean, var, mean_ref, var_ref = _bn_stats(L, shape, engine, bm, bn, splits, None)
    torch.testing.assert_close(mean, mean_ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(var, var_ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("engine,bm,bn,splits", _ride(2))
def test_bn_partials_with_large_mean(L, engine, bm, bn, splits):
    """Bias 1024: outputs of mean ~1024 and standard deviation ~1. A partial's fp32 mean may be off
    by rpp 2^-24 max|y| (rpp <= 256); the variance must still be right to 1e-3 relative, which needs
    the partials' two-pass form. Raw sums do not get there: E[y^2] - E[y]^2 in fp32 over the same y
    is off by 5.9e-1 relative at its worst channel and 1.1e-1 at the median one (computed on the CPU
    for this test's data from the fp32-rounded fp64 output; the test re-checks on the kernel's y
    that the worst channel misses by at least 1e-2, ten times the tolerance)."""
    yd, rpp, mean, var, mean_ref, var_ref = _bn_stats(L, S1, engine, bm, bn, splits, _bias(S1[4], 1024.0))
    assert 1000.0 < mean_ref.min() and mean_ref.max() < 1050.0 and 0.5 < var_ref.min() and var_ref.max() < 2.0
    y32 = yd.float()
    naive = (y32 * y32).mean((0, 2, 3)) - y32.mean((0, 2, 3)) ** 2
    assert ((naive.double() - var_ref).abs() / var_ref).max().item() >= 1e-2
    assert (mean - mean_ref).abs().max().item() <= rpp * 2.0 ** -24 * yd.abs().max().item()
    assert ((var - var_ref).abs() / var_ref).max().item() <= 1e-3


@pytest.mark.parametrize("engine,bm,bn,splits", _ride(4))
def test_dgrad_addend_in_place(L, engine, bm, bn, splits):
    c = conv_case(S1, "normal")
    _, wc, gyc = conv_case_gpu(S1, "normal")
    base = cl(torch.randn(c.x.shape, generator=torch.Generator().manual_seed(5)))
    acc = base.cuda()
    L.set_conv_gemm(engine)
    force(L, "dgrad", bm, bn, splits, c.dgrad_mnk, (bm, bn, splits))
    dx = L.conv2d_dgrad(gyc, wc, list(c.x.shape), 1, 1, acc)
    assert dx.data_ptr() == acc.data_ptr()
    check_bound("dgrad+addend", dx, c.dx + base.double(), c.abs_dx, c.K_dgrad, extra=2.0 ** -23 * base.double().abs())


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("engine,bm,bn,splits", _ride_wgrad())
def test_wgrad_into_out(L, engine, bm, bn, splits, accumulate):
    c = conv_case(S1, "normal")
    xc, _, gyc = conv_case_gpu(S1, "normal")
    base = cl(torch.randn(c.w.shape, generator=torch.Generator().manual_seed(6)))
    out = base.cuda()
    L.set_conv_gemm(engine)
    force(L, "wgrad", bm, bn, splits, c.wgrad_mnk, (bm, bn, splits))
    dw = L.conv2d_wgrad(gyc, xc, list(c.w.shape), 1, 1, out, accumulate)
    assert dw.data_ptr() == out.data_ptr()
    if accumulate:
        check_bound("wgrad+=", dw, c.dw + base.double(), c.abs_dw, c.K_wgrad, extra=2.0 ** -23 * base.double().abs())
    else:
        check_bound("wgrad->out", dw, c.dw, c.abs_dw, c.K_wgrad)


@pytest.mark.parametrize("engine,bm,bn", [pytest.param(e, bm, bn, id=f"{e}-{bm}x{bn}") for e in ENGINES
                                          for bm, bn in conv_tiles(e)])
def test_conv_split_k_is_deterministic(L, engine, bm, bn):
    """Two launches under forced split-K are bitwise equal: y and its BN partials, and dX."""
    c = conv_case(S1, "normal")
    xc, wc, gyc = conv_case_gpu(S1, "normal")
    L.set_conv_gemm(engine)
    force(L, "conv", bm, bn, 4, c.fwd_mnk, (bm, bn, 4))
    force(L, "dgrad", bm, bn, 4, c.dgrad_mnk, (bm, bn, 4))
    a = L.conv2d_fwd(xc, wc, None, 1, 1, True)
    b = L.conv2d_fwd(xc, wc, None, 1, 1, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    da = L.conv2d_dgrad(gyc, wc, list(c.x.shape), 1, 1)
    db = L.conv2d_dgrad(gyc, wc, list(c.x.shape), 1, 1)
    assert torch.equal(da, db)


@pytest.mark.parametrize("engine,bm,bn", [pytest.param(e, bm, bn, id=f"{e}-{bm}x{bn}") for e in ENGINES
                                          for bm, bn in wgrad_tiles(e, S1[4])])
def test_wgrad_split_k_is_deterministic(L, engine, bm, bn):
    c = conv_case(S1, "normal")
    xc, _, gyc = conv_case_gpu(S1, "normal")
    L.set_conv_gemm(engine)
    force(L, "wgrad", bm, bn, 3, c.wgrad_mnk, (bm, bn, 3))
    a = L.conv2d_wgrad(gyc, xc, list(c.w.shape), 1, 1)
    b = L.conv2d_wgrad(gyc, xc, list(c.w.shape), 1, 1)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------ host normalisation
def test_overrides_normalise_as_documented(L):
    """The requests this module leaves out run as a configuration it lists, or are refused."""
    M, N, K = conv_case(S1, "normal").fwd_mnk
    rows, Cout, Kdim = conv_case(S1, "normal").wgrad_mnk
    L.set_conv_gemm("f32")
    L.set_gemm_override("conv", 256, 128, 2)
    assert list(L.plan_info("conv", M, N, K)) == [128, 128, 2]
    assert list(L.plan_info("dgrad", M, N, K)) == [128, 128, 2]
    for engine in ("f32", "x3", "bf16"):
        L.set_conv_gemm(engine)
        L.set_gemm_override("wgrad", 256, 128, 3)
        assert list(L.plan_info("wgrad", rows, Cout, Kdim)) == [128, 128, 3]
    L.set_conv_gemm("f16x2")
    assert list(L.plan_info("wgrad", rows, Cout, Kdim)) == [256, 128, 3]
    assert list(L.plan_info("wgrad", rows, 10, 63)) == [128, 128, 3]  # Cout % 4 != 0 (S3)
    L.set_gemm_override("conv", 64, 64, 1000)
    assert list(L.plan_info("conv", M, N, K)) == [64, 64, ktiles(K)]
    L.set_gemm_override("wgrad", 64, 64, 1000)
    assert list(L.plan_info("wgrad", rows, Cout, Kdim)) == [64, 64, (rows + 31) // 32]
    for bad in ((256, 64, 1), (32, 64, 1), (64, 256, 1)):
        with pytest.raises(RuntimeError):
            L.set_gemm_override("conv", *bad)
    with pytest.raises(RuntimeError):
        L.set_gemm_override("fwd", 64, 64, 1)
