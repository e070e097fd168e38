"""The two stem kernels of csrc/kernels/stem.hip -- stem_fwd_kernel and stem_wgrad_kernel<1..4> --
against float64 at tail shapes, through the fused block ops (conv_bn_act_fwd / conv_bn_act_bwd).

Method (tests/_stem_util.py). x, w, the exact conv and its per-element sum |x||w| come from
_gemm_util.conv_case; bias, gamma, beta, the running statistics and gout from a generator seeded
4000 (gout: 5000) + Cin + 7 N + 13 H + 17 W. Every reference is float64 on the CPU and starts from
what the kernel before it returned in fp32: the statistics from the returned y, out from y and the
returned stats, the backward from y, stats and gout. The host's path conditions are mirrored in
_stem_util.py and asserted before every launch; test_launch_log_confirms_the_mirrors runs a list of
the cases, every fallback among them, in a child process under CDP_GEMM_LOG=1 and compares the
stem_fwd / stem_wgrad records (and their absence) with the mirrors.

Covered
  forward   Cin 1..4 (the lo / hi channel split), a single pixel, all-border maps, an image
            boundary inside a 32-pixel half wave, exactly one block (the unmasked stores), a one-row
            statistics partial (M = 257), a tail block with one full and one single-pixel wave
            (M = 321), mean 1024 with a constant channel, 528 partials (bn_finalize instead of
            bn_fin_act); with and without bias; pool x relu on (3, 10, 6) and (5, 5, 7), relu alone
            on the single pixel (a 1x1 map has no 2x2 window)
  backward  stem_wgrad_kernel<1>, <2>, <3>, <4>; 1, 2, 3, 45 (= 4 * 11 + 1), 112 and 126 windows
            (the wok masks, the second unrolled group, two blocks), 65,792 windows (1,024 blocks, a
            third sweep that only 16 blocks take)
  fallbacks an odd map, no bias, need_dx (Cin 3 and 4, dx checked), no ReLU, no pool: the mirror
            says no stem_wgrad, the generic path meets the same bounds

Bounds (U = 2^-23 per fp32 rounding; derived in _stem_util.py and _bn_util.py)
  y         fp32_bound(sum |x||w| + |b|, 9 Cin + 1): the MFMA chain started from the bias
  mean      fp32_bound(sum |y|, 257) / M + U |mean|: a 256-term fp32 sum and a division per partial,
            merged in float64, rounded once
  var       [sum_b fp32_bound(Q_b, 258) + M Bm^2 + 2 sum_b (|tpm_b - mean| + d_b + Bm) cnt_b d_b] / M
            with d_b = gamma_258 sum_b |y| / cnt_b the partial mean's error: the two-pass M2 per
            partial and the Chan merge's cross term, which inexact partial means leave behind
  invstd    its rise at max(var - Bvar, 0), + U; scale 2 U, shift 5 U on top of the propagated bounds
  running   2^-22 (|(1 - f) rm| + |f mean|) + f (the statistic's bound); num_batches_tracked + 1
  out       U |ref| from the returned y and stats (one fmaf)
  dbeta, dgamma, db   _bn_util's, PS = 3: fp32_bound(sum |terms|, K), K = 4 ceil(windows / partials)
  dw        fp32_bound(sum |dy_ref||x|, M) + sum (dy bound + U |sc| (|k1| + |xhat k2|)) |x|
            + sum over ambiguous windows |sc||g||x|; the U term is the kernel's fl(1 / M)
  dx        (need_dx fallbacks) fp32_bound(sum |dy_ref||w|, 9 64) + the same sums against |w|
Routing closer than 2^-20 relative is excluded per element (share asserted <= 1e-5 per case).

Worst error / bound ratios seen on an MI355X (each test prints its own)
  forward   y 0.058 (0.10 with mean 1024), mean 0.0029, invstd 0.0039, scale 0.0046, shift 0.0030,
            running_mean 0.088, running_var 0.20, out 0.50 (one rounding is half of U); where the
            variance is 0 (the single pixel, the constant channel) the bound is the result's own
            rounding: invstd 0.35, scale 0.41, running_mean 0.25, running_var 0.23
  backward  stem path: dbeta 0.018, dgamma 0.066, db 0.29 and dw 0.047 (all at one to three windows;
            at 45 windows dw 0.0031, at 65,792 dw 3.3e-7: K = M carries that bound)
            fallbacks: dbeta 0.0061, dgamma 0.017, db 0.096, db over the odd map 0.0020, dw 0.0071,
            dx 0.00055
Ambiguous routing (bwd_ref on the returned y and stats): 0 in every small case; (2, 3, 514, 256)
44 of 16,842,752 elements (cap 168) -- the same count with torch's fp32 conv standing in for y on
the CPU. (33, 3, 64, 64) is a forward case: nothing is routed.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from _bn_util import Worst, fwd_path
from _gemm_util import lib
from _stem_util import (LOG_CASES, check_stem_bwd, check_stem_out, check_stem_stats, check_y, log_expectation,
                        run_stem_bwd, run_stem_fwd, stem_case, stem_case_gpu, stem_gout, stem_nparts,
                        stem_wgrad_blocks)

pytestmark = pytest.mark.gpu

CINS = [1, 2, 3, 4]
BIAS = [pytest.param(False, id="nobias"), pytest.param(True, id="bias")]
POOL_RELU = [pytest.param(p, r, id=f"{'pool' if p else 'nopool'}-{'relu' if r else 'lin'}")
             for p in (False, True) for r in (True, False)]


@pytest.fixture
def L():
    return lib()


def _state(g):
    return g.rm.clone(), g.rv.clone(), torch.zeros((), dtype=torch.long, device="cuda")


def _fwd(L, name, shape, Cin, bias, pool, relu, kind="normal", nparts=None, path=None, out=True):
    N, H, W = shape
    c = stem_case(N, Cin, H, W, kind)
    g = stem_case_gpu(c)
    if nparts is not None:
        assert stem_nparts(c.M) == nparts
    if path is not None:  # the BatchNorm kernels behind the stem's 256-row partials
        assert fwd_path(stem_nparts(c.M), 64) == path
    state = _state(g)
    state0 = (state[0].clone(), state[1].clone())
    r = run_stem_fwd(L, c, g, bias=bias, pool=pool, relu=relu, state=state)
    wst = Worst(f"{name} Cin={Cin} {shape} M={c.M}")
    check_y(wst, c, r)
    check_stem_stats(wst, c, r, state, state0)
    if out:
        check_stem_out(wst, c, r)
    wst.finish()


# ------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("pool,relu", POOL_RELU)
@pytest.mark.parametrize("bias", BIAS)
@pytest.mark.parametrize("Cin", CINS)
def test_fwd_every_cin(L, Cin, bias, pool, relu):
    """(3, ., 10, 6): 180 rows, one partial block; Cin 1..4 feeds the lo (h < Cin) and hi (2 + h <
    Cin) operands differently and zeroes the weight image's channels >= Cin."""
    _fwd(L, "every-cin", (3, 10, 6), Cin, bias, pool, relu, nparts=1, path="fin_act64")


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "lin"])
@pytest.mark.parametrize("bias", BIAS)
@pytest.mark.parametrize("Cin", CINS)
def test_fwd_one_pixel(L, Cin, bias, relu):
    """(1, ., 1, 1): only the centre tap is valid; M = 1 (variance 0, no unbiased correction)."""
    _fwd(L, "one-pixel", (1, 1, 1), Cin, bias, False, relu, nparts=1)


@pytest.mark.parametrize("pool,relu", POOL_RELU)
@pytest.mark.parametrize("bias", BIAS)
@pytest.mark.parametrize("Cin", CINS)
def test_fwd_image_boundary_in_half_wave(L, Cin, bias, pool, relu):
    """(5, ., 5, 7): 35 pixels per image, so every 32-pixel half wave decodes m -> (n, p, q) across
    an image boundary; pooled, the odd map leaves a border outside every window."""
    _fwd(L, "boundary", (5, 5, 7), Cin, bias, pool, relu, nparts=1)


@pytest.mark.parametrize("bias", BIAS)
@pytest.mark.parametrize("Cin", CINS)
@pytest.mark.parametrize("shape,nparts", [((2, 1, 9), 1), ((2, 9, 1), 1), ((1, 16, 16), 1), ((1, 1, 257), 2),
                                          ((1, 1, 321), 2)],
                         ids=["row-maps", "column-maps", "one-block", "M257", "M321"])
def test_fwd_borders_and_tails(L, shape, nparts, Cin, bias):
    """All-border maps; exactly one block (the `full` stores); M = 257: a second partial of one row
    (cnt = 1, M2 = 0, weight 1 / 257 in the merge) whose waves 1..3 hold no pixel; M = 321: a tail
    block with one full wave, one wave of a single pixel and two empty ones."""
    _fwd(L, "tails", shape, Cin, bias, False, True, nparts=nparts, path="fin_act64")


@pytest.mark.parametrize("pool,relu", [(True, True), (False, False)], ids=["pool-relu", "nopool-lin"])
@pytest.mark.parametrize("Cin", CINS)
def test_fwd_large_mean(L, Cin, pool, relu):
    """bias = 1024 on a conv of unit variance, channel 32 constant: the same bounds. (A one-pass
    variance loses 1024^2 2^-24 = 0.06 per term against a variance of 1.)"""
    _fwd(L, "large-mean", (3, 10, 6), Cin, True, pool, relu, kind="large_mean", nparts=1)


@pytest.mark.parametrize("bias", BIAS)
def test_fwd_past_512_partials(L, bias):
    """(33, 3, 64, 64): 528 partials of 256 rows, past bn_fin_act's 512: bn_finalize + bn_act_fwd."""
    _fwd(L, "528-partials", (33, 64, 64), 3, bias, True, True, nparts=528, path="finalize+act")


# ------------------------------------------------------------------------------ weight gradient
def _wgrad(L, name, shape, Cin, nblk=None):
    N, H, W = shape
    c = stem_case(N, Cin, H, W)
    g = stem_case_gpu(c)
    if nblk is not None:
        assert stem_wgrad_blocks(N, H, W) == nblk
    r = run_stem_fwd(L, c, g, bias=True, pool=True, relu=True)
    gout = stem_gout(c, True)
    b = run_stem_bwd(L, c, g, r, gout, need_dx=False, has_bias=True, expect_stem=True)
    wst = Worst(name)
    ref = check_stem_bwd(wst, c, r, b, gout)
    wst.name = f"{name} Cin={Cin} {shape} windows={N * (H // 2) * (W // 2)} ambiguous={ref.n_amb}/{ref.n_total}"
    wst.finish()


@pytest.mark.parametrize("Cin", CINS)
def test_wgrad_every_instantiation(L, Cin):
    """(3, ., 10, 6): 45 windows = 11 groups of 4 and one window; stem_wgrad_kernel<Cin>."""
    _wgrad(L, "wgrad-cin", (3, 10, 6), Cin, nblk=1)


@pytest.mark.parametrize("Cin", [3, 1])
def test_wgrad_one_window(L, Cin):
    """(1, ., 2, 2): lanes j > 0 of wave 0 and waves 1..3 contribute exact zeros."""
    _wgrad(L, "wgrad-one-window", (1, 2, 2), Cin, nblk=1)


@pytest.mark.parametrize("shape", [(1, 2, 4), (1, 2, 6), (5, 6, 6), (7, 8, 8)], ids=["w2", "w3", "w45", "w112"])
def test_wgrad_window_count_residues(L, shape):
    """2 and 3 windows (one masked group), 45 and 112 (a second unrolled group present, partial or
    whole): the wok masks."""
    _wgrad(L, "wgrad-residue", shape, 3)


def test_wgrad_several_blocks(L):
    """(2, 3, 18, 14): 126 windows, two blocks: the slab sum over blocks, 4 -> Cin columns."""
    _wgrad(L, "wgrad-blocks", (2, 18, 14), 3, nblk=2)


def test_wgrad_past_the_block_cap(L):
    """(2, 3, 514, 256): 65,792 windows = 16,448 groups over 1,024 blocks of 4 waves with 2 groups
    per sweep: two full sweeps and a third that only the first 64 waves take."""
    _wgrad(L, "wgrad-cap", (2, 514, 256), 3, nblk=1024)


# ------------------------------------------------------------------------------ fallbacks
FALLBACKS = [
    pytest.param((2, 7, 9), 3, dict(bias=True, pool=True, relu=True), False, id="odd-map"),
    pytest.param((3, 10, 6), 3, dict(bias=False, pool=True, relu=True), False, id="no-bias"),
    pytest.param((3, 10, 6), 3, dict(bias=True, pool=True, relu=True), True, id="need-dx-cin3"),
    pytest.param((3, 10, 6), 4, dict(bias=True, pool=True, relu=True), True, id="need-dx-cin4"),
    pytest.param((3, 10, 6), 3, dict(bias=True, pool=True, relu=False), False, id="no-relu"),
    pytest.param((3, 10, 6), 3, dict(bias=True, pool=False, relu=True), False, id="no-pool"),
]


@pytest.mark.parametrize("shape,Cin,fkw,need_dx", FALLBACKS)
def test_wgrad_fallbacks_meet_the_same_bounds(L, shape, Cin, fkw, need_dx):
    """What the stem weight gradient does not take goes through bn_bwd_apply (or the fused finalize)
    and the generic weight- and data-gradient GEMMs, at the bounds of the stem path."""
    N, H, W = shape
    c = stem_case(N, Cin, H, W)
    g = stem_case_gpu(c)
    r = run_stem_fwd(L, c, g, **fkw)
    gout = stem_gout(c, fkw["pool"])
    b = run_stem_bwd(L, c, g, r, gout, need_dx=need_dx, has_bias=fkw["bias"], expect_stem=False)
    wst = Worst("fallback")
    ref = check_stem_bwd(wst, c, r, b, gout)
    wst.name = f"fallback Cin={Cin} {shape} {fkw} need_dx={need_dx} ambiguous={ref.n_amb}/{ref.n_total}"
    wst.finish()


# ------------------------------------------------------------------------------ the mirrors
def test_launch_log_confirms_the_mirrors():
    """A fresh process under CDP_GEMM_LOG=1 (the flag is read once per process) runs LOG_CASES and
    prints the launch records: stem_fwd (M, 64, 9 Cin, 256, 64, 1) and stem_wgrad with the mirrored
    block count exactly where the mirrors say, and no stem_wgrad on any fallback."""
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, CDP_GEMM_LOG="1")
    env["PYTHONPATH"] = os.pathsep.join([os.path.dirname(tests), tests, env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", "import _stem_util; _stem_util.log_child()"], env=env,
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("STEM_LOG ")]
    assert len(line) == 1, r.stdout[-2000:]
    got = {name: (f, b) for name, f, b in json.loads(line[0][len("STEM_LOG "):])}
    assert list(got) == [n for n, *_ in LOG_CASES]
    n_fwd = n_wg = n_fallback = 0
    for name, shape, fkw, bkw in LOG_CASES:
        want_f, want_w = log_expectation(shape, fkw, bkw)
        frec, brec = got[name]
        stem_f = [t for t in frec if t[0] == "stem_fwd"]
        assert stem_f == ([want_f] if want_f else []), (name, frec)
        if want_f:  # the stem forward launches no GEMM besides
            assert frec == [want_f], (name, frec)
            n_fwd += 1
        else:
            assert frec and all(t[0] == "fwd" for t in frec), (name, frec)
        if bkw is None:
            continue
        stem_w = [t for t in brec if t[0] == "stem_wgrad"]
        assert stem_w == ([want_w] if want_w else []), (name, brec)
        if want_w:
            assert brec == [want_w], (name, brec)
            n_wg += 1
        else:  # the generic weight gradient ran instead (alone, or paired with the data gradient)
            assert any(t[0] in ("wgrad", "pair_wgrad") for t in brec), (name, brec)
            n_fallback += 1
    assert (n_fwd, n_wg, n_fallback) == (13, 6, 6)
