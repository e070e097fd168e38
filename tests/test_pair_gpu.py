"""The paired gradient launch (csrc/kernels/bwd_pair.h: a block's data- and weight-gradient GEMMs in
one grid) against the two separate launches (CDP_BWD_PAIR=0, read on every call) and against fp64.

* At the VGG-11 layer shapes of the bench (256 images) and of the reference's strong-scaling
  points (128 / 64 / 32 images at W = 2 / 4 / 8, /root/reference/src/Part 2a/main.py:22) -- each
  under its plans, the tuned-plan table's included -- the pair is really taken (the runtime's
  launch counter moves), and dX / dW equal the unpaired launches' (and, for the unpooled layers,
  torch fp64's).
* An NCHW-contiguous input that needs a gradient: the weight-gradient GEMM held back for the pair
  reads a channels_last copy of x and |max| partials made inside the backward call; both must stay
  alive until the paired launch is enqueued (else dX, allocated in between, may reuse their memory).
* Every paired instantiation -- the planner reaches only the pairs that beat its cost model -- forced
  through set_gemm_override on a small block whose two GEMMs have M and N tails under every tile.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

VGG_LAYERS = [(64, 128, 16), (128, 256, 8), (256, 256, 8), (256, 512, 4), (512, 512, 4), (512, 512, 2),
              (512, 512, 2)]
POOL_AFTER = {1, 3, 5, 7}  # VGG-11 blocks followed by 'M' (cfg, models/vgg.py)


def _lib():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


def _block(Ci, Co, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(Ci, Co, 3, padding=1).cuda()
    conv.weight.data = conv.weight.data.contiguous(memory_format=torch.channels_last)
    bn = torch.nn.BatchNorm2d(Co).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    return conv, bn


def _grads(monkeypatch, pair, x, conv, bn, pool, gy, relu=True):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    monkeypatch.setenv("CDP_BWD_PAIR", "1" if pair else "0")
    xr = x.detach().clone().requires_grad_()
    for p in (conv.weight, conv.bias, bn.weight, bn.bias):
        p.grad = None
    n0 = _lib().pair_launches()
    out = CF.conv_bn_act(xr, conv, bn, relu=relu, pool=pool)
    out.backward(gy)
    torch.cuda.synchronize()
    return xr.grad.clone(), conv.weight.grad.clone(), _lib().pair_launches() - n0


def _fp64(x, conv, bn, pool, gy, relu=True):
    xd = x.double().detach().requires_grad_()
    wd = conv.weight.double().detach().requires_grad_()
    y = F.conv2d(xd, wd, conv.bias.double(), 1, 1)
    y = F.batch_norm(y, None, None, bn.weight.double(), bn.bias.double(), True, 0.0, bn.eps)
    if relu:
        y = F.relu(y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    y.backward(gy.double())
    return xd.grad, wd.grad


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


@pytest.mark.parametrize("B", [256, 128, 64, 32])
@pytest.mark.parametrize("layer", range(1, 8))
def test_paired_gradients_match_separate_launches_and_fp64(monkeypatch, B, layer):
    lib = _lib()
    orig = lib.get_conv_gemm()
    try:
        lib.set_conv_gemm("f16x2")
        Ci, Co, HW = VGG_LAYERS[layer - 1]
        conv, bn = _block(Ci, Co, 10 + layer)
        pool = layer in POOL_AFTER
        x = torch.relu(torch.randn(B, Ci, HW, HW, device="cuda")).contiguous(memory_format=torch.channels_last)
        oh = HW // 2 if pool else HW
        gy = torch.randn(B, Co, oh, oh, device="cuda").contiguous(memory_format=torch.channels_last)
        dx_p, dw_p, n_pair = _grads(monkeypatch, True, x, conv, bn, pool, gy)
        dx_s, dw_s, n_sep = _grads(monkeypatch, False, x, conv, bn, pool, gy)
    finally:
        lib.set_conv_gemm(orig)
    assert n_pair == 1 and n_sep == 0, (n_pair, n_sep)
    # same tiles, same split-K partition, same reduction order: the pair changes only which
    # workgroup runs which tile
    assert _rel(dx_p, dx_s) <= 1e-6 and _rel(dw_p, dw_s) <= 1e-6, (_rel(dx_p, dx_s), _rel(dw_p, dw_s))
    if pool:
        # max-pool backward routes each window's gradient to its argmax and ReLU's to the elements
        # above 0: an element within fp32 rounding of its window's maximum, or of 0, can be routed
        # differently than in fp64 (~1 such element per 2M at 256 images: rel-L2 ~1e-3 for every
        # engine, torch fp32 included when it happens; scripts/diag/pair_accuracy.py). The fp64
        # comparison therefore runs on the unpooled layers without the ReLU (the pair's GEMMs and
        # the BatchNorm backward, no discontinuous routing)
        return
    dx_p, dw_p, n_lin = _grads(monkeypatch, True, x, conv, bn, pool, gy, relu=False)
    assert n_lin == 1
    dx_r, dw_r = _fp64(x, conv, bn, pool, gy, relu=False)
    e_dx, e_dw = _rel(dx_p, dx_r.cuda()), _rel(dw_p, dw_r.cuda())
    print(f"B={B} layer {layer}: paired vs fp64 rel-L2 dX {e_dx:.2e} dW {e_dw:.2e}")
    assert e_dx <= 1e-5 and e_dw <= 1e-5, (e_dx, e_dw)


def test_held_weight_gradient_keeps_its_nchw_input_alive(monkeypatch):
    lib = _lib()
    orig = lib.get_conv_gemm()
    try:
        lib.set_conv_gemm("f16x2")
        conv, bn = _block(128, 256, 3)
        x = torch.relu(torch.randn(64, 128, 8, 8, device="cuda"))  # NCHW-contiguous, not channels_last
        assert not x.is_contiguous(memory_format=torch.channels_last)
        gy = torch.randn(64, 256, 8, 8, device="cuda")
        res = []
        for pair in (True, False):
            # several rounds so the caching allocator has freed blocks of x's size to hand out
            for _ in range(3):
                dx, dw, n = _grads(monkeypatch, pair, x, conv, bn, False, gy, relu=False)
            res.append((dx, dw, n))
    finally:
        lib.set_conv_gemm(orig)
    (dx_p, dw_p, n_p), (dx_s, dw_s, n_s) = res
    assert n_p == 1 and n_s == 0
    assert _rel(dx_p, dx_s) <= 1e-6 and _rel(dw_p, dw_s) <= 1e-6, (_rel(dx_p, dx_s), _rel(dw_p, dw_s))
    dx_r, dw_r = _fp64(x, conv, bn, False, gy, relu=False)
    assert _rel(dw_p, dw_r.cuda()) <= 1e-5 and _rel(dx_p, dx_r.cuda()) <= 1e-5


def test_tuned_plans_are_the_planners_choice():
    """The tuned-plan table (csrc/runtime/ops.cpp, tuned_plans()) is what the planner returns for its
    shapes, per GEMM kind: VGG-11 block 5 at 32 images (512->512 at 4x4: M = 512, K = 4608) takes
    128x128 data-gradient tiles over 6 splits while its forward GEMM of the same M, N, K keeps the
    fitted model's plan."""
    lib = _lib()
    orig = lib.get_conv_gemm()
    try:
        lib.set_conv_gemm("f16x2")
        assert list(lib.plan_info("dgrad", 512, 512, 4608)) == [128, 128, 6]
        assert list(lib.plan_info("conv", 512, 512, 4608)) != [128, 128, 6]
        assert list(lib.plan_info("wgrad", 4096, 512, 2304)) == [256, 128, 4]
        lib.set_conv_gemm("x3")  # the table is per engine: x3 keeps its planner's plans
        assert list(lib.plan_info("dgrad", 512, 512, 4608)) == list(lib.plan_info("conv", 512, 512, 4608))
    finally:
        lib.set_conv_gemm(orig)


# ------------------------------------------------------------- every paired instantiation
# The 16 pairs of 256-thread tiles ({64, 128} x {64, 128} data-gradient tiles beside the same four
# weight-gradient tiles, bwd_pair_d*.hip) and the 512-thread 256x128 pair (bwd_pair.hip), forced
# through set_gemm_override on a block whose GEMMs have M and N tails under every tile: 96 -> 160
# channels, 3 images of 10x10 (data gradient M 300, N 96, K 1440; weight gradient 160 x 864 over 300
# rows = ten 32-row steps, the last one 12 rows). The conv override also moves the block's forward
# GEMM to the same tile, which changes nothing that is compared here.
TAIL_BLOCK = (3, 96, 160, 10)  # N, Ci, Co, HW
TILES4 = [(64, 64), (64, 128), (128, 64), (128, 128)]
PAIRS = [(d, w) for d in TILES4 for w in TILES4] + [((256, 128), (256, 128))]


@functools.lru_cache(maxsize=None)
def _tail_block():
    N, Ci, Co, HW = TAIL_BLOCK
    conv, bn = _block(Ci, Co, 31)
    x = torch.relu(torch.randn(N, Ci, HW, HW, device="cuda")).contiguous(memory_format=torch.channels_last)
    gy = torch.randn(N, Co, HW, HW, device="cuda").contiguous(memory_format=torch.channels_last)
    dx_r, dw_r = _fp64(x, conv, bn, False, gy, relu=False)
    return conv, bn, x, gy, dx_r.cuda(), dw_r.cuda()


def _forced_tail_grads(monkeypatch, dtile, wtile, splits):
    """(dX, dW, paired launches) of the tail block with and without the pair under forced plans."""
    N, Ci, Co, HW = TAIL_BLOCK
    conv, bn, x, gy, _, _ = _tail_block()
    lib = _lib()
    orig = lib.get_conv_gemm()
    try:
        lib.set_conv_gemm("f16x2")
        lib.set_gemm_override("conv", *dtile, splits)
        lib.set_gemm_override("wgrad", *wtile, splits)
        assert list(lib.plan_info("dgrad", N * HW * HW, Ci, 9 * Co)) == [*dtile, splits]
        assert list(lib.plan_info("wgrad", N * HW * HW, Co, 9 * Ci)) == [*wtile, splits]
        paired = _grads(monkeypatch, True, x, conv, bn, False, gy, relu=False)
        separate = _grads(monkeypatch, False, x, conv, bn, False, gy, relu=False)
    finally:
        lib.set_conv_gemm(orig)
        lib.set_gemm_override("conv", 0, 0, 0)
        lib.set_gemm_override("wgrad", 0, 0, 0)
    return paired, separate


@pytest.mark.parametrize("splits", [1, 3])
@pytest.mark.parametrize("dtile,wtile", [pytest.param(d, w, id=f"d{d[0]}x{d[1]}-w{w[0]}x{w[1]}") for d, w in PAIRS])
def test_every_paired_instantiation_at_tail_shape(monkeypatch, dtile, wtile, splits):
    (dx_p, dw_p, n_pair), (dx_s, dw_s, n_sep) = _forced_tail_grads(monkeypatch, dtile, wtile, splits)
    assert n_pair == 1 and n_sep == 0, (n_pair, n_sep)
    # the tolerances of test_paired_gradients_match_separate_launches_and_fp64, for its reasons
    assert _rel(dx_p, dx_s) <= 1e-6 and _rel(dw_p, dw_s) <= 1e-6, (_rel(dx_p, dx_s), _rel(dw_p, dw_s))
    _, _, _, _, dx_r, dw_r = _tail_block()
    e_dx, e_dw = _rel(dx_p, dx_r), _rel(dw_p, dw_r)
    assert e_dx <= 1e-5 and e_dw <= 1e-5, (e_dx, e_dw)


@pytest.mark.parametrize("dtile,wtile", [((256, 128), (128, 128)), ((128, 128), (256, 128))],
                         ids=["d256x128-w128x128", "d128x128-w256x128"])
def test_mixed_workgroup_sizes_are_not_paired(monkeypatch, dtile, wtile):
    """A 512-thread tile beside a 256-thread one has no paired kernel (bwd_pair_ok): the two GEMMs
    run as separate launches, and the gradients are still right."""
    (dx_p, dw_p, n_pair), (dx_s, dw_s, n_sep) = _forced_tail_grads(monkeypatch, dtile, wtile, 3)
    assert n_pair == 0 and n_sep == 0, (n_pair, n_sep)
    assert _rel(dx_p, dx_s) <= 1e-6 and _rel(dw_p, dw_s) <= 1e-6
    _, _, _, _, dx_r, dw_r = _tail_block()
    assert _rel(dx_p, dx_r) <= 1e-5 and _rel(dw_p, dw_r) <= 1e-5, (_rel(dx_p, dx_r), _rel(dw_p, dw_r))
