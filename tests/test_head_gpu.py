"""The classifier-head kernels of csrc/kernels/misc.hip against float64 at their edges: the narrow
Linear (small_linear_fwd / small_linear_bwd, O <= 16) and the O = 17 switch to the GEMM + colsum
path, the fused cross-entropy + Linear backward with its BatchNorm link (xent_linear_bwd_kernel),
and the global average pool, forward and backward.

Method. The native ops are called directly (linear_fwd, linear_bwd, xent_linear_bwd; the pool
through ops.functional). References are float64 on the CPU; where a quantity is formed from
another kernel output the reference starts from that fp32 output: dx, dw, db of the fused backward
from the kernel's own dlogits, the link's partials from the kernel's own dx.

Covered
  Linear    (B, I, O) = (1, 1, 1), (5, 63, 1), (7, 65, 16), (33, 500, 10), (4, 512, 16) and
            (37, 130, 17): O = 1 and 16, I off every multiple of 16 and 64, the GEMM's row tail;
            with and without bias, with and without dx
  fused     (1, 20, 2), (31, 20, 10), (33, 20, 10), (33, 512, 10), (512, 36, 16) -- B O = 8,192 =
            kXentLinMax exactly; no link, and links pooled or not, ps 2 or 3, with or without ReLU;
            B = 33 leaves a second 32-row chunk of one row; without dx; without bias
  avg pool  (N, H, W, C) = (1, 1, 1, 4), (3, 7, 7, 20), (2, 5, 3, 2048)

Bounds (U = 2^-23 per fp32 rounding; fp32_bound(a, K) = 4 (2^-22 + K 2^-24) a)
  y         fp32_bound(sum |x||w| + |b|, I + 1)
  dx        fp32_bound(sum |dy||w|, O);  dw fp32_bound(sum |dy||x|, B);  db fp32_bound(sum |dy|, B)
  dlogits   1e-7 + 1e-5 |ref| against the float64 softmax gradient: test_fused_tail_gpu.py's
            tolerance for this quantity (expf's error is the library's)
  part      [ceil(B / 32), I, ps]; each 32-row chunk against _bn_util.bwd_ref on its rows of link_y,
            the link's stats and the kernel's dx: fp32_bound(sum |terms|, 32), x 4 pooled, + the
            ambiguous routings' slack (none occurred; cap 1e-5 per chunk)
  avg pool  forward fp32_bound(sum |x|, HW) / HW + U |ref|; backward 2 U |ref| (reciprocal, product)

Worst error / bound ratios seen on an MI355X (each test prints its own)
  Linear    y 0.039, dx 0.061, dw 0.078, db 0.030
  fused     dlogits 0.0073, dx 0.071, dw 0.049, db 0.0055; part: sum dz 0.013, sum dz xhat 0.016,
            sum xhat 0.012; ambiguous routing 0 in every chunk
  avg pool  y 0.032, dx 0.47 (one rounding is half of U)
"""
import pytest
import torch

from _bn_util import EPS, U, Worst, bwd_ref
from _gemm_util import cl, fp32_bound, lib

pytestmark = pytest.mark.gpu

SL_MAXO = 16        # misc.hip: the narrow kernels serve O <= 16
XENT_LIN_MAX = 8192  # kernels.h kXentLinMax: B * O the fused backward holds in LDS
XENT_ROWS = 32      # kernels.h kXentLinRows: dX rows per block and per BN partial


@pytest.fixture
def L():
    return lib()


def linear_path(O):
    """linear_fwd / linear_bwd (ops.cpp): the narrow kernels, or the conv GEMM (+ colsum for db)."""
    return "small" if O <= SL_MAXO else "gemm"


def _lin_data(B, I, O, seed):
    gen = torch.Generator().manual_seed(seed + B + 7 * I + 13 * O)
    x = torch.randn(B, I, generator=gen)
    w = torch.randn(O, I, generator=gen) / I ** 0.5
    b = torch.randn(O, generator=gen)
    gy = torch.randn(B, O, generator=gen)
    return x, w, b, gy


def _check_linear_grads(wst, dy, x, w, dx, dw, db):
    """dx, dw, db as float64 products of dy (fp32, CPU) at the dot-product bounds of their lengths."""
    B, O = dy.shape
    dyd, xd, wd = dy.double(), x.double(), w.double()
    if dx is not None:
        wst.add("dx", dx, dyd @ wd, fp32_bound(dyd.abs() @ wd.abs(), O))
    wst.add("dw", dw, dyd.t() @ xd, fp32_bound(dyd.abs().t() @ xd.abs(), B))
    if db is not None:
        wst.add("db", db, dyd.sum(0), fp32_bound(dyd.abs().sum(0), B))


# ------------------------------------------------------------------------------ narrow Linear
@pytest.mark.parametrize("need_dx", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,I,O,path", [(1, 1, 1, "small"), (5, 63, 1, "small"), (7, 65, 16, "small"),
                                        (33, 500, 10, "small"), (4, 512, 16, "small"), (37, 130, 17, "gemm")])
def test_linear(L, B, I, O, path, bias, need_dx):
    assert linear_path(O) == path
    x, w, b, gy = _lin_data(B, I, O, 100)
    xg, wg, bg = x.cuda(), w.cuda(), (b.cuda() if bias else None)
    wst = Worst(f"linear {(B, I, O)} {path}")
    y = L.linear_fwd(xg, wg, bg)
    xd, wd = x.double(), w.double()
    ref = xd @ wd.t() + (b.double() if bias else 0.0)
    absref = xd.abs() @ wd.abs().t() + (b.double().abs() if bias else 0.0)
    wst.add("y", y, ref, fp32_bound(absref, I + 1))
    dx, dw, db = L.linear_bwd(gy.cuda(), xg, wg, need_dx, bias)
    assert (dx is not None) == need_dx and (db is not None) == bias
    _check_linear_grads(wst, gy, x, w, dx, dw, db)
    wst.finish()


# ------------------------------------------------------------------------------ fused xent + Linear backward
def _link_data(B, I, pool, seed):
    """The linked block's pre-BN output y [B, I, hw, hw] (channels_last) and its fp32 stats block."""
    gen = torch.Generator().manual_seed(seed)
    hw = 2 if pool else 1
    y = torch.randn(B, I, hw, hw, generator=gen)
    g, bt = 0.5 + torch.rand(I, generator=gen), torch.randn(I, generator=gen)
    mu = y.mean((0, 2, 3))
    istd = 1.0 / torch.sqrt(y.var((0, 2, 3), unbiased=False) + EPS) if B * hw * hw > 1 else torch.ones(I)
    stats = torch.stack([mu, istd, g * istd, bt - mu * g * istd]).contiguous()
    return y, stats


LINKS = {None: "nolink", (False, 2, True): "link-ps2-relu", (True, 3, True): "link-pool-ps3-relu",
         (True, 2, False): "link-pool-ps2-lin", (False, 3, False): "link-ps3-lin", (True, 2, True): "link-pool-ps2-relu",
         (False, 3, True): "link-ps3-relu"}
XENT_CASES = [
    # B, I, O, link (pool, ps, relu), need_dx, bias
    (1, 20, 2, None, True, True), (1, 20, 2, (False, 2, True), True, True), (1, 20, 2, None, False, False),
    (31, 20, 10, None, True, False), (31, 20, 10, (True, 3, True), True, True),
    (33, 20, 10, (False, 2, True), True, True), (33, 20, 10, (True, 3, True), True, True),
    (33, 20, 10, (True, 2, False), True, True), (33, 20, 10, (False, 3, False), True, False),
    (33, 512, 10, None, False, True), (33, 512, 10, (True, 3, True), True, True),
    (512, 36, 16, None, True, True), (512, 36, 16, (True, 2, True), True, True),
    (512, 36, 16, (False, 3, True), True, True),
]


@pytest.mark.parametrize("B,I,O,link,need_dx,bias", XENT_CASES,
                         ids=[f"{B}x{I}x{O}-{LINKS[lk]}-{'dx' if nd else 'nodx'}-{'bias' if bs else 'nobias'}"
                              for B, I, O, lk, nd, bs in XENT_CASES])
def test_xent_linear_bwd(L, B, I, O, link, need_dx, bias):
    assert O <= SL_MAXO and B * O <= XENT_LIN_MAX
    x, w, b, _ = _lin_data(B, I, O, 200)
    gen = torch.Generator().manual_seed(300 + B + I + O)
    t = torch.randint(0, O, (B,), generator=gen)
    xg, wg = x.cuda(), w.cuda()
    logits = L.linear_fwd(xg, wg, b.cuda() if bias else None)  # the forward's own fp32 logits
    gloss = torch.tensor(0.5, device="cuda")                   # a non-unit incoming gradient
    kw = {}
    if link is not None:
        pool, ps, relu = link
        ly, lst = _link_data(B, I, pool, 400 + B + I)
        kw = dict(link_y=cl(ly.cuda()), link_stats=lst.cuda(), link_pool=pool, link_relu=relu, link_ps=ps)
    dl, dx, dw, db, part = L.xent_linear_bwd(gloss, logits, t.cuda(), xg, wg, need_dx, bias, **kw)
    wst = Worst(f"xent_linear_bwd {(B, I, O)} {LINKS[link]}")
    # dlogits = (softmax - onehot) gloss / B
    ld = logits.double().cpu()
    ref = (torch.softmax(ld, 1) - torch.nn.functional.one_hot(t, O).double()) * 0.5 / B
    wst.add("dlogits", dl, ref, 1e-7 + 1e-5 * ref.abs())
    assert (dx is not None) == need_dx and (db is not None) == bias
    _check_linear_grads(wst, dl.cpu(), x, w, dx, dw, db)
    if link is None:
        assert part is None
        wst.finish()
        return
    nchunk = (B + XENT_ROWS - 1) // XENT_ROWS
    assert tuple(part.shape) == (nchunk, I, ps)
    dxc, n_amb = dx.cpu(), 0
    K = XENT_ROWS * (4 if pool else 1)
    for k in range(nchunk):
        rows = slice(XENT_ROWS * k, min(B, XENT_ROWS * (k + 1)))
        r = bwd_ref(ly[rows], lst, dxc[rows].view(-1, I, 1, 1), pool, relu)  # asserts the ambiguity cap
        n_amb += r.n_amb
        got = part[k].double().cpu()
        wst.add(f"S0[{k}]", got[:, 0], r.S0, fp32_bound(r.A0, K) + r.slack0)
        wst.add(f"S1[{k}]", got[:, 1], r.S1, fp32_bound(r.A1, K) + r.slack1)
        if ps == 3:
            wst.add(f"S2[{k}]", got[:, 2], r.S2, fp32_bound(r.A2, K))
    if B % XENT_ROWS == 1:
        assert rows.stop - rows.start == 1  # the last chunk holds one row
    # one figure per quantity: the worst chunk's (a NaN ratio outranks every number)
    worst = {}
    for what, v in wst.items:
        worst.setdefault(what.split("[")[0], []).append(v)
    wst.items = [(what, max(vs, key=lambda v: float("inf") if v != v else v)) for what, vs in worst.items()]
    wst.name += f" chunks={nchunk} ambiguous={n_amb}"
    wst.finish()


# ------------------------------------------------------------------------------ global average pool
@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 4), (3, 7, 7, 20), (2, 5, 3, 2048)])
def test_global_avg_pool(L, N, H, W, C):
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    gen = torch.Generator().manual_seed(500 + N + H + W + C)
    x = torch.randn(N, C, H, W, generator=gen)
    gy = torch.randn(N, C, generator=gen)
    xg = cl(x.cuda()).requires_grad_()
    assert CF.use_native(xg), "global_avg_pool would not take the native kernels"
    y = CF.global_avg_pool(xg)
    y.backward(gy.cuda())
    HW = H * W
    xd = x.double()
    ref = xd.mean((2, 3))
    wst = Worst(f"avgpool {(N, H, W, C)}")
    wst.add("y", y.detach(), ref, fp32_bound(xd.abs().sum((2, 3)), HW) / HW + U * ref.abs())
    gref = (gy.double() / HW).view(N, C, 1, 1).expand(N, C, H, W)
    wst.add("dx", xg.grad, gref, 2 * U * gref.abs())
    wst.finish()
