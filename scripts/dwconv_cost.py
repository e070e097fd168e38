"""The depthwise 3x3 conv kernels (csrc/kernels/dwconv.hip) at the 13 depthwise layers of `mobilenet_v1`, 64 images
of 224 x 224, beside `F.conv2d(groups=C)` of stock PyTorch-ROCm on the same tensors, and one eager training step of
a model under both backends (docs/PERF.md, "Depthwise convolution").

    python scripts/dwconv_cost.py --layers [--batch 64] [--reps 3]
    python scripts/dwconv_cost.py --step mobilenet_v1 [--backend native|torch] [--batch 64]

Times are device events around `iters` back-to-back calls (at least 0.2 s of work), the two sides alternating,
the best of `reps`; bytes are what a kernel must move once (its two activations and the weight)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gconv_cost import step, timed  # noqa: E402  (the same timing method and the same eager step)

# (C, input side, stride) of blocks.0 .. blocks.12's depthwise conv
LAYERS = [(32, 112, 1), (64, 112, 2), (128, 56, 1), (128, 56, 2), (256, 28, 1), (256, 28, 2), (512, 14, 1),
          (512, 14, 1), (512, 14, 1), (512, 14, 1), (512, 14, 1), (512, 14, 2), (1024, 7, 1)]


def layers(args):
    from cs744_distributed_data_parallel_amd import _native

    L = _native.lib()
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    print("| block | C | map | stride | op | bytes (MB) | dwconv (us) | GB/s | F.conv2d (us) |")
    print("|---|---|---|---|---|---|---|---|---|")
    seen = {}
    for i, (C, side, s) in enumerate(LAYERS):
        if (C, side, s) in seen:  # blocks 6 .. 10 are one shape: measured once
            print(f"| {i} | {C} | {side} | {s} | as block {seen[(C, side, s)]} | | | | |")
            continue
        seen[(C, side, s)] = i
        torch.manual_seed(0)
        x = cl(torch.randn(args.batch, C, side, side, device="cuda"))
        w = torch.randn(C, 1, 3, 3, device="cuda") / 3.0
        y = L.dwconv2d_fwd(x, w, None, s, 1, False)[0]
        gy = cl(torch.randn_like(y))
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
        shape_x, shape_w = list(x.shape), list(w.shape)
        mb = lambda *ts: sum(t.numel() for t in ts) * 4 / 1e6
        fwd = lambda: F.conv2d(x, w, None, s, 1, 1, C)
        ops = {
            "fwd": (lambda: L.dwconv2d_fwd(x, w, None, s, 1, True), fwd, mb(x, y, w)),
            "dgrad": (lambda: L.dwconv2d_dgrad(gy, w, shape_x, s, 1, None),
                      lambda: torch.autograd.grad(F.conv2d(xr, w, None, s, 1, 1, C), xr, gy), mb(gy, x, w)),
            "wgrad": (lambda: L.dwconv2d_wgrad(gy, x, shape_w, s, 1, None, False),
                      lambda: torch.autograd.grad(F.conv2d(x, wr, None, s, 1, 1, C), wr, gy), mb(gy, x, w)),
        }
        for name, (ours, stock, mbytes) in ops.items():
            a, b = [], []
            for _ in range(args.reps):  # alternating
                a.append(timed(ours))
                b.append(timed(stock))
            stock_us = min(b) - (timed(fwd) if name != "fwd" else 0.0)
            note = "" if name == "fwd" else " (backward alone: forward + backward minus forward)"
            print(f"| {i} | {C} | {side} | {s} | {name} | {mbytes:.1f} | {min(a):.1f} | {mbytes / min(a) * 1e3:.0f} | "
                  f"{stock_us:.1f}{note} |", flush=True)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--layers", action="store_true")
    p.add_argument("--step", default=None, help="a model name: one eager training step")
    p.add_argument("--backend", default="native", choices=["native", "torch"])
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--iters", type=int, default=20)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_cost.py measures on the GPU; none found")
    if args.layers:
        layers(args)
    if args.step:
        step(args)


if __name__ == "__main__":
    main()
