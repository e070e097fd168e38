"""The grouped 3x3 conv kernels (csrc/kernels/gconv.hip) at the grouped layers of `resnext50_32x4d`, 64 images of
224 x 224, beside `F.conv2d(groups=32)` of stock PyTorch-ROCm on the same tensors, and one eager training step of
a model under both backends (docs/PERF.md, "Grouped convolution").

    python scripts/gconv_cost.py --layers [--batch 64] [--reps 3]
    python scripts/gconv_cost.py --step resnext50_32x4d [--backend native|torch] [--batch 64]

Times are device events around `iters` back-to-back calls (at least 0.2 s of work), the two sides alternating,
the best of `reps`; bytes are what a kernel must move once (its two activations and the weight)."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (C, input side, stride) of conv2 in layer1 .. layer4: the first block of layers 2-4 strides, the others do not
LAYERS = [(128, 56, 1), (256, 56, 2), (256, 28, 1), (512, 28, 2), (512, 14, 1), (1024, 14, 2), (1024, 7, 1)]


def timed(fn, min_s=0.2):
    """us per call by device events; iters sized from a first timed call so the window is >= min_s."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    iters = max(10, int(min_s * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def layers(args):
    from cs744_distributed_data_parallel_amd import _native

    L, G = _native.lib(), 32
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    print("| C | map | stride | op | bytes (MB) | gconv (us) | GB/s | F.conv2d (us) |")
    print("|---|---|---|---|---|---|---|---|")
    for C, side, s in LAYERS:
        torch.manual_seed(0)
        x = cl(torch.randn(args.batch, C, side, side, device="cuda"))
        w = cl(torch.randn(C, C // G, 3, 3, device="cuda") * 0.05)
        y = L.gconv2d_fwd(x, w, None, s, 1, G, False)[0]
        gy = cl(torch.randn_like(y))
        xr, wr = x.clone().requires_grad_(), w.clone().requires_grad_()
        shape_x, shape_w = list(x.shape), list(w.shape)
        mb = lambda *ts: sum(t.numel() for t in ts) * 4 / 1e6
        ops = {
            "fwd": (lambda: L.gconv2d_fwd(x, w, None, s, 1, G, True), lambda: F.conv2d(x, w, None, s, 1, 1, G),
                    mb(x, y, w)),
            "dgrad": (lambda: L.gconv2d_dgrad(gy, w, shape_x, s, 1, G, None),
                      lambda: torch.autograd.grad(F.conv2d(xr, w, None, s, 1, 1, G), xr, gy), mb(gy, x, w)),
            "wgrad": (lambda: L.gconv2d_wgrad(gy, x, shape_w, s, 1, G, None, False),
                      lambda: torch.autograd.grad(F.conv2d(x, wr, None, s, 1, 1, G), wr, gy), mb(gy, x, w)),
        }
        for name, (ours, stock, mbytes) in ops.items():
            a, b = [], []
            for _ in range(args.reps):  # alternating
                a.append(timed(ours))
                b.append(timed(stock))
            stock_us = min(b) - (timed(lambda: F.conv2d(x, w, None, s, 1, 1, G)) if name != "fwd" else 0.0)
            note = "" if name == "fwd" else " (backward alone: forward + backward minus forward)"
            print(f"| {C} | {side} | {s} | {name} | {mbytes:.1f} | {min(a):.1f} | {mbytes / min(a) * 1e3:.0f} | "
                  f"{stock_us:.1f}{note} |")


def step(args):
    if args.backend == "torch":
        os.environ["CDP_FORCE_REFERENCE"] = "1"
    import cs744_distributed_data_parallel_amd as cdp

    torch.manual_seed(0)
    model = cdp.get_model(args.step).cuda().to(memory_format=torch.channels_last)
    native = args.backend == "native"
    opt = (cdp.SGD if native else torch.optim.SGD)(model.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    crit = cdp.CrossEntropyLoss() if native else torch.nn.CrossEntropyLoss()
    x = torch.randn(args.batch, 3, 224, 224, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (args.batch,), device="cuda")

    def once():
        opt.zero_grad()
        crit(model(x), y).backward()
        opt.step()

    for _ in range(5):
        once()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            once()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / args.iters)
    print(f"STEP {args.step} {args.backend} batch {args.batch}: " + ", ".join(f"{t:.2f}" for t in times)
          + f" ms per eager step ({args.batch / min(times) * 1e3:.0f} img/s at the best)")


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
        raise SystemExit("gconv_cost.py measures on the GPU; none found")
    if args.layers:
        layers(args)
    if args.step:
        step(args)


if __name__ == "__main__":
    main()
