"""The GroupNorm block tail (csrc/kernels/gn.hip) at ResNet-50's four stage output shapes, 64 images, 32 groups:
`CF.group_norm_act(y, ..., relu=True, residual=r)` forward and backward, `--iters` times after a warm-up.

Run one stage per process under `rocprofv3 --kernel-trace --stats` for the per-launch times of the five kernels
(docs/PERF.md, "GroupNorm"); without a profiler it prints the device-event time of one forward + backward.

    python scripts/gn_cost.py --stage 1 [--iters 50] [--batch 64]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cs744_distributed_data_parallel_amd.ops import functional as CF  # noqa: E402

STAGES = {1: (256, 56), 2: (512, 28), 3: (1024, 14), 4: (2048, 7)}  # channels, map side


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--stage", type=int, choices=sorted(STAGES), required=True)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--groups", type=int, default=32)
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("gn_cost.py measures on the GPU; none found")
    C, side = STAGES[args.stage]
    torch.manual_seed(0)
    cl = lambda t: t.contiguous(memory_format=torch.channels_last)
    y = cl(torch.randn(args.batch, C, side, side, device="cuda")).requires_grad_()
    r = cl(torch.randn_like(y)).requires_grad_()
    w, b = torch.randn(C, device="cuda").requires_grad_(), torch.randn(C, device="cuda").requires_grad_()
    gout = cl(torch.randn_like(y))

    def once():
        for t in (y, r, w, b):
            t.grad = None
        CF.group_norm_act(y, w, b, args.groups, relu=True, residual=r).backward(gout)

    for _ in range(5):
        once()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.iters):
        once()
    t1.record()
    torch.cuda.synchronize()
    mb = y.numel() * 4 / 1e6
    print(f"stage {args.stage}: [{args.batch}, {C}, {side}, {side}] ({mb:.1f} MB per tensor), G = {args.groups}: "
          f"{t0.elapsed_time(t1) / args.iters * 1e3:.1f} us per forward + backward (host enqueue included)")


if __name__ == "__main__":
    main()
