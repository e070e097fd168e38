#!/usr/bin/env python
"""Cost of mixup / CutMix in the two places it touches (docs/PERF.md, "Batch mixing").

Times, at the benchmark's two shapes (256 x 32^2 with 10 classes, 64 x 224^2 with 1000 classes):
  * the augment launch with mixing off, and with it forced to each mode (none / mixup / cutmix);
  * the loss forward + backward (xent_fwd + xent_bwd; the standalone kernels, no classifier fusion)
    with one target and with a target pair.
Every variant is a captured hipGraph of ``--inner`` back-to-back calls; after a warm-up the variants are
timed in alternation (round-robin blocks of replays, host clock around replays that end in a device
synchronise), so all of them see the same box in the same minutes. In a tree without the mixing
kernels (the parent commit) only the unmixed variants are timed, under the same names, so the two
trees' records compare directly.

    python scripts/mix_cost.py [--rounds 10] [--block 5] [--inner 50] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(name="256x32^2", B=256, S=32, classes=10), dict(name="64x224^2", B=64, S=224, classes=1000)]
# forced modes: prob / switch_prob pick the mode with certainty
MODES = {"mix:none": dict(mixup_alpha=1.0, mix_prob=0.0), "mix:mixup": dict(mixup_alpha=1.0),
         "mix:cutmix": dict(cutmix_alpha=1.0)}


def capture(torch, fn, inner):
    for _ in range(3):
        fn()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [fn() for _ in range(inner)]
    torch.cuda.synchronize()
    return g, keep


def variants(cdp, torch, shape, has_mix):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, synthetic_cifar10, synthetic_imagenet
    from cs744_distributed_data_parallel_amd.ops import functional as CF

    B, S, K = shape["B"], shape["S"], shape["classes"]
    ds = synthetic_cifar10(4 * B, device="cuda") if S == 32 else synthetic_imagenet(4 * B, device="cuda", size=S)
    if S != 32:
        ds.pad = 4  # crop on, as in training
    idx = torch.arange(len(ds), device="cuda")
    out = torch.empty(B, 3, S, S, device="cuda").contiguous(memory_format=torch.channels_last)
    fns = {}

    def loader_fn(kw):
        ld = DeviceLoader(ds, B, seed=1, **kw)
        return lambda: ld.batch(idx, 0, B, out=out, nbatches=4)

    fns["augment:off"] = loader_fn({})
    gen = torch.Generator(device="cuda").manual_seed(0)
    logits = torch.randn(B, K, device="cuda", generator=gen).requires_grad_()
    t = torch.randint(0, K, (B,), device="cuda", generator=gen)
    tb = torch.randint(0, K, (B,), device="cuda", generator=gen)
    lam = torch.tensor([0.3], device="cuda")

    def loss_fn(**kw):
        def f():
            logits.grad = None
            loss = CF.cross_entropy(logits, t, label_smoothing=0.1, **kw)
            loss.backward()
            return loss

        return f

    fns["loss:one-target"] = loss_fn()
    if has_mix:
        for name, kw in MODES.items():
            fns["augment:" + name] = loader_fn(kw)
        fns["loss:target-pair"] = loss_fn(target_b=tb, lam=lam)
    return fns, (ds, idx, out, logits, t, tb, lam)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=5, help="replays per timed block")
    p.add_argument("--inner", type=int, default=50, help="calls per captured graph")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    if not torch.cuda.is_available():
        raise SystemExit("mix_cost: needs the GPU (a CPU timing says nothing about it)")
    has_mix = hasattr(cdp._native.lib(), "mix_params")
    rec = {"device": torch.cuda.get_device_name(0), "mixing_kernels": has_mix, "rounds": args.rounds,
           "block": args.block, "inner": args.inner, "points": []}
    for shape in SHAPES:
        fns, keep = variants(cdp, torch, shape, has_mix)
        graphs = {k: capture(torch, f, args.inner) for k, f in fns.items()}
        for g, _ in graphs.values():
            for _ in range(5):
                g.replay()
        torch.cuda.synchronize()
        us = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, (g, _) in graphs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.block):
                    g.replay()
                torch.cuda.synchronize()
                us[k].append((time.perf_counter() - t0) / (args.block * args.inner) * 1e6)
        for k in graphs:
            pt = {"shape": shape["name"], "variant": k, "calls": args.rounds * args.block * args.inner,
                  "us_per_call_median": round(statistics.median(us[k]), 3), "us_per_call_min": round(min(us[k]), 3),
                  "us_per_call_max": round(max(us[k]), 3)}
            rec["points"].append(pt)
            print(json.dumps(pt), flush=True)
        del graphs, keep
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
