#!/usr/bin/env python
"""Cost of stochastic depth in the captured ResNet-50 step (docs/PERF.md, "Stochastic depth in the
residual apply").

Two variants of the same captured training step (zero_grad, forward, CrossEntropy, backward, fused SGD)
at B = 64, 224 x 224: ``drop_path_rate`` 0 and 0.05. Each variant is its own model + optimizer + hipGraph
over the same static batch; after a warm-up the variants are timed in alternation (round-robin blocks of
replays, host clock around replays that end in a device synchronise), so both see the same box in the same
minutes. A second graph of the rate-0.05 model holds the draw launch alone (20 launches per graph and the
time divided by 20) and is timed the same way.

For the A/B of the rate-0 build against the parent commit, run this file with ``--variants off`` from a
checkout of each (``--repo DIR`` imports the package from DIR) on the same box, alternating the two, and
compare the medians with the spread of the parent's own repeats.

    python scripts/drop_path_cost.py [--batch 64] [--size 224] [--rounds 10] [--block 10] [--variants off,drop]
                                     [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

VARIANTS = {"off": {}, "drop": dict(drop_path_rate=0.05)}
DRAWS_PER_GRAPH = 20  # launches in the graph of the stand-alone draw, so that its replay is not all graph launch


def capture(torch, body):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    torch.cuda.synchronize()
    return g


def build(cdp, torch, batch, size, kw):
    torch.manual_seed(0)
    model = cdp.resnet50(**kw).cuda()
    opt = cdp.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    crit = cdp.CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(batch, 3, size, size, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (batch,), device="cuda", generator=gen)

    def body():
        opt.zero_grad()
        crit(model(x), y).backward()
        opt.step()

    for _ in range(3):
        body()
    graphs = {"step": capture(torch, body)}
    if kw:

        def draws():  # the draw launch alone, in the form the forward runs it, DRAWS_PER_GRAPH times over
            for _ in range(DRAWS_PER_GRAPH):
                model._draw_drop_scales(x)

        graphs["draw"] = capture(torch, draws)
    # the graphs replay over the model's parameters and buffers and over x / y: everything they touch is
    # returned and kept alive by the caller for as long as they are replayed
    return graphs, (model, opt, crit, x, y)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=10, help="replays per timed block")
    p.add_argument("--variants", default=",".join(VARIANTS), help="comma list of: " + ", ".join(VARIANTS))
    p.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   help="import the package from this checkout (default: the one this file is in)")
    p.add_argument("--label", default=None, help="a name for this run in the records (e.g. parent / new)")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    if not torch.cuda.is_available():
        raise SystemExit("drop_path_cost: needs the GPU (a CPU timing says nothing about it)")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "block": args.block, "label": args.label,
           "batch": args.batch, "size": args.size, "points": []}
    runs = {k: build(cdp, torch, args.batch, args.size, kw) for k, kw in VARIANTS.items()
            if k in args.variants.split(",")}
    for what in ("step", "draw"):
        timed = {k: g[what] for k, (g, _) in runs.items() if what in g}
        for g in timed.values():  # warm-up as replays of the graphs that are timed next
            for _ in range(10):
                g.replay()
        torch.cuda.synchronize()
        ms = {k: [] for k in timed}
        for _ in range(args.rounds):
            for k, g in timed.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.block):
                    g.replay()
                torch.cuda.synchronize()
                per = args.block * (DRAWS_PER_GRAPH if what == "draw" else 1)
                ms[k].append((time.perf_counter() - t0) / per * 1e3)
        for k in timed:
            pt = {"label": args.label, "batch": args.batch, "what": what, "variant": k,
                  "steps": args.rounds * args.block, "ms_median": round(statistics.median(ms[k]), 4),
                  "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4)}
            rec["points"].append(pt)
            print(json.dumps(pt), flush=True)
    torch.cuda.synchronize()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
