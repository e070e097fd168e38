#!/usr/bin/env python
"""Cost of the weight EMA in the captured VGG-11 step (docs/PERF.md, "Weight EMA").

Two variants of the same captured training step (zero_grad, forward, CrossEntropy, backward, fused
SGD) at each batch size: ``ema_decay`` off and on. Each variant is its own model + optimizer + hipGraph
over the same static batch; after a warm-up the variants are timed in alternation (round-robin blocks
of replays, host clock around replays that end in a device synchronise), so both see the same box in
the same minutes. A second graph per variant holds the optimizer step alone (the stand-alone SGD
launch over the model's arena, gradients left as the last backward wrote them, 20 launches per graph
and the time divided by 20) and is timed the same way.

For the A/B of the EMA-off build against the parent commit, run this file with ``--variants off`` from
a checkout of each (``--repo DIR`` imports the package from DIR) on the same box, alternating the two,
and compare the medians with the spread of the parent's own repeats.

    python scripts/ema_cost.py [--batches 256,32] [--rounds 10] [--block 25] [--variants off,ema] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

VARIANTS = {"off": {}, "ema": dict(ema_decay=0.999)}
SGD_PER_GRAPH = 20  # launches in the graph of the stand-alone step, so that its replay is not all graph launch


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


def build(cdp, torch, batch, kw):
    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    opt = cdp.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, **kw)
    crit = cdp.CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(batch, 3, 32, 32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (batch,), device="cuda", generator=gen)

    def body():
        opt.zero_grad()
        crit(model(x), y).backward()
        opt.step()

    for _ in range(3):
        body()
    step = capture(torch, body)

    def steps():  # the optimizer's launch alone, in the form the step runs it, SGD_PER_GRAPH times over
        for _ in range(SGD_PER_GRAPH):
            opt.step()

    sgd = capture(torch, steps)
    # the graphs replay over the model's parameters and buffers and over x / y: everything they touch is
    # returned and kept alive by the caller for as long as they are replayed
    return {"step": step, "sgd": sgd}, (model, opt, crit, x, y)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="256,32")
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=25, help="replays per timed block (rounds x block >= 200 steps)")
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
        raise SystemExit("ema_cost: needs the GPU (a CPU timing says nothing about it)")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "block": args.block, "label": args.label,
           "points": []}
    for batch in [int(b) for b in args.batches.split(",")]:
        runs = {k: build(cdp, torch, batch, kw) for k, kw in VARIANTS.items() if k in args.variants.split(",")}
        for what in ("step", "sgd"):
            for graphs, _ in runs.values():  # warm-up as replays of the graphs that are timed next
                for _ in range(20):
                    graphs[what].replay()
            torch.cuda.synchronize()
            ms = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, (graphs, _) in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.block):
                        graphs[what].replay()
                    torch.cuda.synchronize()
                    per = args.block * (SGD_PER_GRAPH if what == "sgd" else 1)
                    ms[k].append((time.perf_counter() - t0) / per * 1e3)
            for k in runs:
                pt = {"label": args.label, "batch": batch, "what": what, "variant": k, "steps": args.rounds * args.block,
                      "ms_median": round(statistics.median(ms[k]), 4), "ms_min": round(min(ms[k]), 4),
                      "ms_max": round(max(ms[k]), 4)}
                rec["points"].append(pt)
                print(json.dumps(pt), flush=True)
        torch.cuda.synchronize()
        del runs
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
