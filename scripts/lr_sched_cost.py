#!/usr/bin/env python
"""Cost of the learning-rate schedule in the captured VGG-11 step (docs/PERF.md, "Learning-rate schedule
in the fused step").

Four variants of the same captured training step (zero_grad, forward, CrossEntropy, backward, fused SGD)
at each batch size:

  a  parent    a build of the parent commit (``--parent DIR``: a checkout of it with its extension built)
  b  off       this tree, no schedule
  c  sched     this tree, ``lr_schedule`` set: the rate evaluated in the SGD kernel's prologue, the step
               index advanced by the arrival count of its workgroups
  d  off+inc   this tree, no schedule, plus one ``counter_inc`` launch in the graph: the price of the
               one-thread launch a host-fed ``lr_tensor`` costs per step, the design (c) replaces

The two builds take turns: every round starts one fresh worker process per build (never two at a time),
parent first, and inside a worker its variants are timed in alternation (round-robin blocks of replays,
host clock around replays that end in a device synchronise), so all of them see the same box in the same
minutes. A second graph per variant holds the optimizer step alone (20 launches per graph, the time
divided by 20), timed the same way. The spread of the parent's own repeats (its rounds' medians) is what
(b) is compared with.

    python scripts/lr_sched_cost.py --parent DIR [--batches 256,32] [--rounds 3] [--blocks 8] [--block 25] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

SGD_PER_GRAPH = 20  # launches in the graph of the stand-alone step, so that its replay is not all graph launch
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def build(cdp, torch, batch, variant):
    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    kw = {}
    if variant == "sched":
        # a schedule long enough that no replay of this run reaches its end branch
        kw["lr_schedule"] = cdp.LRSchedule("cosine", total_steps=10 ** 9, warmup_steps=1000, warmup_start_factor=0.1)
    opt = cdp.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4, **kw)
    crit = cdp.CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(batch, 3, 32, 32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (batch,), device="cuda", generator=gen)
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    inc = cdp._native.lib().counter_inc if variant == "off+inc" else None

    def body():
        opt.zero_grad()
        crit(model(x), y).backward()
        opt.step()
        if inc is not None:
            inc(ctr)

    for _ in range(3):
        body()
    step = capture(torch, body)

    def steps():  # the optimizer's launch alone, in the form the step runs it, SGD_PER_GRAPH times over
        for _ in range(SGD_PER_GRAPH):
            opt.step()
            if inc is not None:
                inc(ctr)

    sgd = capture(torch, steps)
    # everything the graphs touch is returned and kept alive by the caller for as long as they are replayed
    return {"step": step, "sgd": sgd}, (model, opt, crit, x, y, ctr)


def worker(args):
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    if not torch.cuda.is_available():
        raise SystemExit("lr_sched_cost: needs the GPU (a CPU timing says nothing about it)")
    variants = args.variants.split(",")
    for batch in [int(b) for b in args.batches.split(",")]:
        runs = {v: build(cdp, torch, batch, v) for v in variants}
        for what in ("step", "sgd"):
            for graphs, _ in runs.values():  # warm-up as replays of the graphs that are timed next
                for _ in range(20):
                    graphs[what].replay()
            torch.cuda.synchronize()
            ms = {v: [] for v in runs}
            for _ in range(args.blocks):
                for v, (graphs, _) in runs.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.block):
                        graphs[what].replay()
                    torch.cuda.synchronize()
                    per = args.block * (SGD_PER_GRAPH if what == "sgd" else 1)
                    ms[v].append((time.perf_counter() - t0) / per * 1e3)
            for v in runs:
                print(json.dumps({"label": args.label, "batch": batch, "what": what, "variant": v,
                                  "steps": args.blocks * args.block, "ms_median": round(statistics.median(ms[v]), 5),
                                  "ms_min": round(min(ms[v]), 5), "ms_max": round(max(ms[v]), 5)}), flush=True)
        torch.cuda.synchronize()
        del runs
    return 0


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None, help="a checkout of the parent commit with its extension built")
    p.add_argument("--batches", default="256,32")
    p.add_argument("--rounds", type=int, default=3, help="worker processes per build, taking turns")
    p.add_argument("--blocks", type=int, default=8, help="timed blocks per variant in a worker")
    p.add_argument("--block", type=int, default=25, help="replays per timed block")
    p.add_argument("--out", default=None)
    # worker mode (one build, one process)
    p.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--repo", default=HERE, help=argparse.SUPPRESS)
    p.add_argument("--label", default="new", help=argparse.SUPPRESS)
    p.add_argument("--variants", default="off,sched,off+inc", help=argparse.SUPPRESS)
    args = p.parse_args(argv)
    if args.worker:
        return worker(args)
    builds = ([("parent", os.path.abspath(args.parent), "parent")] if args.parent else []) + [("new", HERE, args.variants)]
    points = []
    for rnd in range(args.rounds):
        for label, repo, variants in builds:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--repo", repo, "--label", label, "--variants",
                   "off" if label == "parent" else variants, "--batches", args.batches, "--blocks", str(args.blocks),
                   "--block", str(args.block)]
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=repo)  # a fresh process, one at a time
            if r.returncode != 0:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"lr_sched_cost: the {label} worker failed in round {rnd} (exit {r.returncode})")
            for ln in r.stdout.splitlines():
                if ln.startswith("{"):
                    pt = json.loads(ln)
                    pt["round"] = rnd
                    if label == "parent":
                        pt["variant"] = "parent"
                    points.append(pt)
                    print(json.dumps(pt), flush=True)
    # per (batch, what, variant): the rounds' medians, their median and their spread
    summary = []
    keys = sorted({(pt["batch"], pt["what"], pt["variant"]) for pt in points}, key=lambda k: (-k[0], k[1], k[2]))
    for batch, what, variant in keys:
        meds = [pt["ms_median"] for pt in points if (pt["batch"], pt["what"], pt["variant"]) == (batch, what, variant)]
        row = {"batch": batch, "what": what, "variant": variant, "rounds": len(meds),
               "ms_median": round(statistics.median(meds), 5), "ms_lo": round(min(meds), 5), "ms_hi": round(max(meds), 5)}
        summary.append(row)
        print("SUMMARY " + json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"rounds": args.rounds, "blocks": args.blocks, "block": args.block, "points": points,
                       "summary": summary}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
