#!/usr/bin/env python
"""Cost of the LARS step against the plain fused SGD step (docs/PERF.md, "LARS").

On the VGG-11 arena after one forward/backward at ``--batch`` images, ``opt.step()`` ALONE is captured
into a hipGraph for ``cdp.SGD`` and for ``cdp.LARS`` (each its own model, both in the
weight-preparation form of the step); after a warm-up the graphs are replayed in alternation, in
blocks timed with device events. Also timed, the same way: the norms pass alone, whose traffic is one
read of the parameter range and one of the gradient range, against the HBM peak.

A tree without ``cdp.LARS`` times ``cdp.SGD`` alone, so the same script gives the yardstick of an
older commit:

    python scripts/bench_lars_step.py [--batch 256] [--rounds 10] [--block 25] [--repeat 3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X


def build(cdp, torch, batch, kind):
    torch.manual_seed(0)
    model = cdp.VGG11().cuda()
    hp = dict(momentum=0.9, weight_decay=1e-4)
    opt = cdp.SGD(model.parameters(), lr=0.01, **hp) if kind == "sgd" else cdp.LARS(model.parameters(), 0.01, **hp)
    crit = cdp.CrossEntropyLoss()
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(batch, 3, 32, 32, device="cuda", generator=gen).contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (batch,), device="cuda", generator=gen)
    for _ in range(2):  # the second step is a "later" momentum step, as every captured one below
        opt.zero_grad()
        crit(model(x), y).backward()
        opt.step()
    opt.zero_grad()
    crit(model(x), y).backward()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        opt.step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        opt.step()
    torch.cuda.synchronize()
    return g, (model, opt, crit, x, y)


def build_norms(cdp, torch, opt):
    """The norms launch of a LARS optimizer alone, captured."""
    C = cdp._native.lib()
    arena = opt._arena
    lp = opt._lars_plan[1]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        C.lars_norms(arena.data, arena.grad, lp["desc"], lp["meta"], lp["part"])
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        C.lars_norms(arena.data, arena.grad, lp["desc"], lp["meta"], lp["part"])
    torch.cuda.synchronize()
    return g, 2 * 4 * arena.total


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batch", type=int, default=256)
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=25, help="replays per timed block (rounds x block >= 200 replays)")
    p.add_argument("--repeat", type=int, default=3, help="whole measurements, for the run-to-run spread")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    if not torch.cuda.is_available():
        raise SystemExit("bench_lars_step: needs the GPU (a CPU timing says nothing about it)")
    kinds = ["sgd"] + (["lars"] if hasattr(cdp, "LARS") else [])
    runs = {k: build(cdp, torch, args.batch, k) for k in kinds}
    graphs = {k: g for k, (g, _) in runs.items()}
    norm_bytes = None
    if "lars" in runs:
        graphs["norms"], norm_bytes = build_norms(cdp, torch, runs["lars"][1][1])
    rec = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "rounds": args.rounds, "block": args.block,
           "points": []}
    for rep in range(args.repeat):
        for g in graphs.values():  # warm-up as replays of the graphs that are timed next
            for _ in range(20):
                g.replay()
        torch.cuda.synchronize()
        us = {k: [] for k in graphs}
        for _ in range(args.rounds):
            for k, g in graphs.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.block):
                    g.replay()
                b.record()
                b.synchronize()
                us[k].append(a.elapsed_time(b) / args.block * 1e3)
        for k in graphs:
            pt = {"repeat": rep, "variant": k, "replays": args.rounds * args.block,
                  "us_per_step_median": round(statistics.median(us[k]), 2), "us_per_step_min": round(min(us[k]), 2),
                  "us_per_step_max": round(max(us[k]), 2)}
            if k == "norms":
                bps = norm_bytes / (statistics.median(us[k]) * 1e-6)
                pt.update(bytes=norm_bytes, bytes_per_s=round(bps, -9), hbm_peak_fraction=round(bps / HBM_PEAK, 3))
            rec["points"].append(pt)
            print(json.dumps(pt), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
