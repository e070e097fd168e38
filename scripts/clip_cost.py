#!/usr/bin/env python
"""Cost of gradient-norm clipping in the captured VGG-11 step (docs/PERF.md, "Gradient clipping").

Three variants of the same captured training step (zero_grad, forward, CrossEntropy, backward, fused
SGD) at each batch size: clipping off, ``max_grad_norm`` on, and on with ``skip_nonfinite``. Each
variant is its own model + optimizer + hipGraph over the same static batch; after a warm-up the
variants are timed in alternation (round-robin blocks of replays, host clock around replays that end
in a device synchronise), so all three see the same box in the same minutes. Also prints the node
count of each captured graph (+1 is expected with clipping on: the sum-of-squares launch).

    python scripts/clip_cost.py [--batches 256,32] [--rounds 10] [--block 25] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = {"off": {}, "clip": dict(max_grad_norm=1.0), "clip+skip": dict(max_grad_norm=1.0, skip_nonfinite=True)}


def graph_nodes(g):
    """Nodes of a captured graph (kernel launches and whatever else was recorded), or None."""
    try:
        raw = g.raw_cuda_graph()
        hip = ctypes.CDLL("libamdhip64.so")
        n = ctypes.c_size_t(0)
        rc = hip.hipGraphGetNodes(ctypes.c_void_p(int(raw)), None, ctypes.byref(n))
        return int(n.value) if rc == 0 else None
    except Exception:  # noqa: BLE001 - a count that cannot be taken is reported as not measured
        return None


def build(cdp, torch, batch, kw, count_nodes=True):
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
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()
    torch.cuda.current_stream().wait_stream(s)
    nodes = None
    try:
        if not count_nodes:
            raise RuntimeError("node count not asked for")
        g = torch.cuda.CUDAGraph(keep_graph=True)  # keeps the hipGraph_t so its nodes can be counted
        with torch.cuda.graph(g):
            body()
        nodes = graph_nodes(g)
        g.instantiate()
    except Exception:  # noqa: BLE001 - no kept graph in this build: capture the plain way, count not measured
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
    torch.cuda.synchronize()
    # the graph replays over the model's parameters and buffers and over x / y: everything it touches is
    # returned and kept alive by the caller for as long as the graph is replayed
    return g, opt, nodes, (model, crit, x, y)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--batches", default="256,32")
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=25, help="replays per timed block (rounds x block >= 200 steps)")
    p.add_argument("--variants", default=",".join(VARIANTS), help="comma list of: " + ", ".join(VARIANTS))
    p.add_argument("--out", default=None)
    p.add_argument("--no-node-count", action="store_true", help="do not keep the captured graphs to count their nodes")
    args = p.parse_args(argv)
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    if not torch.cuda.is_available():
        raise SystemExit("clip_cost: needs the GPU (a CPU timing says nothing about it)")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "block": args.block, "points": []}
    for batch in [int(b) for b in args.batches.split(",")]:
        runs = {k: build(cdp, torch, batch, kw, not args.no_node_count) for k, kw in VARIANTS.items()
                if k in args.variants.split(",")}
        for g, *_ in runs.values():  # warm-up as replays of the graphs that are timed next
            for _ in range(20):
                g.replay()
        torch.cuda.synchronize()
        ms = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, (g, *_) in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.block):
                    g.replay()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / args.block * 1e3)
        for k, (g, opt, nodes, _) in runs.items():
            pt = {"batch": batch, "variant": k, "steps": args.rounds * args.block, "graph_nodes": nodes,
                  "ms_per_step_median": round(statistics.median(ms[k]), 4), "ms_per_step_min": round(min(ms[k]), 4),
                  "ms_per_step_max": round(max(ms[k]), 4)}
            if getattr(opt, "grad_norm", None) is not None:
                pt.update(grad_norm=float(opt.grad_norm), clip_coef=float(opt.clip_coef),
                          skipped_steps=float(opt.skipped_steps))
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
