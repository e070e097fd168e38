#!/usr/bin/env python
"""Cost of the fused AdamW / LAMB step (docs/PERF.md, "AdamW and LAMB in the fused step").

On the parameter sets of VGG-11 and ResNet-50 (random gradients written into the arena; no forward is
needed to time a step), ``step()`` alone of

* ``cdp.AdamW`` and ``cdp.LAMB``,
* ``cdp.SGD`` (momentum 0.9) on an arena of the same layout (the plain ``sgd_kernel``: no forward has
  registered a weight-preparation request),
* ``torch.optim.AdamW(fused=True)`` and ``torch.optim.AdamW(foreach=True)`` on the same kind of tensors
  (``capturable=True``, so that they can be captured too)

is captured into a hipGraph each (eager calls where a capture fails, marked ``"mode": "eager"``); after a
warm-up the graphs are replayed in alternation, in blocks timed with device events: rounds x block >= 200
steps per measurement, ``--repeat`` whole measurements for the run-to-run spread. Bytes per second are
reported against the byte counts of the design: AdamW 28 B per element (36 with the EMA), LAMB 40 (48), SGD
with momentum 20. Also timed: the stand-alone weight-preparation launch (maxima and W^T of the conv
weights) that the next forward runs after an AdamW / LAMB step, which the fused SGD step absorbs.

    python scripts/bench_adam.py [--models vgg11 resnet50] [--rounds 10] [--block 25] [--repeat 3] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s, MI355X
BYTES = {"adamw": 28, "adamw_ema": 36, "lamb": 40, "lamb_ema": 48, "sgd": 20, "torch_fused": 28, "torch_foreach": 28}


def _model(cdp, torch, name):
    torch.manual_seed(0)
    return (cdp.VGG11() if name == "vgg11" else cdp.resnet50()).cuda()


def _optimizer(cdp, torch, kind, params):
    if kind == "adamw":
        return cdp.AdamW(params, lr=1e-3)
    if kind == "adamw_ema":
        return cdp.AdamW(params, lr=1e-3, ema_decay=0.999)
    if kind == "lamb":
        return cdp.LAMB(params, lr=1e-3)
    if kind == "lamb_ema":
        return cdp.LAMB(params, lr=1e-3, ema_decay=0.999)
    if kind == "sgd":
        return cdp.SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    if kind == "torch_fused":
        return torch.optim.AdamW(params, lr=1e-3, fused=True, capturable=True)
    return torch.optim.AdamW(params, lr=1e-3, foreach=True, capturable=True)


def build(cdp, torch, name, kind):
    """(replay callable, mode, elements) of one optimizer's step() on its own copy of the model."""
    from cs744_distributed_data_parallel_amd.utils.arena import arena_for

    model = _model(cdp, torch, name)
    params = list(model.parameters())
    arena = arena_for(params)
    arena.attach_grads()
    gen = torch.Generator(device="cuda").manual_seed(1)
    arena.grad.copy_(torch.randn(arena.total, device="cuda", generator=gen) * 0.01)
    for p, off in zip(arena.params, arena.offsets):  # the pad floats stay zero
        n = p.numel()
        arena.grad[off + n:off + (n + 3) // 4 * 4] = 0
    assert all(p.grad is not None for p in params)
    opt = _optimizer(cdp, torch, kind, params)
    for _ in range(2):
        opt.step()
    torch.cuda.synchronize()
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            opt.step()
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        torch.cuda.synchronize()
        return g.replay, "graph", arena.total, (model, opt)
    except Exception as exc:  # a step that cannot be captured is timed eagerly
        torch.cuda.synchronize()
        print(f"# {name} {kind}: capture failed ({type(exc).__name__}: {str(exc)[:120]}); timing eager calls", flush=True)
        return opt.step, "eager", arena.total, (model, opt)


def build_prep(cdp, torch, name):
    """The stand-alone weight preparation of the model's conv weights, captured: what the forward after an
    AdamW / LAMB step launches (FlatArena.prep_refresh runs the same kernel into the same buffers)."""
    model = _model(cdp, torch, name)
    opt = cdp.SGD(model.parameters(), lr=1e-3, momentum=0.9)
    side = 32 if name == "vgg11" else 64
    x = torch.randn(8, 3, side, side, device="cuda").contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 10, (8,), device="cuda")
    for _ in range(2):  # the forward registers the request, the fused step plans it
        opt.zero_grad()
        cdp.CrossEntropyLoss()(model(x), y).backward()
        opt.step()
    arena = opt._arena
    if not arena.prep_refresh():
        return None
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        arena.prep_refresh()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        arena.prep_refresh()
    torch.cuda.synchronize()
    return g.replay, "graph", 0, (model, opt)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--models", nargs="+", default=["vgg11", "resnet50"], choices=["vgg11", "resnet50"])
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=25, help="steps per timed block (rounds x block >= 200 steps)")
    p.add_argument("--repeat", type=int, default=3, help="whole measurements, for the run-to-run spread")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    if not torch.cuda.is_available():
        raise SystemExit("bench_adam: needs the GPU (a CPU timing says nothing about it)")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "block": args.block, "points": []}
    for name in args.models:
        runs = {}
        for kind in BYTES:
            try:
                runs[kind] = build(cdp, torch, name, kind)
            except Exception as exc:
                print(f"# {name} {kind}: not timed ({type(exc).__name__}: {str(exc)[:160]})", flush=True)
        try:
            prep = build_prep(cdp, torch, name)
            if prep is not None:
                runs["weight_prep"] = prep
        except Exception as exc:
            print(f"# {name} weight_prep: not timed ({type(exc).__name__}: {str(exc)[:160]})", flush=True)
        for rep in range(args.repeat):
            for fn, _, _, _ in runs.values():  # warm-up as calls of what is timed next
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            us = {k: [] for k in runs}
            for _ in range(args.rounds):
                for k, (fn, _, _, _) in runs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.block):
                        fn()
                    b.record()
                    b.synchronize()
                    us[k].append(a.elapsed_time(b) / args.block * 1e3)
            for k, (_, mode, n, _) in runs.items():
                med = statistics.median(us[k])
                pt = {"model": name, "repeat": rep, "variant": k, "mode": mode, "steps": args.rounds * args.block,
                      "us_per_step_median": round(med, 2), "us_per_step_min": round(min(us[k]), 2),
                      "us_per_step_max": round(max(us[k]), 2)}
                if k in BYTES:
                    nbytes = BYTES[k] * n
                    pt.update(elements=n, bytes=nbytes, bytes_per_s=round(nbytes / (med * 1e-6), -9),
                              hbm_peak_fraction=round(nbytes / (med * 1e-6) / HBM_PEAK, 3))
                rec["points"].append(pt)
                print(json.dumps(pt), flush=True)
        del runs
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
