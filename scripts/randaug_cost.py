#!/usr/bin/env python
"""Cost of RandAugment in the loader (docs/PERF.md, "RandAugment in the loader").

Times the loader's batch() call with mixup / CutMix and RandomErasing on, at
  * 256x32^2          the plain path (pad-shift crop + flip) on CIFAR-shaped images;
  * 64x256^2->224^2   the resize path (RandomResizedCrop at scale (0.08, 1)) on ImageNet-shaped images,
for
  * randaug:off       the loader without the RandAugment arguments: its one augment launch (and the
                      one-thread counter launch), the launches of the loader before RandAugment existed;
  * randaug:2x9       randaug_num_ops = 2, magnitude 9, mstd 0.5, all 14 ops (the "ResNet strikes back"
                      setting): the randaug launch, then the plain augment launch on the staged batch;
  * randaug:3x15      three operations at magnitude 15.
Every variant is a captured hipGraph of ``--inner`` back-to-back calls (scripts/mix_cost.py's capture); after a
warm-up the variants are timed in alternation, in round-robin blocks of ``--block`` replays between two device
events, ``--rounds`` times: rounds x block >= 200 replays per variant, all in the same minutes on the same box.

``--root DIR`` imports the package from another checkout (one that is built), e.g. the parent commit: a tree
without the RandAugment arguments times ``randaug:off`` alone, the figure to hold this tree's against.

``--variants NAME ...`` keeps the named variants only (``randaug:off`` always runs: it is the base), e.g. for
a kernel trace of the off path alone.

    python scripts/randaug_cost.py [--rounds 20] [--block 10] [--inner 20] [--root DIR] [--variants NAME ...]
                                   [--out FILE.json]
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from mix_cost import capture  # noqa: E402  (the same capture protocol)

SHAPES = [dict(name="256x32^2", B=256, S=32, stored=32), dict(name="64x256^2->224^2", B=64, S=224, stored=256)]
COMMON = dict(mixup_alpha=0.8, cutmix_alpha=1.0, erase_prob=0.25, erase_mode="pixel")
RANDAUG = {"randaug:2x9": dict(randaug_num_ops=2, randaug_magnitude=9.0, randaug_mstd=0.5),
           "randaug:3x15": dict(randaug_num_ops=3, randaug_magnitude=15.0, randaug_mstd=0.5)}


def variants(torch, shape, only=None):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, synthetic_imagenet

    B, S, stored = shape["B"], shape["S"], shape["stored"]
    ds = synthetic_imagenet(4 * B, device="cuda", size=stored)
    ds.pad = 4  # the plain path crops, as in training
    base = dict(rrc_scale=(0.08, 1.0), out_size=S) if stored != S else {}
    out = torch.empty(B, 3, S, S, device="cuda").contiguous(memory_format=torch.channels_last)
    idx = torch.arange(len(ds), device="cuda")

    def loader_fn(**kw):
        ld = DeviceLoader(ds, B, seed=1, **base, **COMMON, **kw)
        return lambda: ld.batch(idx, 0, B, out=out, nbatches=4)

    fns = {"randaug:off": loader_fn()}
    if "randaug_num_ops" in inspect.signature(DeviceLoader.__init__).parameters:
        fns.update({k: loader_fn(**kw) for k, kw in RANDAUG.items() if only is None or k in only})
    return fns, (ds, out, idx)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--block", type=int, default=10, help="replays per timed block")
    p.add_argument("--inner", type=int, default=20, help="calls per captured graph")
    p.add_argument("--root", default=os.path.dirname(HERE), help="the built checkout to import the package from")
    p.add_argument("--variants", nargs="+", default=None, choices=["randaug:off"] + list(RANDAUG))
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.root))
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("randaug_cost: needs the GPU (a CPU timing says nothing about it)")
    rec = {"device": torch.cuda.get_device_name(0), "root": os.path.abspath(args.root), "rounds": args.rounds,
           "block": args.block, "inner": args.inner, "points": []}
    for shape in SHAPES:
        fns, keep = variants(torch, shape, args.variants)
        graphs = {k: capture(torch, f, args.inner) for k, f in fns.items()}
        for g, _ in graphs.values():
            for _ in range(5):
                g.replay()
        torch.cuda.synchronize()
        us = {k: [] for k in graphs}
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.rounds):
            for k, (g, _) in graphs.items():
                start.record()
                for _ in range(args.block):
                    g.replay()
                end.record()
                end.synchronize()
                us[k].append(start.elapsed_time(end) * 1e3 / (args.block * args.inner))
        base = statistics.median(us["randaug:off"])
        for k in graphs:
            med = statistics.median(us[k])
            pt = {"shape": shape["name"], "variant": k, "replays": args.rounds * args.block,
                  "calls": args.rounds * args.block * args.inner, "us_per_call_median": round(med, 3),
                  "us_per_call_min": round(min(us[k]), 3), "us_per_call_max": round(max(us[k]), 3),
                  "us_over_off": round(med - base, 3)}
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
