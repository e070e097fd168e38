#!/usr/bin/env python
"""Cost of RandomErasing in the augment launch (docs/PERF.md, "RandomErasing in the augment launch").

Times the loader's batch() call (the augment launch plus the one-thread counter launch) with erasing off
and with each fill on, at
  * 256x32^2          the plain augment launch (pad-shift crop + flip) on CIFAR-shaped images;
  * 64x256^2->224^2   the resizing launch (RandomResizedCrop at scale (0.08, 1)) on ImageNet-shaped images,
for
  * erase:off                  the launch without the erase arguments;
  * erase:const / rand / pixel erase_prob = 0.25 (timm's recipe) at the default scale and ratio;
  * erase:pixel,p=1            every image erased: the most noise the pixel fill can be asked for;
  * mixup                      the batch mixed and not erased: the baseline of the next line;
  * erase:pixel+mixup          erase_prob = 0.25 with the batch mixed (mixup: both images' boxes are filled).
The protocol is scripts/mix_cost.py's: every variant is a captured hipGraph of ``--inner`` back-to-back
calls; after a warm-up the variants are timed in alternation (round-robin blocks of replays, host clock
around replays that end in a device synchronise), so all of them see the same box in the same minutes.

    python scripts/erase_cost.py [--rounds 10] [--block 5] [--inner 50] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mix_cost import capture  # noqa: E402  (the same capture protocol)

SHAPES = [dict(name="256x32^2", B=256, S=32, stored=32), dict(name="64x256^2->224^2", B=64, S=224, stored=256)]
PROB = 0.25


def variants(torch, shape):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, synthetic_imagenet

    B, S, stored = shape["B"], shape["S"], shape["stored"]
    ds = synthetic_imagenet(4 * B, device="cuda", size=stored)
    ds.pad = 4  # the plain launch crops, as in training
    base = dict(rrc_scale=(0.08, 1.0), out_size=S) if stored != S else {}
    out = torch.empty(B, 3, S, S, device="cuda").contiguous(memory_format=torch.channels_last)

    def loader_fn(**kw):
        ld = DeviceLoader(ds, B, seed=1, **base, **kw)
        idx = torch.arange(len(ds), device="cuda")
        return lambda: ld.batch(idx, 0, B, out=out, nbatches=4)

    fns = {
        "erase:off": loader_fn(),
        "erase:const": loader_fn(erase_prob=PROB, erase_mode="const"),
        "erase:rand": loader_fn(erase_prob=PROB, erase_mode="rand"),
        "erase:pixel": loader_fn(erase_prob=PROB, erase_mode="pixel"),
        "erase:pixel,p=1": loader_fn(erase_prob=1.0, erase_mode="pixel"),
        "mixup": loader_fn(mixup_alpha=1.0),
        "erase:pixel+mixup": loader_fn(erase_prob=PROB, erase_mode="pixel", mixup_alpha=1.0),
    }
    return fns, (ds, out)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=5, help="replays per timed block")
    p.add_argument("--inner", type=int, default=50, help="calls per captured graph")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("erase_cost: needs the GPU (a CPU timing says nothing about it)")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "block": args.block, "inner": args.inner,
           "points": []}
    for shape in SHAPES:
        fns, keep = variants(torch, shape)
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
        base = statistics.median(us["erase:off"])
        for k in graphs:
            med = statistics.median(us[k])
            pt = {"shape": shape["name"], "variant": k, "calls": args.rounds * args.block * args.inner,
                  "us_per_call_median": round(med, 3), "us_per_call_min": round(min(us[k]), 3),
                  "us_per_call_max": round(max(us[k]), 3), "ratio_to_off": round(med / base, 3)}
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
