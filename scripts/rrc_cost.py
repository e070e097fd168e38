#!/usr/bin/env python
"""Cost of the resizing augment launch (docs/PERF.md, "RandomResizedCrop and resize + center crop").

Times the loader's batch() call (the augment launch plus the one-thread counter launch) at the
benchmark's two output shapes, 256 x 32^2 and 64 x 224^2, for
  * augment:off      the plain augment launch (pad-shift crop + flip), stored size = output size;
  * rrc:same-size    RandomResizedCrop at scale (0.08, 1), stored size = output size;
  * rrc:stored-8/7   the same from the larger stored size (256 -> 224, 36 -> 32);
  * eval:center      center_crop = 0.875 of the larger stored size, resized to the output size;
  * rrc:mixup / rrc:cutmix   RandomResizedCrop at the output size with the mix forced to that mode.
The protocol is scripts/mix_cost.py's: every variant is a captured hipGraph of ``--inner`` back-to-back
calls; after a warm-up the variants are timed in alternation (round-robin blocks of replays, host clock
around replays that end in a device synchronise), so all of them see the same box in the same minutes.

    python scripts/rrc_cost.py [--rounds 10] [--block 5] [--inner 50] [--out FILE.json]
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

SHAPES = [dict(name="256x32^2", B=256, S=32, stored=36), dict(name="64x224^2", B=64, S=224, stored=256)]
SCALE = (0.08, 1.0)


def variants(torch, shape):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, synthetic_imagenet

    B, S, big = shape["B"], shape["S"], shape["stored"]
    same = synthetic_imagenet(4 * B, device="cuda", size=S)
    same.pad = 4  # the plain variant crops, as in training
    large = synthetic_imagenet(4 * B, seed=1, device="cuda", size=big)
    out = torch.empty(B, 3, S, S, device="cuda").contiguous(memory_format=torch.channels_last)

    def loader_fn(ds, **kw):
        ld = DeviceLoader(ds, B, seed=1, **kw)
        idx = torch.arange(len(ds), device="cuda")
        return lambda: ld.batch(idx, 0, B, out=out, nbatches=4)

    fns = {
        "augment:off": loader_fn(same),
        "rrc:same-size": loader_fn(same, rrc_scale=SCALE),
        "rrc:stored-8/7": loader_fn(large, rrc_scale=SCALE, out_size=S),
        "eval:center": loader_fn(large, train=False, center_crop=0.875, out_size=S),
        "rrc:mixup": loader_fn(same, rrc_scale=SCALE, mixup_alpha=1.0),
        "rrc:cutmix": loader_fn(same, rrc_scale=SCALE, cutmix_alpha=1.0),
    }
    return fns, (same, large, out)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=10)
    p.add_argument("--block", type=int, default=5, help="replays per timed block")
    p.add_argument("--inner", type=int, default=50, help="calls per captured graph")
    p.add_argument("--out", default=None)
    args = p.parse_args(argv)
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("rrc_cost: needs the GPU (a CPU timing says nothing about it)")
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
        base = statistics.median(us["augment:off"])
        for k in graphs:
            med = statistics.median(us[k])
            pt = {"shape": shape["name"], "variant": k, "calls": args.rounds * args.block * args.inner,
                  "us_per_call_median": round(med, 3), "us_per_call_min": round(min(us[k]), 3),
                  "us_per_call_max": round(max(us[k]), 3), "ratio_to_plain": round(med / base, 3)}
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
