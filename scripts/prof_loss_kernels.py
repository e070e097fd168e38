"""Kernel times of the loss kernels per shape: binary cross-entropy beside softmax cross-entropy.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python scripts/prof_loss_kernels.py run OUT/plan.json
    python scripts/prof_loss_kernels.py summarise OUT/run_kernel_trace.csv OUT/plan.json [OUT/summary.md]

``run`` issues, per entry of its plan, WARM + CALLS launches of one kernel at one shape, back to back, and writes
the plan (label, kernel name substring, warm, calls) as JSON. ``summarise`` walks the trace's dispatches of those
kernels in start order, cuts them by the plan and prints mean / median / min of the CALLS timed launches.
"""
import csv
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, CALLS = 10, 100
SHAPES = [(256, 10), (256, 1000), (64, 1000)]
LINEAR = (256, 512, 10)  # VGG-11's classifier: batch, in features, classes


def run(plan_path):
    import torch

    import cs744_distributed_data_parallel_amd as cdp

    lib = cdp._native.lib()
    plan = []
    g = torch.ones(1, device="cuda")
    lam = torch.full((1,), 0.3, device="cuda")

    def timed(label, kernel, fn):
        for _ in range(WARM + CALLS):
            fn()
        torch.cuda.synchronize()
        plan.append([label, kernel, WARM, CALLS])

    for B, C in SHAPES:
        torch.manual_seed(0)
        z = 3 * torch.randn(B, C, device="cuda")
        t = torch.randint(0, C, (B,), device="cuda")
        tb = t.flip(0).contiguous()
        s = f"({B}, {C})"
        timed(f"xent_fwd {s} eps 0.1", "xent_fwd_kernel", lambda: lib.xent_fwd(z, t, None, 0.1))
        timed(f"xent_fwd {s} eps 0.1 mixed", "xent_fwd_kernel", lambda: lib.xent_fwd(z, t, None, 0.1, 1, tb, lam))
        timed(f"bce_fwd {s} eps 0.1", "bce_fwd_kernel", lambda: lib.bce_fwd(z, t, 0.1))
        timed(f"bce_fwd {s} eps 0.1 mixed thr 0.2", "bce_fwd_kernel", lambda: lib.bce_fwd(z, t, 0.1, 0.2, False, tb, lam))
        timed(f"xent_bwd {s} eps 0.1", "xent_bwd_kernel", lambda: lib.xent_bwd(g, z, t, 0.1))
        timed(f"xent_bwd {s} eps 0.1 mixed", "xent_bwd_kernel", lambda: lib.xent_bwd(g, z, t, 0.1, tb, lam))
        timed(f"bce_bwd {s} eps 0.1", "bce_bwd_kernel", lambda: lib.bce_bwd(g, z, t, 0.1))
        timed(f"bce_bwd {s} eps 0.1 mixed thr 0.2", "bce_bwd_kernel", lambda: lib.bce_bwd(g, z, t, 0.1, 0.2, False, tb, lam))
    B, I, O = LINEAR
    torch.manual_seed(0)
    x = torch.randn(B, I, device="cuda")
    w = torch.randn(O, I, device="cuda") * 0.05
    z = torch.randn(B, O, device="cuda")
    t = torch.randint(0, O, (B,), device="cuda")
    s = f"({B}, {I}, {O})"
    timed(f"xent_linear_bwd {s} eps 0.1, cross-entropy", "xent_linear_bwd_kernel",
          lambda: lib.xent_linear_bwd(g, z, t, x, w, True, True, label_smoothing=0.1))
    timed(f"xent_linear_bwd {s} eps 0.1, BCE thr 0.2", "xent_linear_bwd_kernel",
          lambda: lib.xent_linear_bwd(g, z, t, x, w, True, True, label_smoothing=0.1, bce=True, target_threshold=0.2))
    with open(plan_path, "w") as fh:
        json.dump(plan, fh)
    print(f"{len(plan)} entries -> {plan_path}")


def summarise(trace_csv, plan_path, out=None):
    plan = json.load(open(plan_path))
    names = sorted({p[1] for p in plan})
    rows = [r for r in csv.DictReader(open(trace_csv)) if any(n in r["Kernel_Name"] for n in names)]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    lines = ["| kernel, shape | calls | mean us | median us | min us |", "|---|---|---|---|---|"]
    i = 0
    for label, kernel, warm, calls in plan:
        chunk = rows[i:i + warm + calls]
        i += warm + calls
        if len(chunk) != warm + calls or not all(kernel in r["Kernel_Name"] for r in chunk):
            raise SystemExit(f"trace does not follow the plan at {label!r}")
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk[warm:]]
        lines.append(f"| {label} | {calls} | {statistics.mean(us):.2f} | {statistics.median(us):.2f} | {min(us):.2f} |")
    if i != len(rows):
        raise SystemExit(f"{len(rows) - i} dispatches beyond the plan")
    text = "\n".join(lines)
    if out:
        open(out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "run":
        run(a[1])
    elif a and a[0] == "summarise":
        summarise(*a[1:4])
    else:
        raise SystemExit(__doc__)
