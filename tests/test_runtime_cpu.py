"""Single-process CPU tests: optimizer, flat arenas, bucket planning, data pipeline, checkpoints,
timers/tracing, the training CLI (log-format parity) and the native extension surface."""
import io
import json
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

import cs744_distributed_data_parallel_amd as cdp
from cs744_distributed_data_parallel_amd.data import (
    DeviceLoader,
    DistributedSampler,
    cifar10_binary,
    synthetic_cifar10,
)
from cs744_distributed_data_parallel_amd.parallel.buckets import plan_buckets
from cs744_distributed_data_parallel_amd.utils import FlatArena, load_checkpoint, save_checkpoint
from cs744_distributed_data_parallel_amd.utils.profiling import TraceRecorder
from cs744_distributed_data_parallel_amd.utils.timer import PhaseTimer


# ----------------------------------------------------------------------------- optimizer
@pytest.mark.parametrize("kw", [dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.9, nesterov=True),
                                dict(momentum=0.5, dampening=0.1, weight_decay=1e-3), dict(), dict(maximize=True)])
def test_sgd_matches_torch_reference(kw):
    torch.manual_seed(0)
    a = torch.nn.Linear(5, 3)
    b = torch.nn.Linear(5, 3)
    b.load_state_dict(a.state_dict())
    o1 = cdp.SGD(a.parameters(), lr=0.1, **kw)
    o2 = torch.optim.SGD(b.parameters(), lr=0.1, **kw)
    for _ in range(4):
        x = torch.randn(7, 5)
        for m, o in ((a, o1), (b, o2)):
            o.zero_grad()
            m(x).pow(2).sum().backward()
            o.step()
    for p, q in zip(a.parameters(), b.parameters()):
        assert torch.allclose(p, q, atol=1e-7)


def test_sgd_state_dict_is_torch_compatible():
    m = torch.nn.Linear(4, 2)
    o = cdp.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    m(torch.randn(3, 4)).sum().backward()
    o.step()
    sd = o.state_dict()
    g = sd["param_groups"][0]
    assert g["lr"] == 0.1 and g["momentum"] == 0.9 and g["weight_decay"] == 1e-4 and g["dampening"] == 0
    assert g["nesterov"] is False
    assert set(sd["state"][0]) == {"momentum_buffer"}
    o2 = torch.optim.SGD(torch.nn.Linear(4, 2).parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    o2.load_state_dict(sd)


def test_sgd_rejects_bad_hparams():
    p = [torch.nn.Parameter(torch.zeros(2))]
    with pytest.raises(ValueError):
        cdp.SGD(p, lr=-1)
    with pytest.raises(ValueError):
        cdp.SGD(p, lr=0.1, nesterov=True)


# ----------------------------------------------------------------------------- arenas
def test_flat_arena_views_and_relayout():
    m = cdp.VGG11()
    before = [p.detach().clone() for p in m.parameters()]
    ar = FlatArena(list(m.parameters()))
    for p, b in zip(m.parameters(), before):
        assert torch.equal(p.detach(), b)
        assert p.data_ptr() >= ar.data.data_ptr()
        assert p.data_ptr() % 16 == 0
    assert m.layers[0].weight.is_contiguous(memory_format=torch.channels_last)
    for p in m.parameters():
        p.grad.fill_(float(p._cdp_index))
    ar.momentum_buffer().copy_(ar.grad)
    order = list(range(len(ar.params)))[::-1]
    ar.relayout(order)
    for p, b in zip(m.parameters(), before):
        assert torch.equal(p.detach(), b)
        assert torch.all(p.grad == float(len(order) - 1 - p._cdp_index))
    mv = ar.momentum_views()
    for p in m.parameters():
        assert torch.equal(mv[p._cdp_index], p.grad)


def test_arena_claims_once_per_iteration():
    m = torch.nn.Linear(3, 2)
    ar = FlatArena(list(m.parameters()))
    for p in m.parameters():
        p.grad = None
    s = ar.claim(m.weight)
    assert s is not None and s.shape == m.weight.shape
    assert ar.claim(m.weight) is None
    ar.reset_claims()
    m.weight.grad = torch.zeros_like(m.weight)
    assert ar.claim(m.weight) is None


# ----------------------------------------------------------------------------- buckets
def test_bucket_plan_matches_torch_assignment():
    sizes = [6912, 256, 256, 256, 294912, 512, 512, 512, 1179648, 1024, 1024, 1024, 2359296, 1024, 1024, 1024,
             4718592, 2048, 2048, 2048, 9437184, 2048, 2048, 2048, 9437184, 2048, 2048, 2048, 9437184, 2048, 2048,
             2048, 20480, 40]
    rev = sizes[::-1]
    b = plan_buckets(rev, cap_mb=25.0, first_cap_mb=1.0)
    assert sum(len(x) for x in b) == len(sizes)
    tensors = [torch.empty(n // 4) for n in rev]
    ref = torch.distributed._compute_bucket_assignment_by_size(tensors, [1024 * 1024, 25 * 1024 * 1024])
    ref = ref[0] if isinstance(ref, tuple) else ref
    assert [list(x) for x in b] == [list(x) for x in ref]


# ----------------------------------------------------------------------------- data
@pytest.mark.parametrize("n,world,shuffle,drop_last", [(50000, 2, True, False), (10, 4, True, False),
                                                       (103, 3, False, False), (103, 3, True, True)])
def test_distributed_sampler_matches_torch(n, world, shuffle, drop_last):
    ds = list(range(n))
    for r in range(world):
        ours = DistributedSampler(ds, num_replicas=world, rank=r, shuffle=shuffle, drop_last=drop_last)
        ref = torch.utils.data.distributed.DistributedSampler(ds, num_replicas=world, rank=r, shuffle=shuffle,
                                                              drop_last=drop_last)
        for ep in (0, 3):
            ours.set_epoch(ep)
            ref.set_epoch(ep)
            assert list(ours) == list(ref)
        assert len(ours) == len(ref)


def test_reference_epoch_arithmetic():
    ds = synthetic_cifar10(50000)
    for w in (1, 2, 4, 8):
        s = DistributedSampler(ds, num_replicas=w, rank=0) if w > 1 else None
        ld = DeviceLoader(ds, int(256 / w), sampler=s)
        assert len(ld) == 196


def test_cpu_loader_normalisation_and_augment():
    ds = synthetic_cifar10(32)
    x, y = next(iter(DeviceLoader(ds, 8, train=False)))
    ref = (ds.images[:8].permute(0, 3, 1, 2).float() / 255 - torch.tensor(ds.mean).view(1, 3, 1, 1)) / torch.tensor(
        ds.std).view(1, 3, 1, 1)
    assert torch.allclose(x, ref, atol=1e-6) and torch.equal(y, ds.labels[:8])
    xa, _ = next(iter(DeviceLoader(ds, 8, train=True, seed=1)))
    assert xa.shape == (8, 3, 32, 32)
    assert not torch.allclose(xa, x)


def test_cifar10_binary_reader(tmp_path):
    d = tmp_path / "cifar-10-batches-bin"
    d.mkdir()
    rng = np.random.default_rng(0)
    recs = {}
    for f in [f"data_batch_{i}.bin" for i in range(1, 6)] + ["test_batch.bin"]:
        a = rng.integers(0, 256, size=(3, 3073), dtype=np.uint8)
        a[:, 0] = rng.integers(0, 10, size=3)
        a.tofile(d / f)
        recs[f] = a
    tr = cifar10_binary(str(tmp_path), train=True)
    te = cifar10_binary(str(tmp_path), train=False)
    assert len(tr) == 15 and len(te) == 3
    a = recs["data_batch_1.bin"]
    assert int(tr.labels[0]) == int(a[0, 0])
    img = a[0, 1:].reshape(3, 32, 32).transpose(1, 2, 0)
    assert np.array_equal(tr.images[0].numpy(), img)


# ----------------------------------------------------------------------------- checkpoint
def test_checkpoint_roundtrip_and_torch_compat(tmp_path):
    torch.manual_seed(0)
    m = cdp.VGG11()
    o = cdp.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    cdp.CrossEntropyLoss()(m(torch.randn(2, 3, 32, 32)), torch.tensor([1, 2])).backward()
    o.step()
    path = save_checkpoint(str(tmp_path / "c.pt"), m, o, epoch=3, iteration=7)
    raw = torch.load(path, weights_only=True)
    assert raw["epoch"] == 3 and len(raw["model"]) == 58
    ref = cdp.VGG11(channels_last=False)
    ref.load_state_dict(raw["model"])  # plain torch layout
    m2 = cdp.VGG11()
    o2 = cdp.SGD(m2.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
    st = load_checkpoint(path, m2, o2)
    assert st["iteration"] == 7
    for a, b in zip(m.parameters(), m2.parameters()):
        assert torch.equal(a, b)
    ddp_sd = {"module." + k: v for k, v in raw["model"].items()}
    torch.save({"model": ddp_sd}, str(tmp_path / "ddp.pt"))
    m3 = cdp.VGG11()
    load_checkpoint(str(tmp_path / "ddp.pt"), m3)  # module. prefix stripped
    for a, b in zip(m.parameters(), m3.parameters()):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------- timers / tracing
def test_phase_timer_and_trace(tmp_path):
    t = PhaseTimer(None)
    t.mark("start")
    t.mark("forward")
    t.mark("backward")
    assert t.pop("forward") >= 0 and t.pop("backward") >= 0
    tr = TraceRecorder(0, None)
    with tr.phase("fwd"):
        pass
    p = tr.dump(str(tmp_path / "t.json"))
    ev = json.load(open(p))["traceEvents"]
    assert [e["name"] for e in ev if e["ph"] == "X"] == ["fwd"]


# ----------------------------------------------------------------------------- CLI
def test_train_cli_single_process_log_format():
    from cs744_distributed_data_parallel_amd import train

    buf = io.StringIO()
    with redirect_stdout(buf):
        train.main(["--epochs", "1", "--iters", "40", "--batch-size", "8", "--synthetic-size", "400",
                    "--device", "cpu"])
    out = buf.getvalue()
    assert "Size of training set is 50" in out
    # Part 1 prints "epochs" here (src/Part 1/main.py:49); only Part 3 (ddp) says "iterations"
    assert re.search(r"Training loss after 20 epochs is \d", out)
    assert re.search(r"Forward Pass time in iter 40 is ", out)
    assert re.search(r"Backward Pass time in iter 40 is ", out)
    assert re.search(r"Average Pass time in iter 40 is ", out)
    assert "Forward Pass time in iter 20" not in out  # first window discarded like the reference
    assert re.search(r"Training time after 1 epoch is ", out)
    assert re.search(r"Test set: Average loss: \d+\.\d{4}, Accuracy: \d+/400 \(\d+%\)", out)


def test_train_cli_ddp_log_format_and_trace(tmp_path):
    """Part 3 log string ("iterations") and --trace: phases plus the reducer's hook / bucket-launch
    events, with bucket launches interleaved with gradient-ready hooks (overlap)."""
    import os
    import subprocess
    import sys

    from _dist_util import free_port

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()), RANK="0", WORLD_SIZE="1",
               PYTHONPATH=repo, OMP_NUM_THREADS="2")
    tr = str(tmp_path / "trace.json")
    r = subprocess.run([sys.executable, "-m", "cs744_distributed_data_parallel_amd.train", "--strategy", "ddp",
                        "--backend", "gloo", "--device", "cpu", "--iters", "20", "--batch-size", "4",
                        "--synthetic-size", "80", "--bucket-cap-mb", "2", "--trace", tr],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Training loss after 20 iterations is \d", r.stdout), r.stdout
    ev = json.load(open(tr))["traceEvents"]
    phases = {e["name"] for e in ev if e["ph"] == "X"}
    assert {"forward", "backward", "step"} <= phases
    host = [e["name"] for e in ev if e["ph"] == "i"]
    assert sum(n.startswith("bucket_allreduce_launch") for n in host) >= 20 * 3
    assert host.count("backward_done") == 20
    # within the last iteration the first bucket launches before the last gradient is ready
    done = [i for i, n in enumerate(host) if n == "backward_done"]
    last = host[done[-2] + 1:done[-1]]
    first_launch = next(i for i, n in enumerate(last) if n.startswith("bucket_allreduce_launch"))
    last_hook = max(i for i, n in enumerate(last) if n.startswith("grad_ready"))
    assert first_launch < last_hook, last


# ----------------------------------------------------------------------------- native surface
def test_native_extension_surface():
    if not cdp.native_available():
        pytest.skip("native extension not built")
    C = cdp._native.lib()
    for name in ["conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv_bn_act_fwd", "conv_bn_act_bwd", "linear_fwd",
                 "linear_bwd", "xent_fwd", "xent_bwd", "sgd_step", "augment", "RcclComm", "Reducer"]:
        assert hasattr(C, name)
    assert C.ARCH == "gfx950"


def test_gpu_tensor_without_extension_raises(monkeypatch):
    from cs744_distributed_data_parallel_amd import _native

    class Fake:
        is_cuda = True

    monkeypatch.setattr(_native, "_C", None)
    monkeypatch.setattr(_native, "_err", RuntimeError("missing"))
    with pytest.raises(RuntimeError, match="native runtime"):
        _native.require(Fake())


# ----------------------------------------------------------------------------- bench.py contract
def _bench(args, env_extra=None, timeout=600):
    import os
    import subprocess
    import sys

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=repo, OMP_NUM_THREADS="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(repo, "bench.py")] + args, env=env, capture_output=True,
                          text=True, timeout=timeout, cwd=repo)


def test_bench_self_launches_ranks_cpu():
    """`bench.py --gpus 2` without WORLD_SIZE starts both ranks itself; rank 0 prints one JSON line
    with n_gpus == ranks_seen == 2, the strong-scaling point, the exposed-comm estimate and the
    reference's whole multi-process experiment: every sync strategy at its strong-scaling rule
    (int(global / W) images per rank), each with ms/step, exposed sync, scaling_eff and a
    bit-identical-replicas check -- BASELINE.md's Part 2a / 2b / 3 rows map onto these keys."""
    r = _bench(["--gpus", "2", "--device", "cpu", "--full", "--steps", "2", "--warmup", "1", "--local-batch", "4",
                "--global-batch", "16", "--dataset-size", "64"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["ranks_seen"] == 2
    assert rec["config"]["parallelism"] == "dp2" and rec["config"]["global_batch"] == 8
    assert rec["strong"]["global_batch"] == 16 and rec["strong"]["local_batch"] == 8
    assert rec["exposed_comm_ms"] >= 0 and rec["value"] > 0
    # self-verification: every rank holds the same parameters + momentum after the timed steps
    assert rec["replicas_identical"] is True
    assert rec["config"]["comm_fallback_reason"] is None and rec["config"]["graph_collectives"] is None
    assert rec["config"]["graph_fallbacks"] == []  # CPU steps are eager by design, not by a failed capture
    blk = rec["strategies"]
    assert blk["local_batch"] == 8 and blk["global_batch"] == 16 and blk["no_sync"]["ms_per_step"] > 0
    for strat, part in (("gather_scatter", "Part 2a"), ("allreduce_blocking", "Part 2b"),
                        ("bucketed_overlap", "config #3"), ("ddp", "Part 3")):
        e = blk[strat]
        assert part in e["reference"]
        assert e["ms_per_step"] > 0 and e["value"] > 0 and e["exposed_sync_ms"] >= 0
        assert 0 < e["scaling_eff"] <= 1.0
        assert e["replicas_identical"] is True, strat
    # the bucketed strategies report their plan in launch order
    for strat in ("bucketed_overlap", "ddp"):
        b = blk[strat]["buckets"]
        assert b["count"] == len(b["launch_order"]) >= 2
        assert sum(x["bytes"] for x in b["launch_order"]) >= 36_924_456  # every VGG-11 gradient
        # designed at the ready-order rebuild from the measured backward timeline + comm model
        assert b["planner"] == "timed" and b["backward_end_us"] > 0 and b["alpha_us"] >= 0
    assert set(rec["scaling_eff"]) == {"weak", "strong"}
    assert rec["scaling_eff"]["strong"] == blk["ddp"]["scaling_eff"]
    # BASELINE.json config #5 at N > 1: ResNet-50 under DDP with the timed bucket plan (reduced
    # 32x32 images in CPU mode)
    rn = rec["resnet50"]
    for k in ("ms_per_step", "ms_per_step_no_sync", "exposed_comm_ms", "scaling_eff", "value", "buckets",
              "replicas_identical", "local_batch", "global_batch"):
        assert k in rn, k
    assert rn["replicas_identical"] is True and rn["strategy"] == "ddp" and rn["global_batch"] == 2 * rn["local_batch"]
    assert 0 < rn["scaling_eff"] <= 1.0 and rn["exposed_comm_ms"] >= 0
    rb = rn["buckets"]
    assert rb["params"] == 161 and rb["count"] == len(rb["launch_order"]) >= 1
    assert sum(x["bytes"] for x in rb["launch_order"]) == 25_557_032 * 4  # every ResNet-50 gradient
    assert rb["planner"] == "timed"


def test_bench_launcher_at_eight_ranks_cpu():
    """The driver's largest point, rehearsed over gloo on the CPU: eight rank processes, one record."""
    r = _bench(["--gpus", "8", "--device", "cpu", "--steps", "1", "--warmup", "1", "--local-batch", "2",
                "--dataset-size", "32", "--no-extra"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 8 and rec["ranks_seen"] == 8 and rec["config"]["parallelism"] == "dp8"
    assert rec["config"]["global_batch"] == 16 and rec["replicas_identical"] is True


@pytest.mark.parametrize("strategy", ["gather_scatter", "allreduce_blocking", "bucketed_overlap"])
def test_bench_every_strategy_through_the_launcher_cpu(strategy):
    """Parts 2a / 2b / bucketed overlap through the same self-launching bench path (ddp is the
    default, covered above): each produces one record with both ranks seen."""
    r = _bench(["--gpus", "2", "--device", "cpu", "--strategy", strategy, "--steps", "1", "--warmup", "1",
                "--local-batch", "2", "--dataset-size", "16", "--no-extra"])
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["ranks_seen"] == 2 and rec["config"]["strategy"] == strategy
    assert rec["replicas_identical"] is True


def test_bench_failing_rank_fails_the_launcher():
    r = _bench(["--gpus", "2", "--device", "cpu", "--steps", "1", "--warmup", "1", "--local-batch", "2",
                "--dataset-size", "16", "--no-extra"], env_extra={"CDP_BENCH_FAIL_RANK": "1"})
    assert r.returncode != 0
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.parametrize("fault,phase", [("raise", "strong_allreduce_blocking"), ("hang", "strong_bucketed_overlap"),
                                         ("crash", "no_sync")])
def test_bench_failed_extra_keeps_the_headline(fault, phase):
    """A secondary measurement that raises, hangs or crashes on ONE rank (CDP_BENCH_FAULT) costs only
    its own block: the run exits 0 in bounded time with one JSON line carrying the headline, the named
    error in the failed block, and every other phase (before and after it) measured."""
    import time

    t0 = time.monotonic()
    r = _bench(["--gpus", "2", "--device", "cpu", "--full", "--steps", "1", "--warmup", "1", "--local-batch", "2",
                "--global-batch", "4", "--dataset-size", "16",
                "--extras", "no_sync,strong_allreduce_blocking,strong_bucketed_overlap"],
               env_extra={"CDP_BENCH_FAULT": f"{phase}:1:{fault}", "CDP_BENCH_PHASE_LIMIT_S": "30"}, timeout=300)
    assert time.monotonic() - t0 < 180
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["value"] > 0 and rec["ranks_seen"] == 2 and rec["replicas_identical"] is True
    st = {p["name"]: p for p in rec["phases"]}
    assert list(st) == ["headline", "no_sync", "strong_allreduce_blocking", "strong_bucketed_overlap"]
    assert st[phase]["status"] == "error"
    assert all(p["status"] == "ok" for n, p in st.items() if n != phase), st
    err = st[phase]["error"]
    if fault == "raise":
        assert "rank 1: RuntimeError: injected fault" in err, err
    elif fault == "hang":
        assert "timeout" in err, err
    else:
        assert "rank 1: worker exited with -9" in err, err
    if phase == "no_sync":
        assert rec["no_sync"]["error"] == err and "exposed_comm_ms" not in rec
    else:
        blk = rec["strategies"][phase[len("strong_"):]]
        assert blk["error"] == err and "ms_per_step" not in blk
    others = [s for s in ("allreduce_blocking", "bucketed_overlap") if s != phase[len("strong_"):]]
    for s in others:
        assert rec["strategies"][s]["replicas_identical"] is True


def test_bench_time_budget_skips_extras():
    """When the budget is spent before an extra could finish, that extra is skipped by agreement (every
    rank the same way) and the headline is still printed."""
    r = _bench(["--gpus", "2", "--device", "cpu", "--full", "--steps", "1", "--warmup", "1", "--local-batch", "2",
                "--global-batch", "4", "--dataset-size", "16", "--extras", "no_sync,strong_allreduce_blocking"],
               env_extra={"CDP_BENCH_BUDGET_S": "1", "CDP_BENCH_PHASE_LIMIT_S": "30"}, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    st = {p["name"]: p["status"] for p in rec["phases"]}
    assert st["headline"] == "ok"
    assert st["no_sync"].startswith("skipped: time budget") and st["strong_allreduce_blocking"].startswith("skipped")
    assert rec["value"] > 0


@pytest.mark.parametrize("strategy", ["ddp", "allreduce_blocking"])
def test_bench_detects_diverged_replicas(strategy):
    """One rank's gradient perturbed after the sync (CDP_BENCH_CORRUPT_RANK=1): the replicas differ
    after the timed steps, the record says so and the run fails (a broken reducer cannot produce a
    pretty number)."""
    r = _bench(["--gpus", "2", "--device", "cpu", "--strategy", strategy, "--steps", "1", "--warmup", "1",
                "--local-batch", "2", "--dataset-size", "16", "--no-extra"], env_extra={"CDP_BENCH_CORRUPT_RANK": "1"})
    assert r.returncode != 0
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["replicas_identical"] is False


def _npy_dir(path):
    return {n: np.load(os.path.join(path, n)) for n in sorted(os.listdir(path))}


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """Without --full a run measures the headline and nothing else (N = 2: one phase, no strategies
    block, no no-sync step), --steps is the number of timed steps the record divides by, and
    --dump-outputs writes the last timed step's outputs."""
    r = _bench(["--gpus", "2", "--device", "cpu", "--steps", "2", "--warmup", "1", "--local-batch", "2",
                "--dataset-size", "16", "--dump-outputs", str(tmp_path / "d")])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert [p["name"] for p in rec["phases"]] == ["headline"]
    for k in ("strategies", "strong", "exposed_comm_ms", "resnet50", "no_sync", "scaling_eff"):
        assert k not in rec, k
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["replicas_identical"] is True
    assert rec["value"] == pytest.approx(4 / rec["ms_per_step"] * 1e3, rel=1e-3)
    out = _npy_dir(str(tmp_path / "d"))
    assert out["loss.npy"].shape == () and out["logits.npy"].shape == (2, 10)
    assert out["param.fc1.weight.npy"].shape == (10, 512)


def test_bench_dump_outputs_repeats_bit_for_bit(tmp_path):
    """Same arguments, same inputs: two N = 1 runs dump the same arrays (float32, every parameter
    and buffer of VGG-11 whole, within the 64 MB limit), and more timed steps give other values."""
    args = ["--gpus", "1", "--device", "cpu", "--warmup", "1", "--local-batch", "4", "--dataset-size", "32"]
    outs = []
    for name, steps in (("a", "2"), ("b", "2"), ("c", "3")):
        r = _bench(args + ["--steps", steps, "--dump-outputs", str(tmp_path / name)])
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(_npy_dir(str(tmp_path / name)))
    a, b, c = outs
    assert list(a) == list(b) == list(c) and "loss.npy" in a and "logits.npy" in a
    assert sum(1 for n in a if n.startswith("param.")) == 34
    assert sum(x.nbytes for x in a.values()) <= 64 * 10**6
    for n in a:
        assert a[n].dtype == np.float32 and np.isfinite(a[n]).all(), n
        np.testing.assert_array_equal(a[n], b[n], err_msg=n)
    assert a["param.layers.0.weight.npy"].shape == (64, 3, 3, 3)
    assert not np.array_equal(a["param.fc1.weight.npy"], c["param.fc1.weight.npy"])


def test_bench_dump_samples_large_outputs(tmp_path):
    """Over the budget every large tensor is cut to the same seeded, sorted choice of its elements;
    small ones stay whole."""
    import bench

    g = torch.Generator().manual_seed(0)
    named = {"big0": torch.randn(9_000_000, generator=g), "small": torch.arange(10.0),
             "big1": torch.randn(3000, 3000, generator=g)}
    bench._dump_outputs(str(tmp_path / "a"), named)
    bench._dump_outputs(str(tmp_path / "b"), named)
    a, b = _npy_dir(str(tmp_path / "a")), _npy_dir(str(tmp_path / "b"))
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_BUDGET_BYTES <= 64 * 10**6
    np.testing.assert_array_equal(a["small.npy"], np.arange(10.0, dtype=np.float32))
    for n in ("big0.npy", "big1.npy"):
        np.testing.assert_array_equal(a[n], b[n])
        assert a[n].ndim == 1 and 0.6 < a[n].size / 9_000_000 < 0.72  # 48 MiB / 72 MB of big tensors
    assert np.isin(a["big0.npy"], named["big0"].numpy()).all()
