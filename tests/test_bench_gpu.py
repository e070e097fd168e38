"""bench.py on the GPU: a plain run is the headline alone, and --dump-outputs hands out what the
captured step's last replay computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_replayed_step(tmp_path):
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=repo)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(repo, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2",
                        "--local-batch", "32", "--dataset-size", "512", "--dump-outputs", d],
                       env=env, capture_output=True, text=True, timeout=200, cwd=repo)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert rec["config"]["hipgraph"] is True and rec["steps"] == 5 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(32 / rec["ms_per_step"] * 1e3, rel=1e-3)
    for k in ("strict_fp32", "per_gpu_strong", "resnet50"):  # --full only
        assert k not in rec, k
    out = {n: np.load(os.path.join(d, n)) for n in os.listdir(d)}
    assert sum(1 for n in out if n.startswith("param.")) == 34
    assert sum(a.nbytes for a in out.values()) <= 64 * 10**6
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    # loss and logits are of the same (last) step: a mean cross-entropy lies between the mean of
    # logsumexp - max logit and the mean of logsumexp - min logit, whatever the labels are
    z = out["logits.npy"].astype(np.float64)
    assert z.shape == (32, 10) and out["loss.npy"].shape == ()
    lse = np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1)
    assert (lse - z.max(1)).mean() - 1e-5 <= float(out["loss.npy"]) <= (lse - z.min(1)).mean() + 1e-5
