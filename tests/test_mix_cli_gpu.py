"""The training CLI with mixup + CutMix on the GPU: 21 iterations of VGG-11 end with a finite loss
line on stdout and one mix line on stderr."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_cli_with_mixing_on_the_gpu():
    """(336 synthetic images: 21 batches of 16, so that the epoch reaches iteration 20 and its log lines.)"""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "cs744_distributed_data_parallel_amd.train", "--model", "vgg11",
                        "--synthetic-size", "336", "--batch-size", "16", "--iters", "21", "--mixup-alpha", "0.2",
                        "--cutmix-alpha", "1.0"], env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    losses = re.findall(r"Training loss after 20 epochs is (?:tensor\()?([-0-9.eE+naif]+)", r.stdout)
    assert len(losses) == 1 and math.isfinite(float(losses[0])), r.stdout
    mix = [ln for ln in r.stderr.splitlines() if "mix in iter" in ln]
    assert len(mix) == 1 and re.fullmatch(r"\[cdp\] rank 0: mix in iter 20 is mode (none|mixup|cutmix) lam [\d.e-]+",
                                          mix[0]), r.stderr[-3000:]
    assert "mix in iter" not in r.stdout
