"""The training CLI with RandomErasing on the GPU, together with RandomResizedCrop and mixup: 21 iterations
of VGG-11 end with a finite loss line on stdout and one erase line on stderr."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the reference's stdout lines
STDOUT_LINES = [r"Size of training set is \d+", r"Size of test set is \d+",
                r"Training loss after \d+ epochs is (?:tensor\()?[-0-9.eE+naif]+.*",
                r"(Forward|Backward|Average) Pass time in iter \d+ is [-0-9.eE+]+",
                r"Training time after \d+ epoch is [-0-9.eE+]+",
                r"Test set: Average loss: [-0-9.eE+naif]+, Accuracy: \d+/\d+ \(\d+%\)", r""]


def test_train_cli_with_erasing_on_the_gpu():
    """(336 synthetic images: 21 batches of 16, so that the epoch reaches iteration 20 and its log lines.)"""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "cs744_distributed_data_parallel_amd.train", "--model", "vgg11",
                        "--synthetic-size", "336", "--batch-size", "16", "--iters", "21", "--random-erase", "0.5",
                        "--erase-mode", "pixel", "--rrc-scale", "0.08", "1", "--mixup-alpha", "0.2"],
                       env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    losses = re.findall(r"Training loss after 20 epochs is (?:tensor\()?([-0-9.eE+naif]+)", r.stdout)
    assert len(losses) == 1 and math.isfinite(float(losses[0])), r.stdout
    for ln in r.stdout.splitlines():
        assert any(re.fullmatch(p, ln) for p in STDOUT_LINES), ln
    erase = [ln for ln in r.stderr.splitlines() if "erase of image 0 in iter" in ln]
    assert len(erase) == 1 and re.fullmatch(
        r"\[cdp\] rank 0: erase of image 0 in iter 20 is (none|\d+ x \d+ at \(\d+, \d+\))", erase[0]), r.stderr[-3000:]
    assert "erase of image" not in r.stdout
