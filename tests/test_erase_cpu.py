"""RandomErasing on the CPU path of DeviceLoader: the shared checks of _erase_util.py, the draws'
independence of the other generators, and the CLI flags."""
import io
import re
from contextlib import redirect_stderr, redirect_stdout

import pytest
import torch

from _erase_util import (FILLS, PLAIN_CASES, PROB, RESIZE_CASES, SCALES, check_argument_errors,
                         check_defaults_change_nothing, check_draw_statistics, check_erased_pixels,
                         check_mixing_composes, check_noise_moments)
from _mix_util import MIX, dataset


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("case", PLAIN_CASES + RESIZE_CASES)
def test_cpu_erased_pixels_follow_the_plain_batch(case, scale):
    check_erased_pixels(case, scale, "cpu")


def test_cpu_noise_moments():
    check_noise_moments("cpu")


def test_cpu_draw_statistics():
    check_draw_statistics("cpu")


@pytest.mark.parametrize("fill", [FILLS[3], dict()], ids=["pixel", "const0"])
@pytest.mark.parametrize("case", [(4, 8, 8), (5, 8, 8), (5, 6, 10, 8, 12)])
def test_cpu_mixing_composes_with_erasing(case, fill):
    check_mixing_composes(case, "cpu", fill)


def test_cpu_default_erase_arguments_change_nothing():
    check_defaults_change_nothing("cpu")


def test_cpu_erase_argument_errors():
    check_argument_errors("cpu")


def test_cpu_erase_draws_leave_the_other_draws_and_the_global_rng_alone():
    """The boxes and the noise come from generators of their own: windows, flips and mix rows are those of a
    loader without erasing, and torch's default generator is untouched."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    ds = dataset(4, 8, 8, "cpu")
    idx = torch.arange(len(ds))
    kw = dict(seed=2, rrc_scale=(0.3, 1.0), **MIX)
    a = DeviceLoader(ds, 4, erase_prob=PROB, erase_mode="pixel", **kw)
    b = DeviceLoader(ds, 4, **kw)
    torch.manual_seed(77)
    want = torch.rand(3)
    torch.manual_seed(77)
    for k in range(4):
        assert int(a._counter.item()) == k
        _, ta = a.batch(idx, 0, 4)
        _, tb = b.batch(idx, 0, 4)
        assert torch.equal(ta.info, tb.info) and torch.equal(a.last_crops, b.last_crops), k
    assert torch.equal(torch.rand(3), want)


def test_train_cli_erase_flags_keep_the_reference_lines():
    """VGG-11 on 21 batches of 2: the run ends, stdout's line set is that of a run without the flags, and
    stderr carries the erase line of iteration 20."""
    from cs744_distributed_data_parallel_amd import train

    def cli(extra):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(["--device", "cpu", "--model", "vgg11", "--synthetic-size", "42", "--batch-size", "2",
                        "--epochs", "1"] + extra)
        return out.getvalue(), err.getvalue()

    # (every number: the erased run trains on other pixels, so its test accuracy count may differ too)
    strip = lambda s: [re.sub(r"-?\d+(\.\d+)?(e-?\d+)?", "#", ln) for ln in s.splitlines()]  # noqa: E731
    plain, perr = cli([])
    erased, err = cli(["--random-erase", "0.5", "--erase-mode", "pixel", "--erase-scale", "0.1", "0.4",
                       "--erase-ratio", "0.5", "2"])
    assert strip(plain) == strip(erased)
    lines = [ln for ln in err.splitlines() if "erase of image 0 in iter" in ln]
    assert len(lines) == 1 and re.fullmatch(
        r"\[cdp\] rank 0: erase of image 0 in iter 20 is (none|\d+ x \d+ at \(\d+, \d+\))", lines[0]), err
    assert "erase of image" not in perr and "erase of image" not in erased
