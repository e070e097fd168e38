"""RandomResizedCrop and resize + center crop on the CPU path of DeviceLoader: the shared checks of
_rrc_util.py, the draws' independence of the other generators, and the CLI flags."""
import io
import re
from contextlib import redirect_stderr, redirect_stdout

import pytest
import torch

from _mix_util import MIX, dataset
from _rrc_util import (MIX_CASES, PIXEL_CASES, check_argument_errors, check_defaults_change_nothing, check_eval,
                       check_mixing_composes, check_pixels)


@pytest.mark.parametrize("B,H,W,OH,OW", PIXEL_CASES)
def test_cpu_resized_pixels_match_fp64(B, H, W, OH, OW):
    check_pixels(B, H, W, OH, OW, "cpu")


def test_cpu_eval_resize_and_center_crop():
    check_eval("cpu")


def test_cpu_default_resize_arguments_change_nothing():
    check_defaults_change_nothing("cpu")


@pytest.mark.parametrize("B,H,W,OH,OW", MIX_CASES)
def test_cpu_mixing_composes_with_the_resize(B, H, W, OH, OW):
    check_mixing_composes(B, H, W, OH, OW, "cpu")


def test_cpu_resize_argument_errors():
    check_argument_errors("cpu")


def test_cpu_crop_draws_leave_the_mix_draws_and_the_global_rng_alone():
    """The windows come from a generator of their own: the mix rows of a resizing loader whose output has the
    stored size are those of a loader without the resize, and torch's default generator is untouched."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    ds = dataset(4, 8, 8, "cpu")
    idx = torch.arange(len(ds))
    a = DeviceLoader(ds, 4, seed=2, rrc_scale=(0.3, 1.0), **MIX)
    b = DeviceLoader(ds, 4, seed=2, **MIX)
    torch.manual_seed(77)
    want = torch.rand(3)
    torch.manual_seed(77)
    for k in range(4):
        assert int(a._counter.item()) == k
        _, ta = a.batch(idx, 0, 4)
        _, tb = b.batch(idx, 0, 4)
        assert torch.equal(ta.info, tb.info), k
    assert torch.equal(torch.rand(3), want)


def test_train_cli_resize_flags_keep_the_reference_lines():
    """ResNet-18 on 40 x 40 stored images cropped to 32: the run ends, stdout's line set is that of a run
    without the flags, and stderr carries the crop line of iteration 20."""
    from cs744_distributed_data_parallel_amd import train

    def cli(extra):
        out, err = io.StringIO(), io.StringIO()
        with redirect_stdout(out), redirect_stderr(err):
            train.main(["--device", "cpu", "--model", "resnet18", "--synthetic-size", "40", "--batch-size", "2",
                        "--epochs", "1"] + extra)
        return out.getvalue(), err.getvalue()

    strip = lambda s: [re.sub(r"-?\d+\.\d+(e-?\d+)?", "#", ln) for ln in s.splitlines()]  # noqa: E731
    plain, perr = cli(["--stored-size", "32"])
    sized, err = cli(["--stored-size", "40", "--crop-size", "32", "--rrc-scale", "0.35", "1", "--center-crop", "0.875"])
    assert strip(plain) == strip(sized)
    lines = [ln for ln in err.splitlines() if "crop of image 0 in iter" in ln]
    assert len(lines) == 1 and re.fullmatch(r"\[cdp\] rank 0: crop of image 0 in iter 20 is \d+ x \d+ at \(\d+, \d+\)",
                                            lines[0]), err
    assert "crop of image" not in perr and "crop of image" not in sized
