"""Shared checks of the RandAugment DeviceLoader, run on the GPU kernel (test_randaug_gpu.py) and on the CPU
path (test_randaug_cpu.py)."""
import math

import pytest
import torch

from _mix_util import MIX, dataset

# (B, H, W, OH, OW): the resizing loader's cases of _rrc_util with the heavy upscale at 33 x 35 = 1155 output
# pixels: more than one pass of a 1024-thread workgroup, and many clamped edges
RESIZE_SHAPES = [(4, 8, 8, 8, 8), (3, 6, 10, 10, 6), (2, 12, 9, 5, 7), (2, 5, 7, 33, 35), (1, 40, 40, 8, 8)]
PLAIN_SHAPES = [(5, 32, 32), (3, 9, 7)]  # (B, H, W), pad = 4
PAD = 4
SEED = 11
STEPS = 3
RRC = dict(rrc_scale=(0.25, 1.0))
ERASE = dict(erase_prob=0.6, erase_mode="pixel")


def names():
    from cs744_distributed_data_parallel_amd.randaug import RANDAUG_OPS

    return RANDAUG_OPS


def make_dataset(B, H, W, device):
    ds = dataset(B, H, W, device)
    ds.pad = PAD
    return ds


def loader(ds, B, out_size=None, seed=SEED, **kw):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    if out_size is not None:
        kw = dict(RRC, out_size=out_size, **kw)
    return DeviceLoader(ds, B, seed=seed, **kw)


def staged_input(ds, ld, src, ctr):
    """The twin's staging of a batch: from the published crops (resize) or the augment hash's own crop / flip."""
    from cs744_distributed_data_parallel_amd import randaug as ra

    imgs = ds.images.cpu()[src]
    if ld.resizing:
        return ra.stage_resize(imgs, ld.last_crops.cpu(), *ld.out_size)
    oy, ox, fl = ra.aug_crop_flip(ld.seed, ctr, len(src), ds.pad, True)
    return ra.stage_plain(imgs, oy, ox, fl)


def normalise(ds, u8):
    """(v / 255 - mean) / std of a uint8 NHWC batch in fp64, NCHW."""
    mean = torch.tensor(ds.mean, dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(ds.std, dtype=torch.float64).view(1, 3, 1, 1)
    return (u8.cpu().permute(0, 3, 1, 2).double() / 255.0 - mean) / std


def check_pixels_bitwise(device, op_names, num_ops):
    """Check 6: last_randaug_images against randaug_reference of the twin's staging, on every shape and both paths.
    Returns the op kinds and signs seen."""
    from cs744_distributed_data_parallel_amd.randaug import randaug_reference

    kinds, signs = set(), set()
    cases = [(B, H, W, (OH, OW)) for B, H, W, OH, OW in RESIZE_SHAPES] + [(B, H, W, None) for B, H, W in PLAIN_SHAPES]
    for B, H, W, out_size in cases:
        ds = make_dataset(B, H, W, device)
        ld = loader(ds, B, out_size, randaug_num_ops=num_ops, randaug_magnitude=15.0, randaug_mstd=0.5,
                    randaug_ops=op_names)
        idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(device)
        for step in range(STEPS):
            off = 1 + (step % 2) * B
            out, y = ld.batch(idx, off, B)
            src = idx[off : off + B].cpu()
            OH, OW = out_size or (H, W)
            rows = ld.last_randaug.cpu()
            got = ld.last_randaug_images.cpu()
            assert rows.shape == (B, num_ops, 8) and rows.dtype == torch.int32
            assert got.shape == (B, OH, OW, 3) and got.dtype == torch.uint8
            assert out.shape == (B, 3, OH, OW) and out.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(y.cpu(), ds.labels.cpu()[src]), (B, H, W, out_size, step)
            want = randaug_reference(staged_input(ds, ld, src, step), rows, ld.randaug_fill)
            assert torch.equal(got, want), (op_names, B, H, W, out_size, step, rows.tolist())
            kinds.update((rows[..., 0] & 255).flatten().tolist())
            signs.update((rows[..., 0] >> 8).flatten().tolist())
            assert set((rows[..., 0] & 255).flatten().tolist()) <= {names().index(n) for n in op_names}
    return kinds, signs


def check_argument_errors(device):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, ImageDataset

    ds = make_dataset(4, 8, 8, device)
    for kw in (dict(randaug_num_ops=-1), dict(randaug_num_ops=9), dict(randaug_num_ops=2, randaug_magnitude=-0.5),
               dict(randaug_num_ops=2, randaug_magnitude=30.5), dict(randaug_num_ops=2, randaug_mstd=-1.0),
               dict(randaug_num_ops=2, randaug_ops=("Rotate", "Invert")), dict(randaug_num_ops=2, randaug_ops=()),
               dict(randaug_num_ops=2, randaug_fill=(0, 0)), dict(randaug_num_ops=2, randaug_fill=(0, 0, 256)),
               dict(randaug_num_ops=2, randaug_fill=(0.5, 1, 2)), dict(randaug_num_ops=2, randaug_fill=(-1, 1, 2))):
        with pytest.raises(ValueError):
            DeviceLoader(ds, 4, **kw)
    gray = ImageDataset(ds.images[..., :1].contiguous(), ds.labels, [0.5], [0.25], pad=0)
    with pytest.raises(ValueError):
        DeviceLoader(gray, 4, randaug_num_ops=1)
    DeviceLoader(gray, 4, randaug_num_ops=1, train=False)  # an evaluation loader ignores the arguments


def check_defaults_change_nothing(device):
    """The new arguments at their defaults, and an evaluation loader with them set: bitwise the loader without."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 4, 8, 8
    ds = make_dataset(B, H, W, device)
    idx = torch.arange(len(ds), device=device)
    for train, kw in ((True, dict(randaug_num_ops=0, randaug_magnitude=9.0, randaug_mstd=0.0, randaug_ops=None,
                                  randaug_fill=None)),
                      (False, dict(randaug_num_ops=2, randaug_magnitude=20.0))):
        a = DeviceLoader(ds, B, seed=5, train=train, **kw)
        b = DeviceLoader(ds, B, seed=5, train=train)
        for _ in range(3):
            xa, ta = a.batch(idx, 0, B)
            xb, tb = b.batch(idx, 0, B)
            assert torch.equal(xa, xb) and torch.equal(ta, tb), train
        assert a.last_randaug is None and a.last_randaug_images is None and not a.randaugmenting


def band(N, p):
    return 5.0 * math.sqrt(N * p * (1.0 - p))


def check_distribution(rows):
    """Check 11 on int rows [..., 8]: every op's count and the sign share inside 5 sigma."""
    ops = (rows[..., 0] & 255).flatten()
    N = ops.numel()
    counts = torch.bincount(ops, minlength=14)
    print("op counts", counts.tolist(), "band", band(N, 1 / 14))
    assert ((counts.double() - N / 14).abs() <= band(N, 1 / 14)).all(), counts
    neg = int((rows[..., 0] >> 8).sum())
    print("negative signs", neg, "of", N, "band", band(N, 0.5))
    assert abs(neg - N / 2) <= band(N, 0.5), neg
