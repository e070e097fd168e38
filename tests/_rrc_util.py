"""Shared checks of the resizing DeviceLoader (RandomResizedCrop, resize + center crop), run on the GPU
kernel (test_rrc_gpu.py) and on the CPU path (test_rrc_cpu.py) with the same assertions."""
import pytest
import torch
import torch.nn.functional as F

from _mix_util import MIX, STEPS, dataset

# (B, H, W, OH, OW): square; non-square both ways (an axis swap shows); a downscale to an odd width (the
# scalar tail); a heavy upscale (many clamped edges, more than one workgroup); a 5x downscale
PIXEL_CASES = [(4, 8, 8, 8, 8), (3, 6, 10, 10, 6), (2, 12, 9, 5, 7), (2, 5, 7, 40, 40), (1, 40, 40, 8, 8)]
MIX_CASES = [(4, 8, 8, 8, 8), (5, 6, 10, 8, 12), (2, 12, 12, 40, 40)]
RRC_STEPS = 6


def pixel_bound(ds):
    """Against fp64, in normalised units. The blend of four values <= 255: 2 weight roundings (the two
    lam divisions), 2 complement roundings (1 - lam), 6 products and 3 sums, each at most 2^-24 * 255,
    i.e. 2^-24 / std after the normalisation; the normalise adds 3 more operations (v / 255, - mean,
    * 1 / std; the kernel fuses the first two, and rounds mean and 1 / std to fp32 once) on values of at most
    (1 + mean) / std. 16 in all, each bounded by 2^-24 * max_c((1 + mean_c) / std_c)."""
    return 16 * 2.0 ** -24 * max((1 + m) / s for m, s in zip(ds.mean, ds.std))


def fp64_batch(ds, src, crops, OH, OW):
    """fp64 build of a batch from its published rows {top, left, h, w, flip}: cut the window from the
    stored image, F.interpolate, flip, normalise. src: the dataset indices of the batch."""
    imgs = ds.images.cpu()
    mean = torch.tensor(ds.mean, dtype=torch.float64).view(3, 1, 1)
    std = torch.tensor(ds.std, dtype=torch.float64).view(3, 1, 1)
    out = []
    for i, (top, left, h, w, fl) in zip(src.tolist(), crops.tolist()):
        win = imgs[i, top : top + h, left : left + w].permute(2, 0, 1).double()[None]
        r = F.interpolate(win, (OH, OW), mode="bilinear", align_corners=False)[0]
        if fl:
            r = r.flip(-1)
        out.append((r / 255.0 - mean) / std)
    return torch.stack(out)


def assert_windows_in_bounds(crops, H, W):
    top, left, h, w = (crops[:, k] for k in range(4))
    assert ((top >= 0) & (top + h <= H) & (left >= 0) & (left + w <= W) & (h >= 1) & (w >= 1)).all(), crops


def check_pixels(B, H, W, OH, OW, device, seed=11):
    """Check 1: every pixel of RRC_STEPS consecutive batches against the fp64 build of its published window."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    ds = dataset(B, H, W, device)
    ld = DeviceLoader(ds, B, seed=seed, rrc_scale=(0.08, 1.0), out_size=(OH, OW))
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(device)
    bound = pixel_bound(ds)
    worst, flips, distinct = 0.0, set(), False
    for step in range(RRC_STEPS):
        off = 1 + (step % 2) * B
        out, y = ld.batch(idx, off, B)
        src = idx[off : off + B].cpu()
        crops = ld.last_crops.cpu()
        assert crops.shape == (B, 5) and crops.dtype == torch.int32
        assert out.shape == (B, 3, OH, OW) and out.dtype == torch.float32
        assert out.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(y.cpu(), ds.labels.cpu()[src]), step
        assert_windows_in_bounds(crops, H, W)
        flips.update(crops[:, 4].tolist())
        distinct = distinct or len({tuple(r) for r in crops[:, :4].tolist()}) > 1
        err = (out.cpu().double() - fp64_batch(ds, src, crops, OH, OW)).abs().max().item()
        worst = max(worst, err)
    print(f"{device} {(B, H, W, OH, OW)}: worst pixel error {worst:.3e} bound {bound:.3e}")
    assert worst <= bound, (worst, bound)
    assert flips == {0, 1}, flips
    assert distinct or B == 1


def check_eval(device):
    """Check 2: the central window, its pixels, determinism, and the identity resize."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 3, 16, 12
    ds = dataset(B, H, W, device)
    idx = torch.arange(len(ds), device=device)
    ld = DeviceLoader(ds, B, train=False, center_crop=0.875, out_size=(7, 9))
    a, ya = ld.batch(idx, 2, B)
    crops = ld.last_crops.cpu()
    assert crops.tolist() == [[1, 1, 14, 10, 0]] * B, crops
    b, yb = ld.batch(idx, 2, B)
    assert torch.equal(a, b) and torch.equal(ya, yb) and torch.equal(ya.cpu(), ds.labels.cpu()[2 : 2 + B])
    assert a.shape == (B, 3, 7, 9) and a.is_contiguous(memory_format=torch.channels_last)
    bound = pixel_bound(ds)
    err = (a.cpu().double() - fp64_batch(ds, torch.arange(2, 2 + B), crops, 7, 9)).abs().max().item()
    print(f"{device} eval: pixel error {err:.3e} bound {bound:.3e}")
    assert err <= bound
    # the whole image at the stored size: every lam is 0, the batch is the plain evaluation loader's
    full = DeviceLoader(ds, B, train=False, center_crop=1.0, out_size=(H, W))
    plain = DeviceLoader(ds, B, train=False)
    xf, _ = full.batch(idx, 0, B)
    xp, _ = plain.batch(idx, 0, B)
    assert full.last_crops.cpu().tolist() == [[0, 0, H, W, 0]] * B and plain.last_crops is None
    err = (xf.double() - xp.double()).abs().max().item()
    print(f"{device} eval identity: difference to the plain loader {err:.3e} bound {bound:.3e}")
    assert err <= bound


def check_defaults_change_nothing(device):
    """Check 3."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 4, 8, 8
    ds = dataset(B, H, W, device)
    idx = torch.arange(len(ds), device=device)
    for train in (True, False):
        a = DeviceLoader(ds, B, seed=5, train=train, out_size=None, rrc_scale=None, rrc_ratio=(3 / 4, 4 / 3),
                         center_crop=None)
        b = DeviceLoader(ds, B, seed=5, train=train)
        for _ in range(3):
            xa, ta = a.batch(idx, 0, B)
            xb, tb = b.batch(idx, 0, B)
            assert torch.equal(xa, xb) and torch.equal(ta, tb), train
        assert a.last_crops is None and not a.resizing


def check_mixing_composes(B, H, W, OH, OW, device, seed=11):
    """Check 4: check_mixed_batches' assertions against the plain resized batch X of a twin loader."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, MixTarget

    ds = dataset(B, H, W, device)
    kw = dict(rrc_scale=(0.25, 1.0), out_size=(OH, OW))
    mixed = DeviceLoader(ds, B, seed=seed, **MIX, **kw)
    plain = DeviceLoader(ds, B, seed=seed, **kw)
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(device)
    seen = set()
    for step in range(STEPS):
        off = 1 + (step % 2) * B
        out, tgt = mixed.batch(idx, off, B)
        X, y = plain.batch(idx, off, B)
        assert isinstance(tgt, MixTarget) and torch.is_tensor(y)
        assert out.shape == X.shape == (B, 3, OH, OW) and out.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(mixed.last_crops, plain.last_crops), step
        info = tgt.info.cpu()
        mode, lam, lam_raw = int(info[0]), info[1].item(), info[2].item()
        y0, y1, x0, x1 = (int(v) for v in info[3:7])
        assert torch.equal(tgt.target, y) and torch.equal(tgt.target_b, y.flip(0)), step
        seen.add(mode)
        Xp = X.flip(0)
        if mode == 0:
            assert torch.equal(out, X) and lam == 1.0, step
        elif mode == 2:
            assert 0 <= y0 <= y1 <= OH and 0 <= x0 <= x1 <= OW, (step, info)
            box = torch.zeros(1, 1, OH, OW, dtype=torch.bool, device=X.device)
            box[..., y0:y1, x0:x1] = True
            assert torch.equal(out, torch.where(box, Xp, X)), step
            want = torch.tensor(1.0 - (y1 - y0) * (x1 - x0) / (OH * OW), dtype=torch.float64).float().item()
            assert lam == want, (step, lam, want)
        else:
            assert mode == 1 and lam == lam_raw and 0.0 <= lam <= 1.0, (step, info)
            ref = lam * X.double() + (1.0 - lam) * Xp.double()
            # two products, one sum and the rounding of 1 - lam, each at most half an ulp
            bound = 4 * 2.0 ** -24 * X.abs().max().item()
            err = (out.double() - ref).abs().max().item()
            print(f"step {step}: mixup lam {lam:.6f} err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (step, err, bound)
    assert seen == {0, 1, 2}, seen


def check_argument_errors(device):
    """Check 5."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    ds = dataset(4, 8, 8, device)
    for kw in (dict(rrc_scale=(0.5, 0.2)), dict(rrc_scale=(0, 1)), dict(rrc_scale=(0.1, 1.5)),
               dict(rrc_ratio=(2, 1)), dict(center_crop=0), dict(center_crop=1.2), dict(out_size=0),
               dict(train=True, out_size=16)):
        with pytest.raises(ValueError):
            DeviceLoader(ds, 4, **kw)
