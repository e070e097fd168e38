"""Shared checks of the mixed batches (mixup / CutMix) of DeviceLoader, run on the GPU kernel
(test_mix_gpu.py) and on the CPU path (test_mix_cpu.py) with the same assertions."""
import torch

# (B, H, W): an even batch; an odd one (the middle image pairs with itself); a non-square image (an
# H / W swap in the box shows); more than one workgroup of pixels per image
CASES = [(4, 8, 8), (5, 8, 8), (3, 6, 10), (2, 40, 40)]
MIX = dict(mixup_alpha=0.4, cutmix_alpha=1.0, mix_prob=0.7, mix_switch_prob=0.5)
STEPS = 24  # consecutive counters: P(a mode missing) < 3 * 0.7^24 = 6e-4 a priori; fixed seed, asserted below


def dataset(B, H, W, device):
    from cs744_distributed_data_parallel_amd.data import ImageDataset

    g = torch.Generator().manual_seed(100 * B + H)
    n = 3 * B + 1
    imgs = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int64, generator=g)
    return ImageDataset(imgs, labels, [0.49, 0.48, 0.45], [0.25, 0.24, 0.26], pad=2).to(device)


def check_mixed_batches(B, H, W, device, seed=11):
    """Every mode against the unmixed batch X, y of a twin loader at the same seed and counter."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, MixTarget

    ds = dataset(B, H, W, device)
    mixed = DeviceLoader(ds, B, seed=seed, **MIX)
    plain = DeviceLoader(ds, B, seed=seed)
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(device)
    seen = set()
    for step in range(STEPS):
        off = 1 + (step % 2) * B
        out, tgt = mixed.batch(idx, off, B)
        X, y = plain.batch(idx, off, B)
        assert isinstance(tgt, MixTarget) and torch.is_tensor(y)
        assert out.shape == X.shape and out.is_contiguous(memory_format=torch.channels_last)
        info = tgt.info.cpu()
        mode, lam, lam_raw = int(info[0]), info[1].item(), info[2].item()
        y0, y1, x0, x1 = (int(v) for v in info[3:7])
        assert info[7].item() == 0 and tgt.lam.shape == (1,) and tgt.lam.item() == lam
        assert tgt.lam.data_ptr() == tgt.info[1:2].data_ptr()  # a view of the published row
        # labels: the image's own, and its partner's (batch reversal)
        assert torch.equal(tgt.target, y) and torch.equal(tgt.target_b, y.flip(0)), step
        seen.add(mode)
        Xp = X.flip(0)
        if mode == 0:
            assert torch.equal(out, X) and lam == 1.0, step
        elif mode == 2:
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W, (step, info)
            box = torch.zeros(1, 1, H, W, dtype=torch.bool, device=X.device)
            box[..., y0:y1, x0:x1] = True
            assert torch.equal(out, torch.where(box, Xp, X)), step
            want = torch.tensor(1.0 - (y1 - y0) * (x1 - x0) / (H * W), dtype=torch.float64).float().item()
            assert lam == want, (step, lam, want)
            assert 0.0 <= lam_raw <= 1.0
        else:
            assert mode == 1 and lam == lam_raw and 0.0 <= lam <= 1.0, (step, info)
            ref = lam * X.double() + (1.0 - lam) * Xp.double()
            # two products, one sum and the rounding of 1 - lam, each at most half an ulp
            bound = 4 * 2.0 ** -24 * X.abs().max().item()
            err = (out.double() - ref).abs().max().item()
            print(f"step {step}: mixup lam {lam:.6f} err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (step, err, bound)
    assert seen == {0, 1, 2}, seen


def check_default_arguments_change_nothing(device):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 4, 8, 8
    ds = dataset(B, H, W, device)
    a = DeviceLoader(ds, B, seed=5, mixup_alpha=0.0, cutmix_alpha=0.0, mix_prob=1.0, mix_switch_prob=0.5)
    b = DeviceLoader(ds, B, seed=5)
    idx = torch.arange(len(ds), device=device)
    for _ in range(3):
        xa, ta = a.batch(idx, 0, B)
        xb, tb = b.batch(idx, 0, B)
        assert torch.is_tensor(ta) and not isinstance(ta, tuple)
        assert torch.equal(xa, xb) and torch.equal(ta, tb)
    assert not a.mixing
    # an evaluation loader never mixes
    e = DeviceLoader(ds, B, train=False, mixup_alpha=0.5)
    assert not e.mixing and torch.is_tensor(e.batch(idx, 0, B)[1])
