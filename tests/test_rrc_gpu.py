"""Fused RandomResizedCrop and resize + center crop: augment_resize_kernel against fp64 at its published
windows (eagerly and in replays of a captured batch), the device-side window stream (rrc_draw /
rrc_params) against the published rule, its independence of the flip and mix streams, the MIX
instantiation against the plain resized batch, the op's argument checks and one training step."""
import math

import pytest
import torch

from _mix_util import MIX, dataset
from _rrc_util import (MIX_CASES, PIXEL_CASES, assert_windows_in_bounds, check_argument_errors,
                       check_defaults_change_nothing, check_eval, check_mixing_composes, check_pixels, fp64_batch,
                       pixel_bound)

pytestmark = pytest.mark.gpu

RATIO = (3 / 4, 4 / 3)


def _lib():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


# ------------------------------------------------------------------------------- shared checks
@pytest.mark.parametrize("B,H,W,OH,OW", PIXEL_CASES)
def test_resized_pixels_match_fp64(B, H, W, OH, OW):
    check_pixels(B, H, W, OH, OW, "cuda")


@pytest.mark.parametrize("OW", [1028, 1030])
def test_rows_wider_than_one_pass_of_columns(OW):
    """More than 1024 output columns: the kernel's second pass over the columns, with 16-byte stores
    (1028) and with the scalar tail (1030)."""
    check_pixels(2, 4, 6, 3, OW, "cuda")


def test_eval_resize_and_center_crop():
    check_eval("cuda")


def test_default_resize_arguments_change_nothing():
    check_defaults_change_nothing("cuda")


@pytest.mark.parametrize("B,H,W,OH,OW", MIX_CASES)
def test_mixing_composes_with_the_resize(B, H, W, OH, OW):
    check_mixing_composes(B, H, W, OH, OW, "cuda")


def test_resize_argument_errors():
    check_argument_errors("cuda")


# ------------------------------------------------------------------------------- window stream
def test_published_windows_are_rrc_params_eagerly_and_in_replays():
    """The windows a batch publishes are rrc_params(seed, counter, 1, B, ...) bitwise: eagerly, and in replays
    of a captured batch whose counter the graph advances itself and whose offset follows it (nbatches = 3)."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W, OH, OW = 4, 12, 9, 8, 12
    scale = (0.08, 1.0)
    ds = dataset(B, H, W, "cuda")
    ld = DeviceLoader(ds, B, seed=21, rrc_scale=scale, out_size=(OH, OW))
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(3)).cuda()
    lib = _lib()
    bound = pixel_bound(ds)

    def want(ctr):
        return lib.rrc_params(21, ctr, 1, B, scale, RATIO, H, W)[0]

    for ctr in range(4):
        assert int(ld._counter.item()) == ctr
        ld.batch(idx, 0, B)
        assert torch.equal(ld.last_crops[:, :4], want(ctr)), ctr
    assert torch.equal(ld.crop_schedule(0, 4, B), torch.stack([want(c) for c in range(4)]))
    buf = torch.empty(B, 3, OH, OW, device="cuda").contiguous(memory_format=torch.channels_last)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ld.batch(idx, 0, B, out=buf, nbatches=3)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        data, tgt = ld.batch(idx, 0, B, out=buf, nbatches=3)
    crops_g = ld.last_crops
    torch.cuda.synchronize()
    assert data.data_ptr() == buf.data_ptr()
    seen = []
    for _ in range(4):
        ctr = int(ld._counter.item())
        gr.replay()
        torch.cuda.synchronize()
        assert int(ld._counter.item()) == ctr + 1
        crops = crops_g.cpu()
        assert torch.equal(crops_g[:, :4], want(ctr)), ctr
        src = idx[(ctr % 3) * B :][:B].cpu()
        assert torch.equal(tgt.cpu(), ds.labels.cpu()[src]), ctr
        err = (data.cpu().double() - fp64_batch(ds, src, crops, OH, OW)).abs().max().item()
        print(f"replay at counter {ctr}: pixel error {err:.3e} bound {bound:.3e}")
        assert err <= bound, (ctr, err, bound)
        seen.append(tuple(map(tuple, crops[:, :4].tolist())))
    assert len(set(seen)) > 1


def test_flip_and_mix_streams_are_independent_of_the_crop():
    """With the resize on, the published flips are the flips of a plain pad = 0 loader at the same seed and
    counter (recovered from its batch), and the mix rows are those of a loader without the resize."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 8, 8, 8
    ds = dataset(B, H, W, "cuda")
    ds.pad = 0
    idx = torch.arange(len(ds), device="cuda")
    rrc = DeviceLoader(ds, B, seed=13, rrc_scale=(0.08, 1.0))
    plain = DeviceLoader(ds, B, seed=13)
    full = torch.tensor([[0, 0, H, W, 0]] * B)
    flips = set()
    for step in range(4):
        rrc.batch(idx, 0, B)
        X, _ = plain.batch(idx, 0, B)
        straight = fp64_batch(ds, torch.arange(B), full, H, W)  # the images as stored, normalised
        X = X.cpu().double()
        got = []
        for b in range(B):
            same = (X[b] - straight[b]).abs().max().item() < 1e-5
            mirrored = (X[b] - straight[b].flip(-1)).abs().max().item() < 1e-5
            assert same != mirrored, (step, b)
            got.append(int(mirrored))
        assert rrc.last_crops[:, 4].tolist() == got, step
        flips.update(got)
    assert flips == {0, 1}
    a = DeviceLoader(ds, B, seed=13, rrc_scale=(0.08, 1.0), **MIX)
    b = DeviceLoader(ds, B, seed=13, **MIX)
    assert torch.equal(a.mix_schedule(0, 32), b.mix_schedule(0, 32))
    for _ in range(3):
        _, ta = a.batch(idx, 0, B)
        _, tb = b.batch(idx, 0, B)
        assert torch.equal(ta.info, tb.info)


def _windows(H, W, scale):
    win = _lib().rrc_params(21, 0, 64, 64, scale, RATIO, H, W)
    assert win.shape == (64, 64, 4) and win.dtype == torch.int32
    return win.reshape(-1, 4).cpu()


def test_the_draw_follows_the_published_rule():
    """4096 windows (64 counters x 64 image slots, seed 21) per setting; the bounds are four standard deviations
    of the mean of 4096 uniform draws, and the rounding of h and w to integers."""
    n = 4096
    # every proposal fits: the area share is U(0.25, 0.5), log(w / h) is U(-ln 4/3, ln 4/3)
    win = _windows(64, 64, (0.25, 0.5)).double()
    top, left, h, w = win.unbind(1)
    assert_windows_in_bounds(win, 64, 64)
    share = h * w / 4096
    d_area = abs(share.mean().item() - 0.375)
    d_ratio = abs(torch.log(w / h).mean().item())
    print(f"area share mean off by {d_area:.4f} (bound {4 * 0.25 / math.sqrt(12 * n):.4f}), "
          f"mean log ratio {d_ratio:.4f} (bound {4 * 2 * math.log(4 / 3) / math.sqrt(12 * n):.4f})")
    assert d_area <= 4 * 0.25 / math.sqrt(12 * n)
    assert d_ratio <= 4 * 2 * math.log(4 / 3) / math.sqrt(12 * n)
    slack = (h + w + 1) / (2 * 4096)
    assert ((share >= 0.25 - slack) & (share <= 0.5 + slack)).all()
    rel = 1 / h + 1 / w
    assert ((w / h >= 3 / 4 * (1 - rel)) & (w / h <= 4 / 3 * (1 + rel))).all()
    assert (top == 0).any() and (top == 64 - h).any() and (left == 0).any() and (left == 64 - w).any()
    # every proposal is rejected: the central fallback, cut to the nearest allowed ratio
    assert (_windows(8, 40, (0.5, 1.0)) == torch.tensor([0, 14, 8, 11], dtype=torch.int32)).all()
    assert (_windows(40, 8, (0.5, 1.0)) == torch.tensor([14, 0, 11, 8], dtype=torch.int32)).all()
    # some proposals are rejected and drawn again
    win = _windows(64, 64, (0.08, 1.0))
    assert_windows_in_bounds(win, 64, 64)
    whole = ((win[:, 2] == 64) & (win[:, 3] == 64)).double().mean().item()
    print(f"whole-image windows at scale (0.08, 1): {whole:.4f}")
    assert whole <= 0.05


# ------------------------------------------------------------------------------- op checks
def test_augment_resize_argument_checks():
    lib = _lib()
    B = 2
    mean, std = [0.5, 0.5, 0.5], [0.25, 0.25, 0.25]
    imgs = torch.zeros(4, 8, 8, 3, dtype=torch.uint8, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")

    def call(images=imgs, scale=(0.5, 1.0), out=None, crops=None):
        crops = torch.empty(B, 5, dtype=torch.int32, device="cuda") if crops is None else crops
        return lib.augment_resize(images, None, 0, B, mean, std, 6, 6, True, scale, RATIO, 1.0, True, ctr, 0, out, 0,
                                  None, None, crops)

    assert call().shape == (B, 3, 6, 6)
    with pytest.raises(RuntimeError):
        call(images=torch.zeros(4, 8, 8, 4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError):
        call(crops=torch.empty(B, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        call(crops=torch.empty(B + 1, 5, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        call(out=torch.empty(B, 3, 6, 6))
    with pytest.raises(RuntimeError):
        call(scale=(0.0, 1.0))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- whole step
def test_one_training_step_at_a_cropped_size():
    """ResNet-18, eager: 40 x 40 stored images cropped and resized to 32 x 32, mixup, label smoothing."""
    import cs744_distributed_data_parallel_amd as cdp
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, synthetic_imagenet

    torch.manual_seed(0)
    ds = synthetic_imagenet(32, size=40, device="cuda")
    ld = DeviceLoader(ds, 8, seed=4, rrc_scale=(0.35, 1.0), out_size=32, mixup_alpha=0.2)
    model = cdp.get_model("resnet18").cuda()
    opt = cdp.SGD(model.parameters(), lr=0.01, momentum=0.9)
    crit = cdp.CrossEntropyLoss(label_smoothing=0.1)
    before = [p.detach().clone() for p in model.parameters()]
    seen = []
    model.register_forward_pre_hook(lambda m, args: seen.append(tuple(args[0].shape)))
    data, tgt = ld.batch(torch.arange(32, device="cuda"), 0, 8)
    opt.zero_grad()
    loss = crit(model(data), tgt)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert math.isfinite(loss.item())
    assert seen == [(8, 3, 32, 32)]
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
