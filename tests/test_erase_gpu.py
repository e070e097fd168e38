"""Fused RandomErasing: the ERASE instantiations of augment_kernel and augment_resize_kernel against the
plain batch of a twin loader (every fill, bitwise), the device-side box stream (erase_draw / erase_params)
against the published rule, the fill noise against its documented function in fp64, the composition with
mixup / CutMix, the op's argument checks and a captured batch whose boxes change at every replay."""
import pytest
import torch

from _erase_util import (FILLS, PLAIN_CASES, PROB, RESIZE_CASES, SCALES, SEED, check_argument_errors,
                         check_defaults_change_nothing, check_draw_statistics, check_erased_pixels,
                         check_mixing_composes, check_noise_moments, documented_noise, noise_bound, noise_loader,
                         resize_kw)
from _mix_util import MIX, dataset

pytestmark = pytest.mark.gpu


def _lib():
    import cs744_distributed_data_parallel_amd as cdp

    return cdp._native.lib()


# ------------------------------------------------------------------------------- shared checks
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("case", PLAIN_CASES + RESIZE_CASES)
def test_erased_pixels_follow_the_plain_batch(case, scale):
    check_erased_pixels(case, scale, "cuda")


def test_noise_moments():
    check_noise_moments("cuda")


def test_draw_statistics():
    check_draw_statistics("cuda")


@pytest.mark.parametrize("fill", [FILLS[3], dict()], ids=["pixel", "const0"])
@pytest.mark.parametrize("case", [(4, 8, 8), (5, 8, 8), (2, 40, 40), (5, 6, 10, 8, 12), (2, 12, 12, 40, 40)])
def test_mixing_composes_with_erasing(case, fill):
    check_mixing_composes(case, "cuda", fill)


def test_default_erase_arguments_change_nothing():
    check_defaults_change_nothing("cuda")


def test_erase_argument_errors():
    check_argument_errors("cuda")


# ------------------------------------------------------------------------------- the noise
def test_noise_is_the_documented_function():
    """The field of (2, 16, 16) against the header's formula evaluated in Python integers and fp64, within
    noise_bound() (derived there); the loader's erase_noise is the op's."""
    B, H, W, ctr = 2, 16, 16, 5
    ld = noise_loader(B, H, W, "cuda")
    z = ld.erase_noise(ctr, B)
    assert z.shape == (B, 3, H, W) and z.dtype == torch.float32 and z.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(z, _lib().erase_noise(SEED, ctr, B, H, W))
    err = (z.cpu().double() - documented_noise(SEED, ctr, B, H, W)).abs().max().item()
    print(f"noise: worst error against fp64 {err:.3e} bound {noise_bound():.3e}")
    assert err <= noise_bound()
    # image slot b's field does not depend on the batch around it
    assert torch.equal(ld.erase_noise(ctr, 1), z[:1])


# ------------------------------------------------------------------------------- the box stream
def test_erase_rows_do_not_depend_on_the_other_streams():
    """The rows of a loader with the resize and the mix on are those of erase_params at the output size, and
    the windows, flips and mix rows of that loader are those of one without erasing."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W, OH, OW = 8, 8, 8, 6, 10
    ds = dataset(B, H, W, "cuda")
    idx = torch.arange(len(ds), device="cuda")
    kw = dict(seed=13, **resize_kw(OH, OW), **MIX)
    a = DeviceLoader(ds, B, erase_prob=PROB, erase_mode="rand", **kw)
    b = DeviceLoader(ds, B, **kw)
    want = _lib().erase_params(13, 0, 4, B, PROB, (0.02, 0.33), (0.3, 3.3), OH, OW)
    assert want.shape == (4, B, 5) and want.dtype == torch.int32
    assert torch.equal(a.erase_schedule(0, 4, B), want)
    assert torch.equal(a.mix_schedule(0, 32), b.mix_schedule(0, 32))
    assert torch.equal(a.crop_schedule(0, 8, B), b.crop_schedule(0, 8, B))
    for step in range(4):
        _, ta = a.batch(idx, 0, B)
        _, tb = b.batch(idx, 0, B)
        assert torch.equal(a.last_erase, want[step]), step
        assert torch.equal(a.last_crops, b.last_crops) and torch.equal(ta.info, tb.info), step
    # an image as tall as 1 pixel, or as wide, is never erased (h < H, w < W)
    assert (_lib().erase_params(1, 0, 8, 8, 1.0, (0.02, 0.33), (0.3, 3.3), 1, 32) == 0).all()
    assert (_lib().erase_params(1, 0, 8, 8, 1.0, (0.02, 0.33), (0.3, 3.3), 32, 1) == 0).all()
    # every proposal is rejected (ratio 100 at half the area: h would be 10 W): not erased, all zeros
    assert (_lib().erase_params(1, 0, 8, 8, 1.0, (0.5, 0.5), (100.0, 100.0), 16, 16) == 0).all()


def test_native_erase_argument_checks():
    lib = _lib()
    B = 2
    mean, std = [0.5, 0.5, 0.5], [0.25, 0.25, 0.25]
    imgs = torch.zeros(4, 8, 8, 3, dtype=torch.uint8, device="cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = torch.full((B, 5), -1, dtype=torch.int32, device="cuda")

    def call(images=imgs, **kw):
        return lib.augment(images, None, 0, B, mean, std, 0, True, ctr, 0, **kw)

    assert call(erase_prob=1.0, erase=rows).shape == (B, 3, 8, 8)
    assert (rows[:, 0] == 1).all()
    for bad in (dict(erase_prob=0.5), dict(erase_prob=0.5, erase=rows[:1]), dict(erase_prob=0.5, erase=rows.long()),
                dict(erase_prob=0.5, erase=rows.cpu()), dict(erase_prob=1.5, erase=rows),
                dict(erase_prob=0.5, erase=rows, erase_scale=(0.0, 0.3)),
                dict(erase_prob=0.5, erase=rows, erase_ratio=(2.0, 1.0)),
                dict(erase_prob=0.5, erase=rows, erase_mode="noise"),
                dict(erase_prob=0.5, erase=rows, erase_value=[1.0, 2.0])):
        with pytest.raises(RuntimeError):
            call(**bad)
    with pytest.raises(RuntimeError):  # erasing is for 3-channel images
        call(images=torch.zeros(4, 8, 8, 1, dtype=torch.uint8, device="cuda"), erase_prob=0.5, erase=rows)
    crops = torch.empty(B, 5, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        lib.augment_resize(imgs, None, 0, B, mean, std, 6, 6, True, (0.5, 1.0), (0.75, 1.33), 1.0, True, ctr, 0, None,
                           0, None, None, crops, erase_prob=0.5)
    with pytest.raises(RuntimeError):
        lib.erase_params(0, 0, 1, B, 2.0, (0.02, 0.33), (0.3, 3.3), 8, 8)
    with pytest.raises(RuntimeError):
        lib.erase_noise(0, 0, B, 0, 8)
    assert lib.erase_params(0, 0, 0, B, 0.5, (0.02, 0.33), (0.3, 3.3), 8, 8).shape == (0, B, 5)
    assert lib.erase_noise(0, 0, 0, 8, 8).shape == (0, 3, 8, 8)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------- hipGraph
@pytest.mark.parametrize("case", [(4, 8, 8), (3, 6, 10, 10, 6)])
def test_captured_batch_erases_anew_at_every_replay(case):
    """One captured batch(..., nbatches=2) with erasing and mixing on, replayed 4 times: each replay's rows are
    the schedule's at its counter, at least two replays differ, and each replayed batch is the eager batch of a
    twin loader at that counter, bitwise."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = case[:3]
    OH, OW = case[3:] if len(case) == 5 else (H, W)
    kw = dict(resize_kw(OH, OW) if len(case) == 5 else {}, seed=21, erase_prob=PROB, erase_scale=SCALES[1],
              erase_mode="pixel", **MIX)
    ds = dataset(B, H, W, "cuda")
    ld, twin = DeviceLoader(ds, B, **kw), DeviceLoader(ds, B, **kw)
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(3)).cuda()
    buf = torch.empty(B, 3, OH, OW, device="cuda").contiguous(memory_format=torch.channels_last)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ld.batch(idx, 0, B, out=buf, nbatches=2)
    torch.cuda.current_stream().wait_stream(s)
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        data, tgt = ld.batch(idx, 0, B, out=buf, nbatches=2)
    rows_g = ld.last_erase
    torch.cuda.synchronize()
    seen = []
    for _ in range(4):
        ctr = int(ld._counter.item())
        gr.replay()
        torch.cuda.synchronize()
        assert int(ld._counter.item()) == ctr + 1
        assert torch.equal(rows_g, ld.erase_schedule(ctr, 1, B)[0]), ctr
        twin._counter.fill_(ctr)
        X, t = twin.batch(idx, 0, B, nbatches=2)
        assert torch.equal(twin.last_erase, rows_g), ctr
        assert torch.equal(data, X), ctr
        assert torch.equal(tgt.info, t.info) and torch.equal(tgt.target, t.target), ctr
        assert torch.equal(tgt.target_b, t.target_b), ctr
        seen.append(tuple(map(tuple, rows_g.tolist())))
    assert len(set(seen)) > 1, seen
