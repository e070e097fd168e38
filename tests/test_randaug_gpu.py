"""RandAugment in the device loader on the GPU: randaug_kernel against the Python twin (bitwise), its
composition with the normalising launch, the mix and the erase, the published rows, capture and the CLI."""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

import _randaug_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- 6. pixels are bitwise
@pytest.mark.parametrize("name", U.names())
def test_each_op_alone_is_bitwise_the_twin(name):
    kinds, _ = U.check_pixels_bitwise(DEV, (name,), 1)
    assert kinds == {U.names().index(name)}


def test_three_ops_of_the_full_set_are_bitwise_the_twin():
    kinds, signs = U.check_pixels_bitwise(DEV, U.names(), 3)
    assert len(kinds) >= 10 and signs == {0, 1}, (kinds, signs)


# ---------------------------------------------------------------- 7. the float output
@pytest.mark.parametrize("case", [U.RESIZE_SHAPES[3], U.PLAIN_SHAPES[1]])
def test_float_output_is_the_normalising_kernel_on_the_staged_images(case):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, ImageDataset

    B, H, W = case[:3]
    ds = U.make_dataset(B, H, W, DEV)
    ld = U.loader(ds, B, tuple(case[3:]) or None, randaug_num_ops=2, randaug_magnitude=15.0, randaug_mstd=0.5)
    idx = torch.arange(len(ds), device=DEV)
    for step in range(U.STEPS):
        out, y = ld.batch(idx, 1, B)
        staged = ImageDataset(ld.last_randaug_images.clone(), y.clone(), ds.mean, ds.std, pad=0)
        ref, yr = DeviceLoader(staged, B, train=False).batch(torch.arange(B, device=DEV), 0, B)
        assert torch.equal(out, ref) and torch.equal(y, yr), step
        assert ld.last_randaug_images.data_ptr() in {t.data_ptr() for t in ld._randaug_bufs[(B,) + out.shape[2:]][:2]}


# ---------------------------------------------------------------- 8. Identity on the plain path
@pytest.mark.parametrize("B,H,W", U.PLAIN_SHAPES)
@pytest.mark.parametrize("num_ops", [1, 2])
def test_identity_on_the_plain_path_is_the_loader_without(B, H, W, num_ops):
    ds = U.make_dataset(B, H, W, DEV)
    a = U.loader(ds, B, randaug_num_ops=num_ops, randaug_ops=("Identity",), **U.MIX, **U.ERASE)
    b = U.loader(ds, B, **U.MIX, **U.ERASE)
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(DEV)
    modes = set()
    for step in range(12):
        off = 1 + (step % 2) * B
        xa, ta = a.batch(idx, off, B)
        xb, tb = b.batch(idx, off, B)
        assert torch.equal(xa, xb), step
        assert all(torch.equal(u, v) for u, v in zip(ta, tb)), step
        assert torch.equal(a.last_erase, b.last_erase)
        modes.add(int(ta.info[0]))
    assert len(modes) >= 2, modes


# ---------------------------------------------------------------- 9. composition
@pytest.mark.parametrize("B,H,W,OH,OW", [U.RESIZE_SHAPES[0], U.RESIZE_SHAPES[3]])
def test_mix_erase_and_resize_compose(B, H, W, OH, OW):
    ds = U.make_dataset(B, H, W, DEV)
    a = U.loader(ds, B, (OH, OW), randaug_num_ops=2, randaug_magnitude=15.0, randaug_mstd=0.5, **U.MIX, **U.ERASE)
    b = U.loader(ds, B, (OH, OW), **U.MIX, **U.ERASE)
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(DEV)
    unmixed = 0
    for step in range(12):
        off = 1 + (step % 2) * B
        xa, ta = a.batch(idx, off, B)
        xb, tb = b.batch(idx, off, B)
        assert torch.equal(a.last_crops, b.last_crops) and torch.equal(a.last_erase, b.last_erase), step
        assert torch.equal(ta.info, tb.info) and torch.equal(ta.lam, tb.lam), step
        assert torch.equal(ta.target, tb.target) and torch.equal(ta.target_b, tb.target_b), step
        assert torch.equal(ta.target_b, ta.target.flip(0))
        if int(ta.info[0]) == 0:
            unmixed += 1
            # outside its erase box an image is its normalised staged image: the plain evaluation launch's bits
            from cs744_distributed_data_parallel_amd.data import DeviceLoader, ImageDataset

            staged = ImageDataset(a.last_randaug_images.clone(), ta.target.clone(), ds.mean, ds.std, pad=0)
            ref, _ = DeviceLoader(staged, B, train=False).batch(torch.arange(B, device=DEV), 0, B)
            keep = torch.ones_like(ref, dtype=torch.bool)
            for i, (on, top, left, h, w) in enumerate(a.last_erase.tolist()):
                if on:
                    keep[i, :, top : top + h, left : left + w] = False
            assert torch.equal(xa[keep], ref[keep]), step
    assert unmixed >= 1


# ---------------------------------------------------------------- 10. published rows
def half_up(x):
    return math.floor(x + 0.5)


@pytest.mark.parametrize("mstd", [0.0, 2.0])
def test_published_rows(mstd):
    from cs744_distributed_data_parallel_amd import randaug as R

    B, H, W, OH, OW = 6, 12, 9, 20, 31
    mag, num_ops, n = 9.3, 3, 8
    ds = U.make_dataset(B, H, W, DEV)
    ld = U.loader(ds, B, (OH, OW), randaug_num_ops=num_ops, randaug_magnitude=mag, randaug_mstd=mstd)
    idx = torch.arange(len(ds), device=DEV)
    sched = ld.randaug_schedule(0, n, B).cpu()
    assert sched.shape == (n, B, num_ops, 8) and sched.dtype == torch.int32
    assert torch.equal(ld.randaug_schedule(3, 2, B).cpu(), sched[3:5])
    levels = set()
    for step in range(n):
        ld.batch(idx, 0, B)
        rows = ld.last_randaug.cpu()
        assert torch.equal(rows, sched[step]), step
        host = R.randaug_draw(U.SEED, step, B, num_ops, mag, mstd, range(14), OH, OW)
        assert torch.equal(rows[..., 0], host[..., 0]), step  # ops and signs: the same bits
        if mstd == 0.0:
            assert (rows[..., 1] == round(256 * mag)).all()
        else:
            assert ((rows[..., 1] - host[..., 1]).abs() <= 1).all(), step
        assert ((rows[..., 1] >= 0) & (rows[..., 1] <= 30 * 256)).all()
        for r in rows.reshape(-1, 8).tolist():
            op, neg, lq = r[0] & 255, r[0] >> 8, r[1]
            levels.add(lq)
            L, sg = lq / 256.0, (-1 if neg else 1)
            t = L / 30.0
            assert r == R.randaug_derive(op, neg, lq, OH, OW) or op == R.ROTATE, r
            if R.BRIGHTNESS <= op <= R.SHARPNESS:
                assert abs(r[2] - half_up(256 * (1 + sg * 0.9 * t))) <= 1 and r[3:] == [0] * 5, r
            elif op == R.POSTERIZE:
                bits = 8 - half_up(4 * t)
                assert abs(r[2] - ((0xFF << (8 - bits)) & 0xFF)) <= 1 and r[3] == bits, r
            elif op == R.SOLARIZE:
                assert abs(r[2] - (256 - half_up(256 * t))) <= 1, r
            elif op in (R.SHEAR_X, R.SHEAR_Y):
                want = [65536, 0, 0, 65536, 0, 0]
                want[1 if op == R.SHEAR_X else 2] = sg * 65536 * 0.3 * t
                assert all(abs(g - w) <= 1 for g, w in zip(r[2:], want)), r
            elif op in (R.TRANSLATE_X, R.TRANSLATE_Y):
                px = int(150 / 331 * (OW if op == R.TRANSLATE_X else OH) * t + 1e-9)
                want = [65536, 0, 0, 65536, 0, 0]
                want[4 if op == R.TRANSLATE_X else 5] = -sg * 131072 * px
                assert r[2:] == want, r
            elif op == R.ROTATE:
                th = sg * math.pi / 6 * t
                want = [65536 * math.cos(th), 65536 * math.sin(th), -65536 * math.sin(th), 65536 * math.cos(th), 0, 0]
                assert all(abs(g - w) <= 2 for g, w in zip(r[2:], want)) and r[3] == -r[4] and r[2] == r[5], r
            else:
                assert r[2:] == [0] * 6, r
    assert (len(levels) == 1) == (mstd == 0.0)


# ---------------------------------------------------------------- 11. distribution
def test_op_and_sign_distribution():
    ds = U.make_dataset(2, 8, 8, DEV)
    ld = U.loader(ds, 2, randaug_num_ops=2)
    rows = ld.randaug_schedule(0, 224, 32).cpu()
    assert rows.shape == (224, 32, 2, 8)
    U.check_distribution(rows)


# ---------------------------------------------------------------- 12. capture
@pytest.mark.parametrize("resize", [False, True])
def test_captured_batch_replays_the_eager_batches(resize):
    B, H, W = 4, 8, 8
    ds = U.make_dataset(B, H, W, DEV)  # 13 images: nbatches = 3
    kw = dict(randaug_num_ops=2, randaug_magnitude=15.0, randaug_mstd=0.5, **U.MIX, **U.ERASE)
    out_size = (10, 6) if resize else None
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(DEV)
    eager = U.loader(ds, B, out_size, **kw)
    want = []
    for step in range(5):
        x, t = eager.batch(idx, 1, B, nbatches=3)
        want.append((x.clone(), [v.clone() for v in t], eager.last_randaug.clone(), eager.last_randaug_images.clone()))
    ld = U.loader(ds, B, out_size, **kw)
    ld._external_advance = True  # an external counter: the test advances it between replays
    static = torch.empty(B, 3, *(out_size or (H, W)), device=DEV).contiguous(memory_format=torch.channels_last)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ld.batch(idx, 1, B, out=static, nbatches=3)  # warm-up at counter 0
    torch.cuda.current_stream().wait_stream(s)
    ld._counter.fill_(1)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        x, t = ld.batch(idx, 1, B, out=static, nbatches=3)
        rows, imgs = ld.last_randaug, ld.last_randaug_images
    prev = None
    for step in range(1, 5):
        ld._counter.fill_(step)
        g.replay()
        torch.cuda.synchronize()
        wx, wt, wrows, wimgs = want[step]
        assert torch.equal(x, wx) and all(torch.equal(u, v) for u, v in zip(t, wt)), step
        assert torch.equal(rows, wrows) and torch.equal(imgs, wimgs), step
        assert prev is None or not torch.equal(prev, x)
        prev = x.clone()


# ---------------------------------------------------------------- 13. the CLI
def test_train_cli_with_randaugment_on_the_gpu():
    """(21 iterations, so that the epoch reaches iteration 20 and its log lines; 2 would print none.)"""
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "cs744_distributed_data_parallel_amd.train", "--model", "resnet18",
                        "--synthetic-size", "84", "--stored-size", "40", "--crop-size", "32", "--batch-size", "4",
                        "--iters", "21", "--randaug", "2", "9", "--randaug-mstd", "0.5", "--rrc-scale", "0.25", "1"],
                       env=env, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-5000:]
    losses = re.findall(r"Training loss after 20 epochs is (?:tensor\()?([-0-9.eE+naif]+)", r.stdout)
    assert len(losses) == 1 and math.isfinite(float(losses[0])), r.stdout
    lines = [ln for ln in r.stderr.splitlines() if "randaug of image 0 in iter" in ln]
    op = r"(?:%s)\(-?[0-9.]+\)" % "|".join(U.names())
    assert len(lines) == 1 and re.fullmatch(r"\[cdp\] rank 0: randaug of image 0 in iter 20 is %s %s" % (op, op),
                                            lines[0]), r.stderr[-3000:]
    assert "randaug" not in r.stdout
