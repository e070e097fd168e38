"""Shared checks of RandomErasing in DeviceLoader, run on the GPU kernels (test_erase_gpu.py) and on the
CPU path (test_erase_cpu.py) with the same assertions."""
import functools
import math

import numpy as np
import pytest
import torch

from _mix_util import MIX, STEPS as MIX_STEPS, dataset

# (B, H, W): an even batch; an odd one (the middle image pairs with itself); non-square; more than one workgroup
PLAIN_CASES = [(4, 8, 8), (5, 8, 8), (3, 6, 10), (2, 40, 40)]
# (B, H, W, OH, OW): non-square both ways; an odd width (the scalar-store tail); the vector path, several passes
RESIZE_CASES = [(3, 6, 10, 10, 6), (2, 12, 9, 5, 7), (2, 5, 7, 40, 40)]
# the default share of the area, and one at which boxes span quads and rows
SCALES = [(0.02, 0.33), (0.1, 0.5)]
RATIO = (0.3, 3.3)
PROB = 0.6
STEPS = 12  # consecutive counters: at least 24 images per case, P(all erased or none) < 0.6^24 = 5e-6 a priori
SEED = 11
# const with a scalar and with a 3-vector (neither is exact in fp32), rand, pixel
FILLS = [dict(erase_mode="const", erase_value=0.3), dict(erase_mode="const", erase_value=(0.1, -1.7, 2.3)),
         dict(erase_mode="rand"), dict(erase_mode="pixel")]


def resize_kw(OH, OW):
    return dict(rrc_scale=(0.25, 1.0), out_size=(OH, OW))


def assert_rows_valid(rows, H, W):
    """Boxes lie inside the image with 1 <= h < H and 1 <= w < W; rows with on = 0 are all zero."""
    assert rows.shape[-1] == 5 and rows.dtype == torch.int32
    r = rows.reshape(-1, 5).cpu().long()
    on, top, left, h, w = r.unbind(1)
    assert ((on == 0) | (on == 1)).all()
    assert (r[on == 0] == 0).all(), r[on == 0]
    e = on == 1
    assert ((top[e] >= 0) & (left[e] >= 0) & (h[e] >= 1) & (w[e] >= 1) & (h[e] < H) & (w[e] < W)
            & (top[e] + h[e] <= H) & (left[e] + w[e] <= W)).all(), r[e]


def expected_fill(kw, noise, b, box):
    """The values of image b's box [3, h, w] under the fill kw; noise: loader.erase_noise of the step."""
    top, left, h, w = box
    if kw["erase_mode"] == "const":
        v = kw["erase_value"]
        v = [v] * 3 if isinstance(v, float) else list(v)
        return torch.tensor(v, dtype=torch.float32, device=noise.device).view(3, 1, 1).expand(3, h, w)
    if kw["erase_mode"] == "rand":
        return noise[b, :, :1, :1].expand(3, h, w)
    return noise[b, :, top : top + h, left : left + w]


def check_erased_pixels(case, scale, device, seed=SEED):
    """Checks 1 and 2: every fill against the plain batch X of a twin loader at the same seed and counter.
    Outside its published box an image is X bitwise; inside it is the fill, bitwise; an image with on = 0 is X
    bitwise; the published rows are erase_schedule's; crops (windows and flips) and labels are the twin's."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = case[:3]
    OH, OW = case[3:] if len(case) == 5 else (H, W)
    kw = resize_kw(OH, OW) if len(case) == 5 else {}
    ds = dataset(B, H, W, device)
    plain = DeviceLoader(ds, B, seed=seed, **kw)
    erased = [DeviceLoader(ds, B, seed=seed, erase_prob=PROB, erase_scale=scale, erase_ratio=RATIO, **f, **kw)
              for f in FILLS]
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(device)
    n_on = n_off = 0
    boxes = set()
    for step in range(STEPS):
        off = 1 + (step % 2) * B
        ctr = int(plain._counter.item())
        X, y = plain.batch(idx, off, B)
        assert plain.last_erase is None and not plain.erasing
        rows0 = None
        for f, ld in zip(FILLS, erased):
            assert ld.erasing and int(ld._counter.item()) == ctr
            out, t = ld.batch(idx, off, B)
            assert out.shape == X.shape == (B, 3, OH, OW) and out.dtype == torch.float32
            assert out.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(t, y), (step, f)
            if kw:
                assert torch.equal(ld.last_crops, plain.last_crops), (step, f)
            rows = ld.last_erase
            assert rows.shape == (B, 5) and rows.dtype == torch.int32 and rows.device == out.device
            assert_rows_valid(rows, OH, OW)
            assert torch.equal(rows, ld.erase_schedule(ctr, 1, B)[0]), (step, f)
            # the box does not depend on the fill
            rows0 = rows if rows0 is None else rows0
            assert torch.equal(rows, rows0), (step, f)
            noise = ld.erase_noise(ctr, B)
            assert noise.shape == (B, 3, OH, OW) and noise.dtype == torch.float32
            for b, (on, top, left, h, w) in enumerate(rows.tolist()):
                if not on:
                    assert torch.equal(out[b], X[b]), (step, f, b)
                    continue
                inside = torch.zeros(3, OH, OW, dtype=torch.bool, device=out.device)
                inside[:, top : top + h, left : left + w] = True
                assert torch.equal(out[b][~inside], X[b][~inside]), (step, f, b)
                want = expected_fill(f, noise, b, (top, left, h, w))
                got = out[b, :, top : top + h, left : left + w]
                assert torch.equal(got, want), (step, f, b, (got - want).abs().max().item())
        for on, top, left, h, w in rows0.tolist():
            n_on += on
            n_off += 1 - on
            if on:
                boxes.add((top, left, h, w))
    print(f"{device} {case} scale {scale}: {n_on} erased, {n_off} plain, {len(boxes)} distinct boxes")
    assert n_on > 0 and n_off > 0 and len(boxes) > 1


# ------------------------------------------------------------------------------- check 3: the noise
def _hash(x):
    """splitmix64, the counter-based hash of the augmentation, in Python integers."""
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


def _uniform(r):
    return ((r >> 41) + 0.5) / 8388608.0  # 23 hash bits + 1/2: exact in fp32 and in fp64


TWO_PI_F32 = float(np.float32(6.2831853))  # the constant of the documented function, as fp32 holds it


def documented_noise(seed, ctr, B, H, W):
    """erase_noise as the header documents it, in fp64: element e = (y W + x) 3 + c of image slot b is
    sqrt(-2 ln u1) cos(K u2) with u1, u2 the uniforms of hash(key + 2 e), hash(key + 2 e + 1), key the
    hash of (seed, counter, b) under the noise tag, K = float32(6.2831853). Returns [B, 3, H, W]."""
    m = (1 << 64) - 1
    out = torch.empty(B, H, W, 3, dtype=torch.float64)
    flat = out.view(B, -1)
    for b in range(B):
        key = _hash(_hash(seed ^ 0x65726173652D6E7A) ^ _hash((_hash((ctr + 0x6E6F6973652D3031) & m) + b) & m))
        for e in range(H * W * 3):
            u1, u2 = _uniform(_hash((key + 2 * e) & m)), _uniform(_hash((key + 2 * e + 1) & m))
            flat[b, e] = math.sqrt(-2.0 * math.log(u1)) * math.cos(TWO_PI_F32 * u2)
    return out.permute(0, 3, 1, 2)


def noise_bound():
    """fp32 evaluation of sqrtf(-2 logf(u1)) * cosf(K u2) against fp64, absolute, with eps = 2^-24 (half an
    ulp, relative). u1 and u2 are exact in both. The radius r = sqrt(-2 ln u1) is at most
    R = sqrt(-2 ln 2^-24) = 5.77 (u1 >= 2^-24), and |cos| <= 1. Named roundings:

    * the product K u2 < 8: half an ulp of [4, 8) is 2^-22 = 4 eps absolute in the angle, and
      |d cos / d angle| <= 1, so 4 eps in the cosine;
    * cosf: at most 2 ulp of a value <= 1, i.e. 4 eps absolute (the HIP math library documents 1 ulp for
      cosf; 2 leaves room for its argument reduction);
    * logf: at most 2 ulp (documented: 1 ulp), 4 eps relative in -2 ln u1 (the product by -2 is exact), which
      the square root halves: 2 eps relative in r;
    * sqrtf: correctly rounded, 1 eps relative in r;
    * the final product: 1 eps relative.

    Relative terms apply to a result of at most R, the cosine's absolute terms are scaled by r <= R:
    (4 + 4 + 2 + 1 + 1) eps R = 12 * 2^-24 * 5.77 = 4.1e-6."""
    return 12 * 2.0 ** -24 * math.sqrt(-2.0 * math.log(2.0 ** -24))


def noise_loader(B, H, W, device, seed=SEED):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    return DeviceLoader(dataset(B, H, W, device), B, seed=seed, erase_prob=PROB, erase_mode="pixel")


def check_noise_moments(device, seed=SEED, ctr=3):
    """Check 3, second half: at (2, 64, 64) the sample mean and variance lie within 5 standard errors of 0, 1."""
    z = noise_loader(2, 64, 64, device, seed).erase_noise(ctr, 2).double()
    assert z.shape == (2, 3, 64, 64)
    n = z.numel()
    mean, var = z.mean().item(), z.var(unbiased=False).item()
    print(f"{device}: n {n} mean {mean:.5f} (bound {5 / math.sqrt(n):.5f}) var {var:.5f} "
          f"(|var - 1| bound {5 * math.sqrt(2 / n):.5f})")
    assert abs(mean) <= 5 / math.sqrt(n)
    assert abs(var - 1) <= 5 * math.sqrt(2 / n)
    # the images' fields differ, and so do the channels and the steps
    assert not torch.equal(z[0], z[1]) and not torch.equal(z[0, 0], z[0, 1])
    assert not torch.equal(z, noise_loader(2, 64, 64, device, seed).erase_noise(ctr + 1, 2).double())


# ------------------------------------------------------------------------------- check 4: the draw rule
@functools.lru_cache(maxsize=None)
def python_rule_reference(H=32, W=32, n=100_000):
    """The Python rule of _cpu_erase over n draws with prob = 1 at the default scale and ratio: (every draw
    got a box, mean and standard deviation of h w / (H W)). A first proposal is rejected now and then (about
    0.6 % at 32 x 32: h or w would reach 32), ten in a row never, so the erased fraction is prob itself."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    g = torch.Generator().manual_seed(2024)
    rows = torch.tensor([DeviceLoader._erase_get_params(H, W, 1.0, SCALES[0], RATIO, g) for _ in range(n)])
    share = (rows[:, 3] * rows[:, 4]).double() / (H * W)
    return bool((rows[:, 0] == 1).all()), share.mean().item(), share.std().item()


def check_draw_statistics(device, seed=SEED):
    """erase_schedule over 400 counters at B = 8 (3200 draws) on a 32 x 32 image, default scale and ratio."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    H = W = 32
    n = 3200
    all_on, ref_mean, ref_sd = python_rule_reference(H, W)
    assert all_on  # no draw of the Python rule runs out of proposals: P(erased) = prob
    ld = DeviceLoader(dataset(8, H, W, device), 8, seed=seed, erase_prob=PROB)
    rows = ld.erase_schedule(0, 400, 8)
    assert rows.shape == (400, 8, 5)
    assert_rows_valid(rows, H, W)
    r = rows.reshape(-1, 5).cpu().double()
    on = r[:, 0] == 1
    k = int(on.sum())
    sd = math.sqrt(n * PROB * (1 - PROB))
    print(f"{device}: erased {k} of {n}, expected {PROB * n:.0f} +- {5 * sd:.1f}")
    assert abs(k - PROB * n) <= 5 * sd
    h, w = r[on, 3], r[on, 4]
    share = h * w / (H * W)
    se = ref_sd * math.sqrt(1 / k + 1 / 100_000)
    print(f"{device}: mean area share {share.mean().item():.5f}, Python rule {ref_mean:.5f} +- {5 * se:.5f}")
    assert abs(share.mean().item() - ref_mean) <= 5 * se
    tall = (h > w).double().mean().item()
    print(f"{device}: h > w in {tall:.4f} of the boxes, expected 0.5 +- {5 * math.sqrt(0.25 / k):.4f} "
          f"(h == w in {(h == w).double().mean().item():.4f})")
    assert abs(tall - 0.5) <= 5 * math.sqrt(0.25 / k)
    # boxes reach every edge
    assert (r[on, 1] == 0).any() and (r[on, 2] == 0).any() and (r[on, 1] + h == H).any() and (r[on, 2] + w == W).any()


# ------------------------------------------------------------------------------- check 5: composition with mix
def check_mixing_composes(case, device, fill, seed=SEED):
    """check_mixed_batches' assertions with erasing on in both twin loaders: the mix acts on the erased batch
    X_e, whose partner X_e.flip(0) shows every image's own box and noise."""
    from cs744_distributed_data_parallel_amd.data import DeviceLoader, MixTarget

    B, H, W = case[:3]
    OH, OW = case[3:] if len(case) == 5 else (H, W)
    kw = dict(resize_kw(OH, OW) if len(case) == 5 else {}, erase_prob=PROB, erase_scale=SCALES[1], **fill)
    ds = dataset(B, H, W, device)
    mixed = DeviceLoader(ds, B, seed=seed, **MIX, **kw)
    plain = DeviceLoader(ds, B, seed=seed, **kw)
    unerased = DeviceLoader(ds, B, seed=seed, **MIX, **{k: v for k, v in kw.items() if not k.startswith("erase")})
    idx = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1)).to(device)
    seen, n_on = set(), 0
    for step in range(MIX_STEPS):
        off = 1 + (step % 2) * B
        out, tgt = mixed.batch(idx, off, B)
        X, y = plain.batch(idx, off, B)
        _, tgt_u = unerased.batch(idx, off, B)
        assert isinstance(tgt, MixTarget) and torch.is_tensor(y)
        assert out.shape == X.shape == (B, 3, OH, OW) and out.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(mixed.last_erase, plain.last_erase), step
        n_on += int(plain.last_erase[:, 0].sum())
        # labels, MixTarget and the mix row are what they are without erasing
        assert torch.equal(tgt.info, tgt_u.info), step
        assert torch.equal(tgt.target, y) and torch.equal(tgt.target_b, y.flip(0)), step
        assert torch.equal(tgt.target, tgt_u.target) and torch.equal(tgt.target_b, tgt_u.target_b), step
        if len(case) == 5:
            assert torch.equal(mixed.last_crops, plain.last_crops), step
            assert torch.equal(mixed.last_crops, unerased.last_crops), step
        info = tgt.info.cpu()
        mode, lam = int(info[0]), info[1].item()
        y0, y1, x0, x1 = (int(v) for v in info[3:7])
        assert tgt.lam.item() == lam
        seen.add(mode)
        Xp = X.flip(0)
        if mode == 0:
            assert torch.equal(out, X) and lam == 1.0, step
        elif mode == 2:
            box = torch.zeros(1, 1, OH, OW, dtype=torch.bool, device=X.device)
            box[..., y0:y1, x0:x1] = True
            assert torch.equal(out, torch.where(box, Xp, X)), step
        else:
            assert mode == 1
            ref = lam * X.double() + (1.0 - lam) * Xp.double()
            # two products, one sum and the rounding of 1 - lam, each at most half an ulp
            bound = 4 * 2.0 ** -24 * X.abs().max().item()
            err = (out.double() - ref).abs().max().item()
            print(f"step {step}: mixup lam {lam:.6f} err {err:.3e} bound {bound:.3e}")
            assert err <= bound, (step, err, bound)
    assert seen == {0, 1, 2}, seen
    assert n_on > 0


# ------------------------------------------------------------------------------- check 6: defaults
def check_defaults_change_nothing(device):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    B, H, W = 4, 8, 8
    ds = dataset(B, H, W, device)
    idx = torch.arange(len(ds), device=device)
    for kw in ({}, dict(rrc_scale=(0.25, 1.0), out_size=(6, 10)), MIX):
        a = DeviceLoader(ds, B, seed=5, erase_prob=0.0, erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3),
                         erase_mode="pixel", erase_value=(1.0, 2.0, 3.0), **kw)
        b = DeviceLoader(ds, B, seed=5, **kw)
        for _ in range(3):
            xa, ta = a.batch(idx, 0, B)
            xb, tb = b.batch(idx, 0, B)
            assert torch.equal(xa, xb)
            assert torch.equal(ta.info, tb.info) if kw is MIX else torch.equal(ta, tb)
        assert a.last_erase is None and not a.erasing
        with pytest.raises(ValueError):
            a.erase_schedule(0, 1, B)
        with pytest.raises(ValueError):
            a.erase_noise(0, B)
    # an evaluation loader never erases
    e = DeviceLoader(ds, B, train=False, erase_prob=1.0, erase_mode="pixel")
    p = DeviceLoader(ds, B, train=False)
    assert not e.erasing
    assert torch.equal(e.batch(idx, 0, B)[0], p.batch(idx, 0, B)[0]) and e.last_erase is None
    # erase_prob = 1 erases every image; the default fill is 0
    full = DeviceLoader(ds, B, seed=5, erase_prob=1.0)
    x, _ = full.batch(idx, 0, B)
    rows = full.last_erase.tolist()
    assert all(r[0] == 1 for r in rows), rows
    for b, (_, top, left, h, w) in enumerate(rows):
        assert (x[b, :, top : top + h, left : left + w] == 0).all()


def check_argument_errors(device):
    from cs744_distributed_data_parallel_amd.data import DeviceLoader

    ds = dataset(4, 8, 8, device)
    for kw in (dict(erase_prob=-0.1), dict(erase_prob=1.5), dict(erase_scale=(0.5, 0.2)), dict(erase_scale=(0, 0.3)),
               dict(erase_scale=(0.1, 1.5)), dict(erase_ratio=(2, 1)), dict(erase_ratio=(0, 1)),
               dict(erase_mode="noise"), dict(erase_value=(1.0, 2.0)), dict(erase_value=float("nan"))):
        with pytest.raises(ValueError):
            DeviceLoader(ds, 4, **kw)
