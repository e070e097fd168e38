"""RandAugment (Cubuk et al.) on uint8 images: the pure-Python twin of ``csrc/kernels/randaug.{h,hip}``.

Every operation of every image is one published row of 8 integers ``{op | sign << 8, level_q, p0 .. p5}``
(``level_q = round(256 L)`` for the level ``L`` in [0, 30]); :func:`randaug_reference` applies rows to uint8
images with numpy int64 arithmetic only, and agrees with the device kernel bitwise. :func:`randaug_draw`
evaluates the device's draw on the host (op and sign exactly, through the same hash; the level's Box-Muller
in Python floats), :func:`randaug_derive` the integers of a row from its level, :func:`stage_resize` and
:func:`stage_plain` the uint8 staging that precedes the operations.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .ops.functional import _mix_hash

RANDAUG_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color",
               "Contrast", "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize")
(IDENTITY, SHEAR_X, SHEAR_Y, TRANSLATE_X, TRANSLATE_Y, ROTATE, BRIGHTNESS, COLOR, CONTRAST, SHARPNESS, POSTERIZE,
 SOLARIZE, AUTO_CONTRAST, EQUALIZE) = range(14)
ROW = 8
NEG_BIT = 256
MAX_OPS = 8
MAX_NAMES = 32


def _round_div(num: int, den: int) -> int:
    """round(num / den) to nearest, halves up (num >= 0, den > 0)."""
    return (2 * num + den) // (2 * den)


def randaug_derive(op: int, neg: int, level_q: int, H: int, W: int):
    """The row of op kind ``op`` with sign ``neg`` at ``level_q`` on an ``H x W`` image (a list of 8 ints). All
    integer arithmetic, except Rotate's ``cos`` / ``sin`` (Python floats: within 2 units of the device's fp32)."""
    r = [op | (NEG_BIT if neg else 0), level_q, 0, 0, 0, 0, 0, 0]
    sg = -1 if neg else 1
    if SHEAR_X <= op <= ROTATE:
        a, b, c, d, tx, ty = 65536, 0, 0, 65536, 0, 0
        if op == SHEAR_X:
            b = sg * _round_div(256 * level_q, 100)
        elif op == SHEAR_Y:
            c = sg * _round_div(256 * level_q, 100)
        elif op == TRANSLATE_X:
            tx = -sg * 131072 * (150 * W * level_q // (331 * 7680))
        elif op == TRANSLATE_Y:
            ty = -sg * 131072 * (150 * H * level_q // (331 * 7680))
        else:
            th = level_q / 7680.0 * math.pi / 6.0
            a = d = int(round(65536 * math.cos(th)))
            b = sg * int(round(65536 * math.sin(th)))
            c = -b
        r[2:8] = [a, b, c, d, tx, ty]
    elif BRIGHTNESS <= op <= SHARPNESS:
        r[2] = 256 + sg * _round_div(3 * level_q, 100)
    elif op == POSTERIZE:
        bits = 8 - _round_div(level_q, 1920)
        r[2], r[3] = (0xFF << (8 - bits)) & 0xFF, bits
    elif op == SOLARIZE:
        r[2] = 256 - _round_div(level_q, 30)
    return r


def _u64(v):
    return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def _uniform(r):
    """MixRng::uniform's map of a hash to (0, 1), in float32."""
    return (np.float32(int(r) >> 41) + np.float32(0.5)) * np.float32(1.0 / 8388608.0)


def randaug_draw(seed: int, counter: int, B: int, num_ops: int, magnitude: float, mstd: float, ops, H: int,
                 W: int) -> torch.Tensor:
    """The rows of the ``B`` images of the batch at step counter ``counter`` (int32 ``[B, num_ops, 8]``), on the
    host. ``ops``: the op kinds to draw from. Op and sign are the device's bits; the level is computed in Python
    floats, so ``level_q`` may differ from the device's in its last unit when ``mstd`` > 0."""
    ops = [int(o) for o in ops]
    rows = np.zeros((B, num_ops, ROW), dtype=np.int32)
    with np.errstate(over="ignore"):
        skey = _mix_hash(_u64(seed) ^ np.uint64(0x72616E646175672D))
        ckey = _mix_hash(_u64(counter) + np.uint64(0x6F70732D72612D31))
        for b in range(B):
            key = _mix_hash(skey ^ _mix_hash(ckey + np.uint64(b)))
            for k in range(num_ops):
                base = key + np.uint64(4 * k)
                r0, r1 = int(_mix_hash(base)), int(_mix_hash(base + np.uint64(1)))
                op = ops[((r0 >> 32) * len(ops)) >> 32]
                neg = r1 >> 63
                L = float(magnitude)
                if mstd > 0.0:
                    u1 = float(_uniform(_mix_hash(base + np.uint64(2))))
                    u2 = float(_uniform(_mix_hash(base + np.uint64(3))))
                    L += float(mstd) * math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)
                L = min(max(L, 0.0), 30.0)
                rows[b, k] = randaug_derive(op, neg, int(math.floor(256.0 * L + 0.5)), H, W)
    return torch.from_numpy(rows)


def aug_crop_flip(seed: int, counter: int, B: int, pad: int, flip: bool):
    """The pad-shift crop offsets and flip bits ``(oy, ox, fl)`` of the augment kernels' own hash for the ``B``
    images of the batch at step counter ``counter`` (three int lists)."""
    oy, ox, fl = [], [], []
    span = 2 * pad + 1
    with np.errstate(over="ignore"):
        for b in range(B):
            r = int(_mix_hash(_u64(seed) ^ _mix_hash(_u64(counter) * np.uint64(0x100000001B3) + np.uint64(b))))
            oy.append(r % span - pad if pad else 0)
            ox.append((r >> 16) % span - pad if pad else 0)
            fl.append(int(bool(flip) and (r >> 40) & 1))
    return oy, ox, fl


def stage_plain(images: torch.Tensor, oy, ox, fl) -> torch.Tensor:
    """uint8 ``[B, H, W, 3]``: image ``b`` shifted by ``(oy[b], ox[b])`` with zero padding, then flipped when
    ``fl[b]`` (RandomCrop(pad) + RandomHorizontalFlip in uint8 space)."""
    src = images.cpu().numpy()
    B, H, W, _ = src.shape
    out = np.zeros_like(src)
    for b in range(B):
        y0, y1 = max(0, -oy[b]), min(H, H - oy[b])
        x0, x1 = max(0, -ox[b]), min(W, W - ox[b])
        if y0 < y1 and x0 < x1:
            out[b, y0:y1, x0:x1] = src[b, y0 + oy[b] : y1 + oy[b], x0 + ox[b] : x1 + ox[b]]
        if fl[b]:
            out[b] = out[b, :, ::-1]
    return torch.from_numpy(out)


def _taps(n_in: int, n_out: int):
    """Per output index of an axis: the two neighbours and the weight numerator of the second (over 2 n_out)."""
    o = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * o + 1) * n_in - n_out, 0)
    den = 2 * n_out
    i0 = num // den
    return np.minimum(i0, n_in - 1), np.minimum(i0 + 1, n_in - 1), num - i0 * den, den


def stage_resize(images: torch.Tensor, crops, OH: int, OW: int) -> torch.Tensor:
    """uint8 ``[B, OH, OW, 3]``: the window ``{top, left, h, w}`` of image ``b`` resampled bilinearly
    (``align_corners=False``, no antialias) to ``OH x OW``, exactly in integers -- the tap weights are the
    rationals ``num / den``, the value is ``(sum w_y w_x p + D / 2) // D`` with ``D = den_y den_x`` -- then
    flipped when the row's fifth entry is set. ``crops``: ``[B, 5]`` rows ``{top, left, h, w, flip}``."""
    src = images.cpu().numpy().astype(np.int64)
    rows = np.asarray(torch.as_tensor(crops).cpu().numpy(), dtype=np.int64)
    out = np.zeros((src.shape[0], OH, OW, 3), dtype=np.uint8)
    for b, (top, left, h, w, fl) in enumerate(rows.tolist()):
        win = src[b, top : top + h, left : left + w]
        y0, y1, wy1, dy = _taps(h, OH)
        x0, x1, wx1, dx = _taps(w, OW)
        wy1, wy0 = wy1[:, None, None], (dy - wy1)[:, None, None]
        wx1, wx0 = wx1[None, :, None], (dx - wx1)[None, :, None]
        r0, r1 = win[y0], win[y1]
        t0 = wx0 * r0[:, x0] + wx1 * r0[:, x1]
        t1 = wx0 * r1[:, x0] + wx1 * r1[:, x1]
        D = dy * dx
        res = (wy0 * t0 + wy1 * t1 + D // 2) // D
        out[b] = (res[:, ::-1] if fl else res).astype(np.uint8)
    return torch.from_numpy(out)


def _gray(img):
    return (77 * img[..., 0] + 150 * img[..., 1] + 29 * img[..., 2] + 128) >> 8


def _blend(f8, v, d):
    return np.clip((f8 * v + (256 - f8) * d + 128) >> 8, 0, 255)


def _apply(img, row, fill):
    """One row on one int64 ``[H, W, 3]`` image."""
    op, p = int(row[0]) & 255, [int(v) for v in row[2:8]]
    H, W, _ = img.shape
    if op == IDENTITY:
        return img
    if SHEAR_X <= op <= ROTATE:
        a, b, c, d, tx, ty = p
        u = (2 * np.arange(W, dtype=np.int64) + 1 - W)[None, :]
        v = (2 * np.arange(H, dtype=np.int64) + 1 - H)[:, None]
        sx = (a * u + b * v + tx + 65536 * W) >> 17
        sy = (c * u + d * v + ty + 65536 * H) >> 17
        inside = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        got = img[np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
        return np.where(inside[..., None], got, np.asarray(fill, dtype=np.int64)[None, None, :])
    if op == BRIGHTNESS:
        return _blend(p[0], img, 0)
    if op == COLOR:
        return _blend(p[0], img, _gray(img)[..., None])
    if op == CONTRAST:
        n = H * W
        return _blend(p[0], img, (int(_gray(img).sum()) + n // 2) // n)
    if op == SHARPNESS:
        out = img.copy()
        if H >= 3 and W >= 3:
            s = 4 * img[1:-1, 1:-1]
            for dy in range(3):
                for dx in range(3):
                    s = s + img[dy : H - 2 + dy, dx : W - 2 + dx]
            out[1:-1, 1:-1] = _blend(p[0], img[1:-1, 1:-1], (s + 6) // 13)
        return out
    if op == POSTERIZE:
        return img & p[0]
    if op == SOLARIZE:
        return np.where(img >= p[0], 255 - img, img)
    if op == AUTO_CONTRAST:
        out = img.copy()
        for c in range(3):
            lo, hi = int(img[..., c].min()), int(img[..., c].max())
            if hi > lo:
                out[..., c] = ((img[..., c] - lo) * 255 + (hi - lo) // 2) // (hi - lo)
        return out
    if op == EQUALIZE:
        out = img.copy()
        for c in range(3):
            hist = np.bincount(img[..., c].ravel(), minlength=256).astype(np.int64)
            step = (int(hist.sum()) - int(hist[np.nonzero(hist)[0][-1]])) // 255
            if step == 0:
                continue
            lut = np.zeros(256, dtype=np.int64)
            lut[1:] = np.clip((np.cumsum(hist)[:-1] + step // 2) // step, 0, 255)
            out[..., c] = lut[img[..., c]]
        return out
    raise ValueError(f"randaug_reference: unknown op {op}")


def randaug_reference(images: torch.Tensor, rows, fill) -> torch.Tensor:
    """Apply published rows to uint8 images: ``images`` uint8 ``[B, H, W, 3]``, ``rows`` int ``[B, num_ops, 8]``,
    ``fill`` three ints in 0 .. 255 (the geometric ops' value outside the image). Returns uint8 ``[B, H, W, 3]``.
    numpy int64 arithmetic only: bitwise what ``randaug_kernel`` writes."""
    src = images.cpu().numpy().astype(np.int64)
    rows = np.asarray(torch.as_tensor(rows).cpu().numpy(), dtype=np.int64)
    out = np.empty(src.shape, dtype=np.uint8)
    for b in range(src.shape[0]):
        img = src[b]
        for row in rows[b]:
            img = _apply(img, row, fill)
        out[b] = img.astype(np.uint8)
    return torch.from_numpy(out)


def describe(row) -> str:
    """``Op(level)`` of a published row, e.g. ``Rotate(-9.25)``: the sign where the op has one."""
    op, lvl = int(row[0]) & 255, int(row[1]) / 256.0
    signed = SHEAR_X <= op <= SHARPNESS
    return "{}({}{:g})".format(RANDAUG_OPS[op], "-" if signed and int(row[0]) & NEG_BIT else "", lvl)
