"""Data pipeline: CIFAR-10 / ImageNet-shaped datasets resident in GPU memory, rank sharding and a
fused on-GPU augmentation loader.

Reference pipeline (``/root/reference/src/Part 1/main.py:82-109``, ``src/Part 2a/main.py:24-55``):
torchvision ``CIFAR10`` -> ``RandomCrop(32, padding=4)`` -> ``RandomHorizontalFlip()`` ->
``ToTensor()`` -> ``Normalize(mean=[125.3,123.0,113.9]/255, std=[63.0,62.1,66.7]/255)``, a
``DistributedSampler(num_replicas=W, rank=r)`` (``set_epoch`` never called), ``DataLoader`` with
2 worker processes and ``pin_memory``; the test loader is not sharded.

MI355X design: the whole uint8 dataset (150 MB for CIFAR-10) is uploaded once to HBM; each batch is
one gather + crop + flip + normalize kernel that writes NHWC fp32 straight into the model's input
layout. No worker processes, no host->device copies in the training loop, and the per-sample
random crop / flip come from a counter-based hash on the device, so the loader is also
hipGraph-capturable. torchvision is not installed here, so datasets are either synthetic (random
images of the right shape, fixed seed) or read from the CIFAR-10 *binary* distribution
(``cifar-10-batches-bin/*.bin``, raw bytes -- no unpickling).
"""
from __future__ import annotations

import math
import os
from typing import Iterator, List, NamedTuple, Optional

import numpy as np
import torch

from . import _native
from . import randaug as _ra
from .randaug import RANDAUG_OPS, randaug_reference

CIFAR_MEAN = [x / 255.0 for x in [125.3, 123.0, 113.9]]
CIFAR_STD = [x / 255.0 for x in [63.0, 62.1, 66.7]]
IMAGENET_MEAN = [0.485, 0.456, 0.406]
IMAGENET_STD = [0.229, 0.224, 0.225]


class ImageDataset:
    """uint8 images ``[N, H, W, C]`` + int64 labels, optionally resident on a device."""

    def __init__(self, images: torch.Tensor, labels: torch.Tensor, mean, std, pad: int = 4, name: str = "dataset"):
        assert images.dtype == torch.uint8 and images.dim() == 4
        self.images, self.labels = images, labels.long()
        self.mean, self.std, self.pad, self.name = list(mean), list(std), pad, name

    def __len__(self):
        return self.images.shape[0]

    def to(self, device):
        return ImageDataset(self.images.to(device), self.labels.to(device), self.mean, self.std, self.pad, self.name)

    @property
    def shape(self):
        return tuple(self.images.shape[1:])


def synthetic_cifar10(n: int = 50000, seed: int = 0, device="cpu", train: bool = True,
                      learnable: bool = False) -> ImageDataset:
    """Random CIFAR-10-shaped data (uint8 32x32x3, 10 classes) -- a stand-in for the real set.

    ``learnable``: the label is a fixed function of the image (argmax of one fixed random projection
    of its 8x8-average-pooled, normalised pixels, the same projection for train and test), so the
    loss falls and test accuracy rises above chance -- a check of the whole pipeline that random
    labels cannot give."""
    g = torch.Generator().manual_seed(seed + (0 if train else 1))
    imgs = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int64, generator=g)
    if learnable:
        proj = torch.randn(10, 3 * 4 * 4, generator=torch.Generator().manual_seed(12345))
        mean = torch.tensor(CIFAR_MEAN).view(1, 3, 1, 1)
        std = torch.tensor(CIFAR_STD).view(1, 3, 1, 1)
        for i in range(0, n, 4096):
            x = (imgs[i : i + 4096].permute(0, 3, 1, 2).float() / 255.0 - mean) / std
            feat = torch.nn.functional.avg_pool2d(x, 8).reshape(x.shape[0], -1)
            labels[i : i + 4096] = (feat @ proj.t()).argmax(1)
    return ImageDataset(imgs, labels, CIFAR_MEAN, CIFAR_STD, 4, "synthetic-cifar10").to(device)


def synthetic_imagenet(n: int = 1281, seed: int = 0, device="cpu", size: int = 224, classes: int = 1000) -> ImageDataset:
    g = torch.Generator().manual_seed(seed)
    imgs = torch.randint(0, 256, (n, size, size, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, classes, (n,), dtype=torch.int64, generator=g)
    return ImageDataset(imgs, labels, IMAGENET_MEAN, IMAGENET_STD, 0, "synthetic-imagenet").to(device)


def cifar10_binary(root: str, train: bool = True, device="cpu") -> ImageDataset:
    """Read the CIFAR-10 binary release (``data_batch_{1..5}.bin`` / ``test_batch.bin``).

    Each record is 1 label byte + 3072 bytes (CHW, R then G then B planes).
    """
    d = root
    if os.path.isdir(os.path.join(root, "cifar-10-batches-bin")):
        d = os.path.join(root, "cifar-10-batches-bin")
    files = [f"data_batch_{i}.bin" for i in range(1, 6)] if train else ["test_batch.bin"]
    recs = []
    for f in files:
        raw = np.fromfile(os.path.join(d, f), dtype=np.uint8)
        recs.append(raw.reshape(-1, 3073))
    a = np.concatenate(recs, 0)
    labels = torch.from_numpy(a[:, 0].astype(np.int64))
    imgs = torch.from_numpy(a[:, 1:].reshape(-1, 3, 32, 32).transpose(0, 2, 3, 1).copy())
    return ImageDataset(imgs, labels, CIFAR_MEAN, CIFAR_STD, 4, "cifar10").to(device)


class DistributedSampler:
    """Same index semantics as ``torch.utils.data.distributed.DistributedSampler``.

    Pads to a multiple of ``num_replicas`` by repeating from the start, shuffles with a generator
    seeded by ``seed + epoch`` and takes ``indices[rank::num_replicas]``. As in the reference,
    ``set_epoch`` is optional (without it every epoch repeats the same permutation).
    """

    def __init__(self, dataset, num_replicas: int = 1, rank: int = 0, shuffle: bool = True, seed: int = 0,
                 drop_last: bool = False):
        if rank >= num_replicas or rank < 0:
            raise ValueError(f"Invalid rank {rank}, rank should be in the interval [0, {num_replicas - 1}]")
        self.n = len(dataset)
        self.num_replicas, self.rank, self.shuffle, self.seed, self.drop_last = num_replicas, rank, shuffle, seed, drop_last
        self.epoch = 0
        if drop_last and self.n % num_replicas != 0:
            self.num_samples = math.ceil((self.n - num_replicas) / num_replicas)
        else:
            self.num_samples = math.ceil(self.n / num_replicas)
        self.total_size = self.num_samples * num_replicas

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def indices(self) -> List[int]:
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        if not self.drop_last:
            pad = self.total_size - len(idx)
            if pad <= len(idx):
                idx += idx[:pad]
            else:
                idx += (idx * math.ceil(pad / len(idx)))[:pad]
        else:
            idx = idx[: self.total_size]
        return idx[self.rank : self.total_size : self.num_replicas]

    def __iter__(self):
        return iter(self.indices())

    def __len__(self):
        return self.num_samples


class MixTarget(NamedTuple):
    """The target of a mixed batch (mixup / CutMix): ``CrossEntropyLoss`` takes it in place of the int64
    target and computes ``lam * CE(z, target) + (1 - lam) * CE(z, target_b)``.

    ``target_b[b]`` is the label of image ``B - 1 - b``, the image that ``b`` was mixed with; ``lam`` is a
    1-element fp32 view of ``info[1]``; ``info`` is the batch's published row
    ``{mode (0 none, 1 mixup, 2 cutmix), lam, lam_raw, y0, y1, x0, x1, 0}``."""

    target: torch.Tensor
    target_b: torch.Tensor
    lam: torch.Tensor
    info: torch.Tensor


MIX_MODES = ("none", "mixup", "cutmix")
ERASE_MODES = ("const", "rand", "pixel")


class DeviceLoader:
    """Batches ``(data[B,C,H,W] fp32 channels_last, target[B] int64)`` from a device-resident dataset.

    ``train=True`` applies RandomCrop(pad)+RandomHorizontalFlip on the device; normalisation always.
    ``sampler`` (e.g. :class:`DistributedSampler`) picks the indices; without one the order is
    sequential (``shuffle=False``) or a seeded permutation (``shuffle=True``).

    ``mixup_alpha`` / ``cutmix_alpha`` > 0 (and ``train=True``) mix every batch in the same kernel: one
    ``lam ~ Beta(alpha, alpha)`` per batch, drawn on the device from the step counter; image ``b`` is
    paired with image ``B - 1 - b``. A batch is mixed with probability ``mix_prob``; with both alphas set
    it is CutMix with probability ``mix_switch_prob``, else mixup. The target is then a
    :class:`MixTarget`. With both alphas 0 the loader returns exactly what it returns without them.

    ``rrc_scale=(lo, hi)`` (and ``train=True``) turns on RandomResizedCrop in the same kernel: per image a
    window of ``U(lo, hi)`` of the stored area and an aspect ratio log-uniform in ``rrc_ratio``
    (torchvision's ``get_params`` rule, drawn on the device from the step counter), resampled bilinearly
    (``align_corners=False``, no antialias) to ``out_size`` (an int or ``(OH, OW)``; default: the stored
    size), then the flip. It **replaces** the pad-shift RandomCrop: the dataset's ``pad`` is ignored. A
    training loader has no other way to change the size, so ``out_size`` without ``rrc_scale`` is an error.
    ``train=False`` with ``out_size`` and / or ``center_crop``: the central window of fraction
    ``center_crop`` (default 1.0) of each side, resized to ``out_size``; no flip, no randomness
    (``rrc_scale`` is ignored there, as the mix arguments are). The blend is not re-quantised to uint8
    before the normalisation. Each batch's windows are kept in ``last_crops`` (int32 ``[B, 5]``:
    ``top, left, h, w, flip``); mixup / CutMix compose (the CutMix box is in output pixels). With all four
    arguments at their defaults the loader is exactly what it is without them, and ``last_crops`` is None.

    ``erase_prob`` > 0 (and ``train=True``) turns on RandomErasing (Zhong et al.) in the same kernel: with
    that probability an image loses one box of ``U(erase_scale)`` of the output area and an aspect ratio
    ``h / w`` log-uniform in ``erase_ratio`` (torchvision's ``RandomErasing.get_params`` rule, drawn on the
    device from the step counter; a proposal needs ``1 <= h < H`` and ``1 <= w < W``, and after 10 rejected
    proposals the image is left alone). The box is in output pixels, on the normalised tensor, after crop,
    resize and flip and **before** the mix: the partner of a mixed image shows its own box. ``erase_mode``:
    ``"const"`` fills with ``erase_value`` (a float or three, in normalised units; 0 is torchvision's
    ``value=0`` after ``Normalize``), ``"rand"`` with one N(0, 1) value per channel per image (timm's
    ``rand``), ``"pixel"`` with one per element (torchvision's ``value="random"``, timm's ``pixel``). Each
    batch's boxes are kept in ``last_erase`` (int32 ``[B, 5]``: ``on, top, left, h, w``; all 0 for an image
    that was not erased); ``erase_schedule`` and ``erase_noise`` give the boxes and the noise of any step.
    ``train=False`` ignores the erase arguments. With ``erase_prob=0`` the loader is exactly what it is
    without them, and ``last_erase`` is None.

    ``randaug_num_ops`` > 0 (and ``train=True``; 3-channel images) turns on RandAugment (Cubuk et al.): every
    image gets that many operations, drawn uniformly with replacement from ``randaug_ops`` (names out of
    :data:`RANDAUG_OPS`; default: all 14), each with a random sign where it has one and a level
    ``L = clamp(randaug_magnitude + randaug_mstd * n, 0, 30)``, ``n ~ N(0, 1)`` per operation (torchvision's 31
    magnitude bins made continuous; ``mstd`` is timm's). They are applied in sequence to the uint8 image
    **between the crop / resize / flip and the normalisation** (torchvision's and timm's position), in one
    launch of their own that stages the batch as uint8 ``[B, OH, OW, 3]``; the loader's usual launch then
    normalises, erases and mixes the staged batch, so erasing and mixing compose with no change to their draws
    and the mix partner of an image shows the partner's own operations. All pixel arithmetic is integer
    arithmetic on the published rows (``last_randaug``, int32 ``[B, num_ops, 8]``:
    ``{op | sign << 8, level_q = round(256 L), p0 .. p5}``), so :func:`randaug_reference` reproduces
    ``last_randaug_images`` (the uint8 batch the normalising launch reads: a view of the staging buffer, valid
    until the next batch) bitwise. With the resize on, the bilinear blend is then exact in integers and
    re-quantised to uint8 (the PIL order), unlike the RandAugment-off resize. The geometric ops are
    nearest-neighbour and fill with ``randaug_fill`` (three ints in 0 .. 255; default ``round(255 * mean)``).
    ``randaug_schedule`` gives the rows of any step. ``train=False`` ignores these arguments. With
    ``randaug_num_ops=0`` the loader is exactly what it is without them, and ``last_randaug`` is None.
    """

    def __init__(self, dataset: ImageDataset, batch_size: int, sampler=None, shuffle: bool = False,
                 train: bool = True, drop_last: bool = False, seed: int = 0, mixup_alpha: float = 0.0,
                 cutmix_alpha: float = 0.0, mix_prob: float = 1.0, mix_switch_prob: float = 0.5,
                 out_size=None, rrc_scale=None, rrc_ratio=(3.0 / 4.0, 4.0 / 3.0), center_crop=None,
                 erase_prob: float = 0.0, erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3),
                 erase_mode: str = "const", erase_value=0.0, randaug_num_ops: int = 0,
                 randaug_magnitude: float = 9.0, randaug_mstd: float = 0.0, randaug_ops=None, randaug_fill=None):
        if not (mixup_alpha >= 0.0 and cutmix_alpha >= 0.0):
            raise ValueError(f"mixup_alpha and cutmix_alpha must be >= 0. Got: {mixup_alpha}, {cutmix_alpha}")
        if not (0.0 <= mix_prob <= 1.0 and 0.0 <= mix_switch_prob <= 1.0):
            raise ValueError(f"mix_prob and mix_switch_prob must be in [0, 1]. Got: {mix_prob}, {mix_switch_prob}")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.mix_prob, self.mix_switch_prob = float(mix_prob), float(mix_switch_prob)
        if rrc_scale is not None:
            rrc_scale = tuple(float(v) for v in rrc_scale)
            if not (len(rrc_scale) == 2 and 0.0 < rrc_scale[0] <= rrc_scale[1] <= 1.0):
                raise ValueError(f"rrc_scale must be (lo, hi) with 0 < lo <= hi <= 1. Got: {rrc_scale}")
        rrc_ratio = tuple(float(v) for v in rrc_ratio)
        if not (len(rrc_ratio) == 2 and 0.0 < rrc_ratio[0] <= rrc_ratio[1] < math.inf):
            raise ValueError(f"rrc_ratio must be (lo, hi) with 0 < lo <= hi. Got: {rrc_ratio}")
        if center_crop is not None and not (0.0 < float(center_crop) <= 1.0):
            raise ValueError(f"center_crop must be in (0, 1]. Got: {center_crop}")
        if out_size is not None:
            out_size = (out_size, out_size) if isinstance(out_size, int) else tuple(int(v) for v in out_size)
            if not (len(out_size) == 2 and all(1 <= v < 32768 for v in out_size)):
                raise ValueError(f"out_size must be an int or (OH, OW) with 1 <= OH, OW < 32768. Got: {out_size}")
        if train and out_size is not None and rrc_scale is None:
            raise ValueError(f"out_size={out_size} on a training loader needs rrc_scale: RandomResizedCrop is its "
                             "only way to change the size")
        self.rrc_scale, self.rrc_ratio = rrc_scale, rrc_ratio
        self.center_crop = 1.0 if center_crop is None else float(center_crop)
        # resizing: the augment_resize path (RandomResizedCrop when training, resize + center crop otherwise)
        self.resizing = rrc_scale is not None if train else (out_size is not None or center_crop is not None)
        self.out_size = out_size if out_size is not None else tuple(dataset.images.shape[1:3])
        self.last_crops = None
        if not (0.0 <= float(erase_prob) <= 1.0):
            raise ValueError(f"erase_prob must be in [0, 1]. Got: {erase_prob}")
        erase_scale = tuple(float(v) for v in erase_scale)
        if not (len(erase_scale) == 2 and 0.0 < erase_scale[0] <= erase_scale[1] <= 1.0):
            raise ValueError(f"erase_scale must be (lo, hi) with 0 < lo <= hi <= 1. Got: {erase_scale}")
        erase_ratio = tuple(float(v) for v in erase_ratio)
        if not (len(erase_ratio) == 2 and 0.0 < erase_ratio[0] <= erase_ratio[1] < math.inf):
            raise ValueError(f"erase_ratio must be (lo, hi) with 0 < lo <= hi. Got: {erase_ratio}")
        if erase_mode not in ERASE_MODES:
            raise ValueError(f"erase_mode must be one of {ERASE_MODES}. Got: {erase_mode!r}")
        value = [float(erase_value)] * 3 if isinstance(erase_value, (int, float)) else [float(v) for v in erase_value]
        if not (len(value) == 3 and all(math.isfinite(v) for v in value)):
            raise ValueError(f"erase_value must be a finite float or three of them. Got: {erase_value}")
        self.erase_prob, self.erase_scale, self.erase_ratio = float(erase_prob), erase_scale, erase_ratio
        self.erase_mode, self.erase_value = erase_mode, value
        self.last_erase = None
        if not (isinstance(randaug_num_ops, int) and 0 <= randaug_num_ops <= _ra.MAX_OPS):
            raise ValueError(f"randaug_num_ops must be an int in 0 .. {_ra.MAX_OPS}. Got: {randaug_num_ops}")
        if not (0.0 <= float(randaug_magnitude) <= 30.0):
            raise ValueError(f"randaug_magnitude must be in [0, 30]. Got: {randaug_magnitude}")
        if not (0.0 <= float(randaug_mstd) < math.inf):
            raise ValueError(f"randaug_mstd must be >= 0. Got: {randaug_mstd}")
        names = RANDAUG_OPS if randaug_ops is None else ((randaug_ops,) if isinstance(randaug_ops, str)
                                                         else tuple(randaug_ops))
        if not (1 <= len(names) <= _ra.MAX_NAMES and all(n in RANDAUG_OPS for n in names)):
            raise ValueError(f"randaug_ops must be 1 .. {_ra.MAX_NAMES} names out of {RANDAUG_OPS}. Got: {randaug_ops}")
        if randaug_fill is None:
            fill = [min(255, max(0, int(round(255.0 * float(dataset.mean[min(c, len(dataset.mean) - 1)])))))
                    for c in range(3)]
        else:
            fill = list(randaug_fill) if isinstance(randaug_fill, (tuple, list)) else None
            if not (fill is not None and len(fill) == 3
                    and all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v <= 255 for v in fill)):
                raise ValueError(f"randaug_fill must be three integers in 0 .. 255. Got: {randaug_fill}")
        if train and randaug_num_ops > 0 and dataset.images.shape[3] != 3:
            raise ValueError(f"RandAugment needs 3-channel images. Got: {dataset.images.shape[3]} channels")
        self.randaug_num_ops, self.randaug_magnitude = randaug_num_ops, float(randaug_magnitude)
        self.randaug_mstd, self.randaug_ops, self.randaug_fill = float(randaug_mstd), names, fill
        self._randaug_kinds = [RANDAUG_OPS.index(n) for n in names]
        self.last_randaug = None
        self.last_randaug_images = None
        self._randaug_bufs = {}
        self.ds, self.batch_size, self.sampler, self.shuffle = dataset, batch_size, sampler, shuffle
        self.train, self.drop_last, self.seed = train, drop_last, seed
        self.dev = dataset.images.device
        self._counter = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self._epoch = 0
        self._external_advance = False

    def _order(self) -> torch.Tensor:
        if self.sampler is not None:
            idx = torch.tensor(list(iter(self.sampler)), dtype=torch.int64)
        elif self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self._epoch)
            idx = torch.randperm(len(self.ds), generator=g)
        else:
            idx = torch.arange(len(self.ds), dtype=torch.int64)
        return idx.to(self.dev)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.ds)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def advance_with(self, optimizer) -> bool:
        """Let ``optimizer`` advance this loader's step counter inside its step kernel (cdp.SGD
        ``advance_each_step``) instead of a one-thread launch per batch. One batch per optimizer
        step only; GPU datasets only (returns False otherwise). ``advance_with(None)`` detaches it
        again (e.g. before gradient accumulation or an evaluation pass over the same loader): the
        loader then advances its counter at every batch itself. An eager batch() fetched twice
        without an optimizer step in between warns once (both batches would share a seed)."""
        prev = getattr(self, "_advancer", None)
        if optimizer is None:
            if prev is not None and getattr(prev, "_step_counter", None) is self._counter:
                prev.advance_each_step(None)
            self._advancer = None
            self._external_advance = False
            return True
        if self.dev.type != "cuda" or not hasattr(optimizer, "advance_each_step"):
            return False
        if prev is not None and prev is not optimizer:
            self.advance_with(None)
        optimizer.advance_each_step(self._counter)
        self._advancer = optimizer
        self._advance_seen = None
        self._external_advance = True
        return True

    def _check_one_batch_per_step(self):
        opt = getattr(self, "_advancer", None)
        if opt is None or torch.cuda.is_current_stream_capturing():
            return
        steps = getattr(opt, "_steps", None)
        if steps is not None and steps == self._advance_seen and not getattr(self, "_warned_reuse", False):
            import warnings

            warnings.warn("DeviceLoader: two batches without an optimizer step while the optimizer advances the "
                          "loader's step counter (advance_with): they share an augmentation seed and batch offset; "
                          "call advance_with(None) for gradient accumulation or evaluation", stacklevel=3)
            self._warned_reuse = True
        self._advance_seen = steps

    @property
    def dataset(self):
        return self.ds

    @property
    def mixing(self) -> bool:
        """Whether batches are mixed (an alpha > 0 on a training loader) and carry a :class:`MixTarget`."""
        return self.train and (self.mixup_alpha > 0.0 or self.cutmix_alpha > 0.0)

    @property
    def erasing(self) -> bool:
        """Whether images are erased (``erase_prob`` > 0 on a training loader)."""
        return self.train and self.erase_prob > 0.0

    @property
    def randaugmenting(self) -> bool:
        """Whether images get RandAugment operations (``randaug_num_ops`` > 0 on a training loader)."""
        return self.train and self.randaug_num_ops > 0

    def _randaug_stage(self, C, idx, offset, bsz, nbatches, pad, flip):
        """The RandAugment launch: the batch gathered, cropped, flipped and augmented as uint8 in the loader's
        staging buffers (allocated once per batch shape: a captured step allocates nothing per replay), and its
        labels. Publishes ``last_randaug``, ``last_randaug_images`` and, with the resize, ``last_crops``."""
        OH, OW = self.out_size if self.resizing else tuple(self.ds.shape[:2])
        bufs = self._randaug_bufs.get((bsz, OH, OW))
        if bufs is None:
            bufs = (torch.empty(bsz, OH, OW, 3, dtype=torch.uint8, device=self.dev),
                    torch.empty(bsz, OH, OW, 3, dtype=torch.uint8, device=self.dev),
                    torch.empty(bsz, dtype=torch.int64, device=self.dev))
            self._randaug_bufs[(bsz, OH, OW)] = bufs
        buf_a, buf_b, staged_labels = bufs
        rows = torch.empty(bsz, self.randaug_num_ops, _ra.ROW, dtype=torch.int32, device=self.dev)
        crops = torch.empty(bsz, 5, dtype=torch.int32, device=self.dev) if self.resizing else None
        C.randaug(self.ds.images, idx, offset, bsz, OH, OW, self.resizing, self.rrc_scale or (1.0, 1.0), self.rrc_ratio,
                  pad, flip, self._counter, self.seed, nbatches, self.ds.labels, staged_labels, crops,
                  self.randaug_num_ops, self.randaug_magnitude, self.randaug_mstd, self._randaug_kinds,
                  self.randaug_fill, buf_a, buf_b, rows)
        self.last_randaug = rows
        self.last_randaug_images = buf_a if self.randaug_num_ops % 2 == 0 else buf_b
        if self.resizing:
            self.last_crops = crops
        return self.last_randaug_images, staged_labels

    def randaug_schedule(self, first_counter: int, n: int, B: int) -> torch.Tensor:
        """The RandAugment rows ``{op | sign << 8, level_q, p0 .. p5}`` of the ``B`` images of the batches at step
        counters ``first_counter .. first_counter + n - 1`` (int32 ``[n, B, num_ops, 8]``; training loaders with
        ``randaug_num_ops`` > 0)."""
        if not self.randaugmenting:
            raise ValueError("randaug_schedule: a training loader with randaug_num_ops > 0 draws operations; this "
                             "one does not")
        H, W = self._erase_size()
        if self.dev.type == "cuda":
            return _native.lib().randaug_params(self.seed, first_counter, n, B, self.randaug_num_ops,
                                                self.randaug_magnitude, self.randaug_mstd, self._randaug_kinds,
                                                self.randaug_fill, H, W)
        return torch.stack([_ra.randaug_draw(self.seed, first_counter + i, B, self.randaug_num_ops,
                                             self.randaug_magnitude, self.randaug_mstd, self._randaug_kinds, H, W)
                            for i in range(n)]) if n else torch.zeros(0, B, self.randaug_num_ops, _ra.ROW,
                                                                      dtype=torch.int32)

    def batch(self, idx: torch.Tensor, offset: int, bsz: int, out: Optional[torch.Tensor] = None,
              nbatches: int = 0):
        """Produce one batch from ``idx[offset:offset+bsz]`` (graph-capturable on GPU).

        ``nbatches > 0``: the batch is ``idx[offset + (step % nbatches) * bsz :][:bsz]`` with ``step``
        the loader's on-device step counter, so one captured hipGraph walks the whole order with no
        per-step host work. The labels are gathered by the same kernel.
        """
        pad = self.ds.pad if self.train else 0
        flip = self.train
        if offset < 0 or offset + max(nbatches, 1) * bsz > idx.numel():
            raise ValueError(f"DeviceLoader.batch: offset {offset} + {max(nbatches, 1)} batches x {bsz} exceeds the "
                             f"{idx.numel()} indices of this shard")
        if self.dev.type == "cuda":
            C = _native.lib()
            target = torch.empty(bsz, dtype=torch.int64, device=self.dev)
            ekw = {}
            if self.erasing:
                # the same launch draws every image's box from the step counter, fills it and publishes it
                self.last_erase = torch.empty(bsz, 5, dtype=torch.int32, device=self.dev)
                ekw = dict(erase_prob=self.erase_prob, erase_scale=self.erase_scale, erase_ratio=self.erase_ratio,
                           erase_mode=self.erase_mode, erase_value=self.erase_value, erase=self.last_erase)
            if self.randaugmenting:
                # one launch stages the batch as uint8 and applies every image's operations; the plain augment
                # launch below then normalises, erases and mixes the staged batch (identity indices, no crop, no
                # flip) with the draws of the same counter
                if self.resizing and out is not None and tuple(out.shape) != (bsz, 3) + tuple(self.out_size):
                    raise ValueError(f"DeviceLoader.batch: out has shape {tuple(out.shape)}, the batch is "
                                     f"{(bsz, 3) + tuple(self.out_size)}")
                staged, staged_labels = self._randaug_stage(C, idx, offset, bsz, nbatches, pad, flip)
                mkw = {}
                if self.mixing:
                    target_b = torch.empty(bsz, dtype=torch.int64, device=self.dev)
                    info = torch.empty(8, dtype=torch.float32, device=self.dev)
                    mkw = dict(mixup_alpha=self.mixup_alpha, cutmix_alpha=self.cutmix_alpha, mix_prob=self.mix_prob,
                               mix_switch_prob=self.mix_switch_prob, mix=info, labels_b=target_b)
                data = C.augment(staged, None, 0, bsz, self.ds.mean, self.ds.std, 0, False, self._counter, self.seed,
                                 out, 0, staged_labels, target, **mkw, **ekw)
                if self.mixing:
                    target = MixTarget(target, target_b, info[1:2], info)
            elif self.resizing:
                OH, OW = self.out_size
                if out is not None and tuple(out.shape) != (bsz, self.ds.shape[2], OH, OW):
                    raise ValueError(f"DeviceLoader.batch: out has shape {tuple(out.shape)}, the batch is "
                                     f"{(bsz, self.ds.shape[2], OH, OW)}")
                crops = torch.empty(bsz, 5, dtype=torch.int32, device=self.dev)
                args = (self.ds.images, idx, offset, bsz, self.ds.mean, self.ds.std, OH, OW, self.train,
                        self.rrc_scale or (1.0, 1.0), self.rrc_ratio, self.center_crop, flip, self._counter,
                        self.seed, out, nbatches, self.ds.labels, target, crops)
                if self.mixing:
                    target_b = torch.empty(bsz, dtype=torch.int64, device=self.dev)
                    info = torch.empty(8, dtype=torch.float32, device=self.dev)
                    data = C.augment_resize(*args, mixup_alpha=self.mixup_alpha, cutmix_alpha=self.cutmix_alpha,
                                            mix_prob=self.mix_prob, mix_switch_prob=self.mix_switch_prob, mix=info,
                                            labels_b=target_b, **ekw)
                    target = MixTarget(target, target_b, info[1:2], info)
                else:
                    data = C.augment_resize(*args, **ekw)
                self.last_crops = crops
            elif self.mixing:
                # the same launch draws the batch's mix from the step counter, applies it and publishes it
                target_b = torch.empty(bsz, dtype=torch.int64, device=self.dev)
                info = torch.empty(8, dtype=torch.float32, device=self.dev)
                data = C.augment(self.ds.images, idx, offset, bsz, self.ds.mean, self.ds.std, pad, flip, self._counter,
                                 self.seed, out, nbatches, self.ds.labels, target, mixup_alpha=self.mixup_alpha,
                                 cutmix_alpha=self.cutmix_alpha, mix_prob=self.mix_prob,
                                 mix_switch_prob=self.mix_switch_prob, mix=info, labels_b=target_b, **ekw)
                target = MixTarget(target, target_b, info[1:2], info)
            else:
                data = C.augment(self.ds.images, idx, offset, bsz, self.ds.mean, self.ds.std, pad, flip,
                                 self._counter, self.seed, out, nbatches, self.ds.labels, target, **ekw)
            if not self._external_advance:
                C.counter_inc(self._counter)
            else:
                self._check_one_batch_per_step()
            return data, target
        ctr = int(self._counter.item()) if (nbatches > 0 or self.mixing or self.resizing or self.erasing
                                            or self.randaugmenting) else None
        if nbatches > 0:
            offset += (ctr % nbatches) * bsz
        if self.randaugmenting:
            self._counter += 1
            data, target = self._cpu_randaug_batch(idx[offset : offset + bsz], pad, flip, ctr)
            if self.erasing:
                data = self._cpu_erase(data, ctr)
            if out is not None:
                data = out.copy_(data)
            return self._cpu_mix(data, target, ctr) if self.mixing else (data, target)
        if self.resizing:
            self._counter += 1
            data, target = self._cpu_resize_batch(idx[offset : offset + bsz], flip, ctr)
            if self.erasing:
                data = self._cpu_erase(data, ctr)
            if out is not None:
                data = out.copy_(data)
            return self._cpu_mix(data, target, ctr) if self.mixing else (data, target)
        if ctr is not None and not pad:
            self._counter += 1  # (the padded path advances it itself)
        data, target = self._cpu_batch(idx[offset : offset + bsz], pad, flip)
        if self.erasing:
            data = self._cpu_erase(data, ctr)
        if self.mixing:
            return self._cpu_mix(data, target, ctr)
        return data, target

    def mix_schedule(self, first_counter: int, n: int) -> torch.Tensor:
        """The rows ``{mode, lam, lam_raw, y0, y1, x0, x1, 0}`` that the batches at step counters
        ``first_counter .. first_counter + n - 1`` publish (float32 ``[n, 8]``; GPU loaders)."""
        H, W = self.out_size if self.resizing else self.ds.shape[:2]
        return _native.lib().mix_params(self.seed, first_counter, n, self.mixup_alpha, self.cutmix_alpha,
                                        self.mix_prob, self.mix_switch_prob, H, W)

    def crop_schedule(self, first_counter: int, n: int, B: int) -> torch.Tensor:
        """The RandomResizedCrop windows ``{top, left, h, w}`` of the ``B`` images of the batches at step
        counters ``first_counter .. first_counter + n - 1`` (int32 ``[n, B, 4]``; GPU training loaders with
        ``rrc_scale``)."""
        if not (self.train and self.rrc_scale is not None):
            raise ValueError("crop_schedule: a training loader with rrc_scale draws windows; this one does not")
        H, W = self.ds.shape[:2]
        return _native.lib().rrc_params(self.seed, first_counter, n, B, self.rrc_scale, self.rrc_ratio, H, W)

    def _erase_size(self):
        return self.out_size if self.resizing else tuple(self.ds.shape[:2])

    def erase_schedule(self, first_counter: int, n: int, B: int) -> torch.Tensor:
        """The RandomErasing rows ``{on, top, left, h, w}`` of the ``B`` images of the batches at step counters
        ``first_counter .. first_counter + n - 1`` (int32 ``[n, B, 5]``; training loaders with ``erase_prob`` > 0)."""
        if not self.erasing:
            raise ValueError("erase_schedule: a training loader with erase_prob > 0 draws boxes; this one does not")
        H, W = self._erase_size()
        if self.dev.type == "cuda":
            return _native.lib().erase_params(self.seed, first_counter, n, B, self.erase_prob, self.erase_scale,
                                              self.erase_ratio, H, W)
        rows = torch.zeros(n, B, 5, dtype=torch.int32)
        for i in range(n):
            g = self._cpu_erase_generator(first_counter + i)
            for b in range(B):
                rows[i, b] = torch.tensor(self._erase_get_params(H, W, self.erase_prob, self.erase_scale,
                                                                 self.erase_ratio, g), dtype=torch.int32)
        return rows

    def erase_noise(self, counter: int, B: int) -> torch.Tensor:
        """The N(0, 1) fill noise of the ``B`` images of the batch at step counter ``counter`` (float32
        ``[B, 3, H, W]`` channels_last, H x W the output size): ``"pixel"`` fills element ``(b, c, y, x)`` of a
        box with ``[b, c, y, x]``, ``"rand"`` fills the whole box of channel ``c`` with ``[b, c, 0, 0]``."""
        if not self.erasing:
            raise ValueError("erase_noise: a training loader with erase_prob > 0 erases; this one does not")
        H, W = self._erase_size()
        if self.dev.type == "cuda":
            return _native.lib().erase_noise(self.seed, counter, B, H, W)
        g = torch.Generator().manual_seed((0x6E6F697365 << 24) + self.seed * 1000003 + counter)
        return torch.randn(B, H, W, 3, generator=g).permute(0, 3, 1, 2)

    def _cpu_erase_generator(self, ctr):
        return torch.Generator().manual_seed((0x6572617365 << 24) + self.seed * 1000003 + ctr)

    @staticmethod
    def _erase_get_params(H, W, prob, scale, ratio, g):
        """torchvision's ``RandomErasing.get_params`` rule with draws from the generator ``g``: the row
        ``(on, top, left, h, w)`` of one image. One probability draw, then 10 proposals of four draws each (area,
        aspect ``h / w``, top, left), all taken from ``g`` whether used or not; a proposal needs ``1 <= h < H`` and
        ``1 <= w < W``."""
        u = torch.rand(41, generator=g, dtype=torch.float64).tolist()
        if not u[0] < prob:
            return 0, 0, 0, 0, 0
        area = H * W
        log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
        for i in range(10):
            u_s, u_r, u_t, u_l = u[1 + 4 * i : 5 + 4 * i]
            target = area * (scale[0] + (scale[1] - scale[0]) * u_s)
            aspect = math.exp(log_lo + (log_hi - log_lo) * u_r)
            h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 1 <= h < H and 1 <= w < W:
                return 1, min(int(u_t * (H - h + 1)), H - h), min(int(u_l * (W - w + 1)), W - w), h, w
        return 0, 0, 0, 0, 0

    def _cpu_erase(self, data, ctr):
        """The device kernels' semantics on the host: per image the box rule from a generator of its own (seeded
        apart from the crop / flip, window and mix generators, whose draws are therefore unchanged), the fill of
        the mode (the noise from a second generator: ``erase_noise`` returns it for any counter), and the
        published rows in ``last_erase``. It runs before ``_cpu_mix``, whose partner ``data.flip(0)`` then shows
        every image's own box."""
        B, _, H, W = data.shape
        rows = self.erase_schedule(ctr, 1, B)[0]
        self.last_erase = rows
        if not bool(rows[:, 0].any()):
            return data
        data = data.clone(memory_format=torch.channels_last)
        noise = self.erase_noise(ctr, B) if self.erase_mode != "const" else None
        value = torch.tensor(self.erase_value, dtype=torch.float32).view(3, 1, 1)
        for b, (on, top, left, h, w) in enumerate(rows.tolist()):
            if not on:
                continue
            if self.erase_mode == "const":
                fill = value
            elif self.erase_mode == "rand":
                fill = noise[b, :, :1, :1]
            else:
                fill = noise[b, :, top : top + h, left : left + w]
            data[b, :, top : top + h, left : left + w] = fill
        return data

    @staticmethod
    def _rrc_get_params(H, W, scale, ratio, g):
        """torchvision's ``RandomResizedCrop.get_params`` rule with draws from the generator ``g``."""
        area = H * W
        log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
        for _ in range(10):
            u_s, u_r, u_t, u_l = torch.rand(4, generator=g, dtype=torch.float64).tolist()
            target = area * (scale[0] + (scale[1] - scale[0]) * u_s)
            aspect = math.exp(log_lo + (log_hi - log_lo) * u_r)
            w, h = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
            if 0 < w <= W and 0 < h <= H:
                return min(int(u_t * (H - h + 1)), H - h), min(int(u_l * (W - w + 1)), W - w), h, w
        in_ratio = W / H
        h, w = H, W
        if in_ratio < ratio[0]:
            h = min(max(int(round(W / ratio[0])), 1), H)
        elif in_ratio > ratio[1]:
            w = min(max(int(round(H * ratio[1])), 1), W)
        return (H - h) // 2, (W - w) // 2, h, w

    def _cpu_resize_batch(self, sel, flip, ctr):
        """The resize kernel's semantics on the host: per image the window rule (a generator of its own,
        seeded apart from the crop / flip and the mix generators), ``F.interpolate`` of the window
        (bilinear, ``align_corners=False``, no antialias, not re-quantised), the flip, the normalisation."""
        H, W = self.ds.shape[:2]
        OH, OW = self.out_size
        g = torch.Generator().manual_seed((0x727263 << 40) + self.seed * 1000003 + ctr)
        # fp64: F.interpolate in fp32 rounds the source coordinate itself, the kernel's integer form does not
        imgs = self.ds.images.index_select(0, sel).permute(0, 3, 1, 2).double()  # NCHW, 0 .. 255
        B = imgs.shape[0]
        out = torch.empty(B, imgs.shape[1], OH, OW, dtype=torch.float64)
        crops = torch.zeros(B, 5, dtype=torch.int32)
        eh, ew = max(1, int(round(self.center_crop * H))), max(1, int(round(self.center_crop * W)))
        for b in range(B):
            if self.train:
                top, left, h, w = self._rrc_get_params(H, W, self.rrc_scale, self.rrc_ratio, g)
                fl = bool(flip) and float(torch.rand(1, generator=g)) < 0.5
            else:
                top, left, h, w, fl = (H - eh) // 2, (W - ew) // 2, eh, ew, False
            win = imgs[b : b + 1, :, top : top + h, left : left + w]
            res = torch.nn.functional.interpolate(win, size=(OH, OW), mode="bilinear", align_corners=False,
                                                  antialias=False)[0]
            out[b] = res.flip(-1) if fl else res
            crops[b] = torch.tensor([top, left, h, w, int(fl)], dtype=torch.int32)
        self.last_crops = crops
        mean = torch.tensor(self.ds.mean, dtype=torch.float64).view(1, -1, 1, 1)
        std = torch.tensor(self.ds.std, dtype=torch.float64).view(1, -1, 1, 1)
        out = ((out / 255.0 - mean) / std).float()
        return out.contiguous(memory_format=torch.channels_last), self.ds.labels.index_select(0, sel)

    def _cpu_randaug_batch(self, sel, pad, flip, ctr):
        """The RandAugment launch's semantics on the host: the batch staged as uint8 (the pad-shift crop and flip
        of ``_cpu_batch``'s generator, or the window rule of ``_cpu_resize_batch``'s generator with the exact
        integer bilinear :func:`randaug.stage_resize`), the host evaluation of the device's draw (ops and signs
        are the device's), :func:`randaug_reference`, then the normalisation."""
        imgs = self.ds.images.index_select(0, sel)
        B, H, W, _ = imgs.shape
        if self.resizing:
            OH, OW = self.out_size
            g = torch.Generator().manual_seed((0x727263 << 40) + self.seed * 1000003 + ctr)
            crops = torch.zeros(B, 5, dtype=torch.int32)
            for b in range(B):
                top, left, h, w = self._rrc_get_params(H, W, self.rrc_scale, self.rrc_ratio, g)
                fl = bool(flip) and float(torch.rand(1, generator=g)) < 0.5
                crops[b] = torch.tensor([top, left, h, w, int(fl)], dtype=torch.int32)
            self.last_crops = crops
            staged = _ra.stage_resize(imgs, crops, OH, OW)
        else:
            OH, OW = H, W
            g = torch.Generator().manual_seed(self.seed * 1000003 + ctr)
            if pad:
                oy = (torch.randint(0, 2 * pad + 1, (B,), generator=g) - pad).tolist()
                ox = (torch.randint(0, 2 * pad + 1, (B,), generator=g) - pad).tolist()
            else:
                oy = ox = [0] * B
            fl = (torch.rand(B, generator=g) < 0.5).tolist() if flip else [False] * B
            staged = _ra.stage_plain(imgs, oy, ox, fl)
        rows = _ra.randaug_draw(self.seed, ctr, B, self.randaug_num_ops, self.randaug_magnitude, self.randaug_mstd,
                                self._randaug_kinds, OH, OW)
        self.last_randaug = rows
        self.last_randaug_images = randaug_reference(staged, rows, self.randaug_fill)
        mean = torch.tensor(self.ds.mean).view(1, -1, 1, 1)
        std = torch.tensor(self.ds.std).view(1, -1, 1, 1)
        x = (self.last_randaug_images.permute(0, 3, 1, 2).float().div_(255.0) - mean) / std
        return x.contiguous(memory_format=torch.channels_last), self.ds.labels.index_select(0, sel)

    def _cpu_mix(self, data, target, ctr):
        """The device kernel's semantics on the host: one draw per batch from a generator of its own
        (seeded apart from the crop / flip generator, whose draws are therefore unchanged), the pairing
        ``b <-> B - 1 - b`` and the published box rule."""
        H, W = data.shape[2], data.shape[3]
        seed = (0x6D6978 << 40) + self.seed * 1000003 + ctr
        g = torch.Generator().manual_seed(seed)
        u_on, u_sw, u_y, u_x = torch.rand(4, generator=g, dtype=torch.float64).tolist()
        mu, cm = self.mixup_alpha > 0.0, self.cutmix_alpha > 0.0
        mode, lam, lam_raw, box = 0, 1.0, 1.0, (0, 0, 0, 0)
        if u_on < self.mix_prob:
            cut = cm and (not mu or u_sw < self.mix_switch_prob)
            alpha = self.cutmix_alpha if cut else self.mixup_alpha
            with torch.random.fork_rng(devices=[]):  # Beta samples from the default generator: seeded, then restored
                torch.manual_seed(seed)
                lam_raw = float(torch.distributions.Beta(torch.tensor(alpha), torch.tensor(alpha)).sample())
            if cut:
                r = math.sqrt(1.0 - lam_raw)
                cut_h, cut_w = int(H * r), int(W * r)
                cy, cx = min(int(u_y * H), H - 1), min(int(u_x * W), W - 1)
                y0, y1 = max(cy - cut_h // 2, 0), min(cy + cut_h // 2, H)
                x0, x1 = max(cx - cut_w // 2, 0), min(cx + cut_w // 2, W)
                mode, box = 2, (y0, y1, x0, x1)
                lam = 1.0 - (y1 - y0) * (x1 - x0) / (H * W)
            else:
                mode, lam = 1, lam_raw
        info = torch.tensor([mode, lam, lam_raw, *box, 0], dtype=torch.float32)
        lam = float(info[1])
        partner = data.flip(0)
        if mode == 1:
            data = (data * lam + partner * (1.0 - lam)).contiguous(memory_format=torch.channels_last)
        elif mode == 2:
            data = data.clone(memory_format=torch.channels_last)
            y0, y1, x0, x1 = box
            data[:, :, y0:y1, x0:x1] = partner[:, :, y0:y1, x0:x1]
        return data, MixTarget(target, target.flip(0), info[1:2], info)

    def _cpu_batch(self, sel, pad, flip):
        imgs = self.ds.images.index_select(0, sel).permute(0, 3, 1, 2).float().div_(255.0)  # NCHW
        if pad:
            g = torch.Generator().manual_seed(self.seed * 1000003 + int(self._counter.item()))
            self._counter += 1
            B, C, H, W = imgs.shape
            padded = torch.nn.functional.pad(imgs, (pad, pad, pad, pad))
            out = torch.empty_like(imgs)
            oy = torch.randint(0, 2 * pad + 1, (B,), generator=g)
            ox = torch.randint(0, 2 * pad + 1, (B,), generator=g)
            fl = torch.rand(B, generator=g) < 0.5 if flip else torch.zeros(B, dtype=torch.bool)
            for b in range(B):
                crop = padded[b, :, oy[b] : oy[b] + H, ox[b] : ox[b] + W]
                out[b] = crop.flip(-1) if fl[b] else crop
            imgs = out
        mean = torch.tensor(self.ds.mean).view(1, -1, 1, 1)
        std = torch.tensor(self.ds.std).view(1, -1, 1, 1)
        imgs = (imgs - mean) / std
        return imgs.contiguous(memory_format=torch.channels_last), self.ds.labels.index_select(0, sel)

    def __iter__(self) -> Iterator:
        idx = self._order()
        n = idx.numel()
        self._epoch += 1
        b = self.batch_size
        stop = (n // b) * b if self.drop_last else n
        for off in range(0, stop, b):
            yield self.batch(idx, off, min(b, n - off))
