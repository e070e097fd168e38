"""nn.Module wrappers of the fused ops."""
import torch.nn as nn

from . import functional as CF


class CrossEntropyLoss(nn.Module):
    """``torch.nn.CrossEntropyLoss(label_smoothing=...)`` (mean reduction) on the fused softmax-xent kernel.

    ``label_smoothing`` in [0, 1] trains against ``(1 - label_smoothing) * onehot + label_smoothing / C``;
    0.0 (the default) is the reference's plain criterion.

    ``target`` is an int64 tensor or the :class:`~..data.MixTarget` of a mixed batch (mixup / CutMix), for
    which the loss is ``lam * CE(logits, target) + (1 - lam) * CE(logits, target_b)`` in the same kernels.

    Reference: ``torch.nn.CrossEntropyLoss().to(device)`` at ``/root/reference/src/Part 1/main.py:110``.
    """

    def __init__(self, label_smoothing: float = 0.0):
        super().__init__()
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
        self.label_smoothing = float(label_smoothing)

    def forward(self, logits, target):
        from ..data import MixTarget

        if isinstance(target, MixTarget):
            return CF.cross_entropy(logits, target.target, self.label_smoothing, target_b=target.target_b,
                                    lam=target.lam)
        return CF.cross_entropy(logits, target, self.label_smoothing)

    def extra_repr(self):
        return f"label_smoothing={self.label_smoothing}"


class BinaryCrossEntropy(nn.Module):
    """Binary cross-entropy with logits over index and mixed targets, on the fused loss kernels: every logit
    is its own one-vs-rest sigmoid classifier (the loss of the "ResNet strikes back" recipe, timm's
    ``BinaryCrossEntropy(smoothing, target_threshold)`` composed with its ``mixup_target``).

    ``target`` is an int64 tensor or the :class:`~..data.MixTarget` of a mixed batch. The dense target
    ``(1 - label_smoothing) * (lam * onehot(target) + (1 - lam) * onehot(target_b)) + label_smoothing / C`` is
    formed inside the kernels; ``target_threshold`` in [0, 1) binarises it (``y > target_threshold``).
    The loss is the mean over all ``B * C`` elements (torch's and timm's default), or with ``sum_classes`` the
    sum over the classes and the mean over the batch. A float target of the logits' shape (multi-label) is
    accepted and takes the PyTorch composition.

    timm spells the first argument ``smoothing=0.1``; here it is ``label_smoothing``, as in
    :class:`CrossEntropyLoss`. Not offered: ``pos_weight``, per-class ``weight``, ``reduction='none'/'sum'``.
    """

    def __init__(self, label_smoothing: float = 0.0, target_threshold=None, sum_classes: bool = False):
        super().__init__()
        if not 0.0 <= label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be between 0.0 and 1.0. Got: {label_smoothing}")
        if target_threshold is not None and not 0.0 <= target_threshold < 1.0:
            raise ValueError(f"target_threshold must be in [0.0, 1.0). Got: {target_threshold}")
        self.label_smoothing = float(label_smoothing)
        self.target_threshold = None if target_threshold is None else float(target_threshold)
        self.sum_classes = bool(sum_classes)

    def forward(self, logits, target):
        from ..data import MixTarget

        if isinstance(target, MixTarget):
            return CF.binary_cross_entropy(logits, target.target, self.label_smoothing, self.target_threshold,
                                           self.sum_classes, target_b=target.target_b, lam=target.lam)
        if target.is_floating_point():  # dense targets carry their own smoothing
            return CF.binary_cross_entropy(logits, target, 0.0, self.target_threshold, self.sum_classes)
        return CF.binary_cross_entropy(logits, target, self.label_smoothing, self.target_threshold, self.sum_classes)

    def extra_repr(self):
        return (f"label_smoothing={self.label_smoothing}, target_threshold={self.target_threshold}, "
                f"sum_classes={self.sum_classes}")
