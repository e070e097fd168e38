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
