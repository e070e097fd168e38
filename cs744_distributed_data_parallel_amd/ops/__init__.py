"""Fused, autograd-visible ops on the gfx950 kernels (see :mod:`.functional`)."""
from . import functional
from .functional import binary_cross_entropy, conv_bn_act, count_correct, cross_entropy, global_avg_pool, linear, max_pool2d, use_native
from .modules import BinaryCrossEntropy, CrossEntropyLoss

__all__ = [
    "functional", "conv_bn_act", "count_correct", "cross_entropy", "global_avg_pool", "linear", "max_pool2d",
    "use_native", "CrossEntropyLoss", "binary_cross_entropy", "BinaryCrossEntropy",
]
