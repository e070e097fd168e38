"""MobileNetV1 (Howard et al., "MobileNets", Table 1) for 3x224x224 inputs / 1000 classes.

A 3x3 / stride-2 stem of 32 channels, then 13 depthwise-separable blocks ``dw3x3 -> BN -> ReLU -> pw1x1 -> BN ->
ReLU`` (widths 64, 128, 128, 256, 256, 512 x 6, 1024, 1024; strides 1, 2, 1, 2, 1, 2, 1 x 5, 2, 1), a global
average pool and ``fc``. The activation is the plain ReLU of the paper's text (not ReLU6); every conv is
``bias=False``. ``width_mult`` scales every width to ``make_divisible(c * width_mult, 8)``; ``small_input`` makes
the stem stride 1 for 32 x 32 inputs. Parameters: ``stem.0`` / ``stem.1``, ``blocks.{i}.dw`` / ``.bn1`` / ``.pw`` /
``.bn2``, ``fc``.

MI355X execution: every layer is one fused ``conv_bn_act`` on NHWC activations -- the depthwise convs on the direct
fp32 kernels of csrc/kernels/dwconv.hip, the 1x1 pointwise convs and the RGB stem on the dense conv GEMMs -- then
``global_avg_pool`` and ``linear``. On CPU tensors the plain modules run (reference semantics).
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import functional as CF
from ..utils.arena import install_load_hooks

# (output channels, stride of the depthwise conv) of the 13 blocks at width_mult = 1
BLOCKS = [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1), (512, 1), (512, 1),
          (512, 1), (1024, 2), (1024, 1)]


def make_divisible(v: float, divisor: int = 8) -> int:
    """``v`` rounded to a multiple of ``divisor`` (at least one), raised by one step below 90 % of ``v``."""
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    if new < 0.9 * v:
        new += divisor
    return new


class DepthwiseSeparable(nn.Module):
    def __init__(self, inp: int, out: int, stride: int):
        super().__init__()
        self.dw = nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False)
        self.bn1 = nn.BatchNorm2d(inp)
        self.pw = nn.Conv2d(inp, out, 1, 1, 0, bias=False)
        self.bn2 = nn.BatchNorm2d(out)

    def forward(self, x):
        # (CF.conv_bn_act is the plain module composition on CPU tensors)
        x = CF.conv_bn_act(x, self.dw, self.bn1, relu=True)
        return CF.conv_bn_act(x, self.pw, self.bn2, relu=True)


class MobileNetV1(nn.Module):
    def __init__(self, num_classes: int = 1000, width_mult: float = 1.0, small_input: bool = False,
                 channels_last: bool = True):
        super().__init__()
        if not float(width_mult) > 0.0:
            raise ValueError(f"width_mult must be positive. Got: {width_mult}")
        install_load_hooks(self)  # loaded weights refresh the optimizer's prepared products
        c = make_divisible(32 * width_mult)
        self.stem = nn.Sequential(nn.Conv2d(3, c, 3, 1 if small_input else 2, 1, bias=False), nn.BatchNorm2d(c),
                                  nn.ReLU(inplace=True))
        blocks = []
        for out, stride in BLOCKS:
            out = make_divisible(out * width_mult)
            blocks.append(DepthwiseSeparable(c, out, stride))
            c = out
        self.blocks = nn.Sequential(*blocks)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(c, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if channels_last:
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)

    def forward(self, x):
        if CF.use_native(x):
            x = x.contiguous(memory_format=torch.channels_last)
            # one launch: the dense convs' f16x2 operand scales and their W^T for the data gradients (the stem's
            # input needs no gradient). A depthwise weight feeds no GEMM: the direct kernels read it unscaled and
            # untransposed, so it is left out of the list and of the optimizer's fused weight preparation that
            # follows it, as a grouped weight is (ResNet._forward)
            convs = [m for m in self.modules() if isinstance(m, nn.Conv2d) and m.groups == 1]
            need = [m.stride[0] == 1 and (m is not self.stem[0] or x.requires_grad) for m in convs]
            wam, wts = CF.weight_prep([m.weight for m in convs], need)
            for i, m in enumerate(convs):
                m._cdp_wamax = wam[i] if wam is not None else None
                m._cdp_wt = wts[i] if wts is not None else None
            try:
                x = CF.conv_bn_act(x, self.stem[0], self.stem[1], relu=True)
                x = self.blocks(x)
            finally:
                for m in convs:
                    m._cdp_wamax = None
                    m._cdp_wt = None
            x = CF.global_avg_pool(x)
            return CF.linear(x, self.fc.weight, self.fc.bias)
        x = self.blocks(self.stem(x))
        return self.fc(torch.flatten(self.avgpool(x), 1))


def mobilenet_v1(**kw):
    return MobileNetV1(**kw)


def mobilenet_v1_075(**kw):
    return MobileNetV1(width_mult=0.75, **kw)


def mobilenet_v1_050(**kw):
    return MobileNetV1(width_mult=0.5, **kw)


def mobilenet_v1_025(**kw):
    return MobileNetV1(width_mult=0.25, **kw)
