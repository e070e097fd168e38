"""ResNet family (ResNet-18/34/50/101/152) for ImageNet-shaped inputs.

This is the ``BASELINE.json`` config #5 model ("ResNet-50 ImageNet-shaped synthetic, bucketed DDP
on 8xMI355X -- larger-model bucket-sizing stress"): 25.6M parameters in 161 tensors, so the
bucketed reducer sees many more, and much more unevenly sized, gradients than VGG-11's 34.
The module tree (``conv1/bn1/layer1..4/fc``, ``downsample.0/1``) and default initialisation follow
the torchvision layout so checkpoints are interchangeable.

MI355X execution: every ``conv -> BN [-> +residual] [-> ReLU]`` is one fused autograd op
(implicit-GEMM MFMA conv, BN statistics fused into the conv epilogue, BN-apply + residual + ReLU in
one NHWC pass); 1x1 convs are plain GEMMs through the same kernel; strided 3x3 / 1x1 convs use the
strided gather (forward) and the divisibility-masked transposed gather (data gradient).

Stochastic depth (``drop_path_rate``): block ``i`` of ``L`` drops its branch for an image with probability
``drop_path_rate * i / (L - 1)`` and scales the kept ones by ``1 / (1 - p)``, per image (timm ``drop_path``,
torchvision ``StochasticDepth(mode="row")``). The scale is applied inside the block's last fused
``conv -> BN -> +residual -> ReLU`` (``conv_bn_act(..., drop_scale=)``); the draws of a step are one device
launch keyed by a device step counter (csrc/kernels/drop_path.h), so a captured step drops different images
at every replay.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn

from .. import _native
from ..ops import functional as CF
from ..ops.functional import drop_path_scales
from ..utils.arena import install_load_hooks

# CDP_DEFER_DS=0: materialize the downsample branch's BatchNorm output (A/B)
_DEFER_DS = os.environ.get("CDP_DEFER_DS", "1") != "0"


class BasicBlock(nn.Module):
    expansion = 1
    _drop_scale = None

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        ds = self._drop_scale  # this forward's stochastic-depth row (ResNet.forward), or None
        if CF.use_native(x):
            sink = CF.GradSink.make(x)
            out = CF.conv_bn_act(x, self.conv1, self.bn1, relu=True, dx_sink=sink)
            if self.downsample is None:
                return CF.conv_bn_act(out, self.conv2, self.bn2, relu=True, residual=x, res_sink=sink,
                                      drop_scale=ds)
            # the downsample's BatchNorm is applied inside conv2's residual add (defer_apply)
            idt = CF.conv_bn_act(x, self.downsample[0], self.downsample[1], relu=False, dx_sink=sink,
                                 defer_apply=_DEFER_DS)
            return CF.conv_bn_act(out, self.conv2, self.bn2, relu=True, residual=idt, drop_scale=ds)
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        if ds is not None:
            out = out * ds.to(out.dtype).view(-1, 1, 1, 1)
        return self.relu(out + idt)


class Bottleneck(nn.Module):
    expansion = 4
    _drop_scale = None

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        width = planes
        self.conv1 = nn.Conv2d(inplanes, width, 1, 1, 0, bias=False)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, planes * 4, 1, 1, 0, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        ds = self._drop_scale  # this forward's stochastic-depth row (ResNet.forward), or None
        if CF.use_native(x):
            # x's two gradients (conv1 + residual, or conv1 + downsample) are summed inside a
            # data-gradient GEMM epilogue instead of an autograd add (GradSink)
            sink = CF.GradSink.make(x)
            out = CF.conv_bn_act(x, self.conv1, self.bn1, relu=True, dx_sink=sink)
            out = CF.conv_bn_act(out, self.conv2, self.bn2, relu=True)
            if self.downsample is None:
                return CF.conv_bn_act(out, self.conv3, self.bn3, relu=True, residual=x, res_sink=sink,
                                      drop_scale=ds)
            # the downsample's BatchNorm is applied inside conv3's residual add (defer_apply)
            idt = CF.conv_bn_act(x, self.downsample[0], self.downsample[1], relu=False, dx_sink=sink,
                                 defer_apply=_DEFER_DS)
            return CF.conv_bn_act(out, self.conv3, self.bn3, relu=True, residual=idt, drop_scale=ds)
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        if ds is not None:
            out = out * ds.to(out.dtype).view(-1, 1, 1, 1)
        return self.relu(out + idt)


class ResNet(nn.Module):
    """``drop_path_rate`` in ``[0, 1)``: stochastic depth at timm's linear per-block rates (``drop_path_rates``),
    drawn on the device from ``drop_path_seed`` and the step counter ``drop_path_step`` (one per training
    forward; ``last_drop_scales`` keeps the last ``[nb, B]`` table, ``nb`` the blocks with a rate above 0).
    The rates, the counter and the table are plain attributes (the ``state_dict()`` keys stay torchvision's)
    that follow the module through ``.cuda()`` / ``.to()``. At 0.0 nothing is allocated or launched and
    ``drop_path_step`` is None. ``zero_init_residual``: every block's last BatchNorm weight starts at 0
    (torchvision's rule), so every block starts as its shortcut."""

    def __init__(self, block, layers, num_classes=1000, channels_last=True, drop_path_rate=0.0, drop_path_seed=0,
                 zero_init_residual=False):
        super().__init__()
        if not 0.0 <= float(drop_path_rate) < 1.0:
            raise ValueError(f"drop_path_rate must be in [0, 1). Got: {drop_path_rate}")
        install_load_hooks(self)  # loaded weights refresh the optimizer's prepared products
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)
                elif isinstance(m, BasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)
        if channels_last:
            for m in self.modules():
                if isinstance(m, nn.Conv2d):
                    m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        # stochastic depth: block i of L in network order drops at drop_path_rate * i / (L - 1)
        self._dp_blocks = [m for m in self.modules() if isinstance(m, (BasicBlock, Bottleneck))]
        L = len(self._dp_blocks)
        self.drop_path_seed = int(drop_path_seed)
        self.drop_path_rates = [float(drop_path_rate) * i / max(L - 1, 1) for i in range(L)]
        self._dp_active = [i for i, p in enumerate(self.drop_path_rates) if p > 0.0]  # the table's rows
        self._dp_rates = self._dp_counter = self.last_drop_scales = None
        if self._dp_active:
            self._dp_rates = torch.tensor([self.drop_path_rates[i] for i in self._dp_active], dtype=torch.float32)
            self._dp_counter = torch.zeros(1, dtype=torch.int64)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self._dp_counter is not None:  # plain attributes: follow the parameters' device (dtypes stay)
            self._dp_counter = fn(self._dp_counter).to(torch.int64)
            self._dp_rates = fn(self._dp_rates).to(torch.float32)
            if self.last_drop_scales is not None:
                self.last_drop_scales = fn(self.last_drop_scales).to(torch.float32)
        return self

    @property
    def drop_path_step(self):
        """The step counter of the next training forward's draws (a 0-dim view; None at rate 0)."""
        return None if self._dp_counter is None else self._dp_counter[0]

    def set_drop_path_step(self, t: int) -> None:
        if self._dp_counter is None:
            raise ValueError("set_drop_path_step: this model has drop_path_rate = 0 and no counter")
        if self._dp_counter.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("set_drop_path_step: not while a stream is capturing (a replay would not see it)")
        self._dp_counter.fill_(int(t))

    def drop_path_schedule(self, first: int, n: int, B: int) -> torch.Tensor:
        """float32 ``[n, nb, B]``: the tables of step counters ``first .. first + n - 1``."""
        if self._dp_counter is None:
            raise ValueError("drop_path_schedule: this model has drop_path_rate = 0 and draws nothing")
        if CF.use_native(self._dp_counter):
            return _native.lib().drop_path_table(self.drop_path_seed, int(first), int(n), self._dp_rates, int(B))
        rates = [self.drop_path_rates[i] for i in self._dp_active]
        rows = [drop_path_scales(self.drop_path_seed, int(first) + t, rates, int(B)) for t in range(int(n))]
        out = torch.stack(rows) if rows else torch.empty(0, len(rates), int(B))
        return out.to(self._dp_counter.device)

    def _draw_drop_scales(self, x):
        """One training forward's ``[nb, B]`` table; advances the counter by one."""
        B = x.shape[0]
        if CF.use_native(x):  # one launch: the table of the counter's step, then counter += 1
            return _native.lib().drop_path_draw(self._dp_counter, self.drop_path_seed, self._dp_rates, B)
        rates = [self.drop_path_rates[i] for i in self._dp_active]
        t = drop_path_scales(self.drop_path_seed, int(self._dp_counter.item()), rates, B).to(x.device)
        self._dp_counter += 1
        return t

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, 1, stride, 0, bias=False),
                nn.BatchNorm2d(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    def forward(self, x):
        if self._dp_counter is None or not self.training:
            return self._forward(x)
        # stochastic depth: this step's table (drawn before the stem), row k to the k-th block with a rate
        table = self._draw_drop_scales(x)
        self.last_drop_scales = table
        try:
            for k, i in enumerate(self._dp_active):
                self._dp_blocks[i]._drop_scale = table[k]
            return self._forward(x)
        finally:
            for i in self._dp_active:
                self._dp_blocks[i]._drop_scale = None

    def _forward(self, x):
        if CF.use_native(x):
            x = x.contiguous(memory_format=torch.channels_last)
            # one launch: every conv weight's f16x2 operand scale and its W^T for the data gradient
            # (stride-1 convs; the stem's input needs no gradient, stride-2 convs use sub-filters);
            # each conv module holds its entries for the duration of this forward (conv_bn_act
            # reads them)
            convs = [m for m in self.modules() if isinstance(m, nn.Conv2d)]
            need = [m.stride[0] == 1 and (m is not self.conv1 or x.requires_grad) for m in convs]
            wam, wts = CF.weight_prep([m.weight for m in convs], need)
            for i, m in enumerate(convs):
                m._cdp_wamax = wam[i] if wam is not None else None
                m._cdp_wt = wts[i] if wts is not None else None
            try:
                x = CF.conv_bn_act(x, self.conv1, self.bn1, relu=True)
                x = CF.max_pool2d(x, 3, 2, 1)
                x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
            finally:
                for m in convs:
                    m._cdp_wamax = None
                    m._cdp_wt = None
            x = CF.global_avg_pool(x)
            return CF.linear(x, self.fc.weight, self.fc.bias)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        x = torch.flatten(self.avgpool(x), 1)
        return self.fc(x)


def resnet18(**kw):
    return ResNet(BasicBlock, [2, 2, 2, 2], **kw)


def resnet34(**kw):
    return ResNet(BasicBlock, [3, 4, 6, 3], **kw)


def resnet50(**kw):
    return ResNet(Bottleneck, [3, 4, 6, 3], **kw)


def resnet101(**kw):
    return ResNet(Bottleneck, [3, 4, 23, 3], **kw)


def resnet152(**kw):
    return ResNet(Bottleneck, [3, 8, 36, 3], **kw)
