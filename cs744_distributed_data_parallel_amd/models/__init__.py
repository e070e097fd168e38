"""Model zoo: the reference's VGG family (CIFAR-shaped) and the ResNet and MobileNetV1 families (ImageNet-shaped)."""
from .mobilenet import MobileNetV1, mobilenet_v1, mobilenet_v1_025, mobilenet_v1_050, mobilenet_v1_075
from .resnet import (ResNet, SEModule, resnet18, resnet18_gn, resnet34, resnet34_gn, resnet50, resnet50_gn, resnet101,
                     resnet101_gn, resnet152, resnet152_gn, seresnet18, seresnet34, seresnet50, seresnet101,
                     seresnet152, resnext50_32x4d, resnext101_32x8d, resnext101_64x4d, seresnext50_32x4d,
                     wide_resnet50_2, wide_resnet101_2)
from .vgg import VGG, VGG11, VGG13, VGG16, VGG19, cfg, make_layers

_REGISTRY = {
    "vgg11": VGG11,
    "vgg13": VGG13,
    "vgg16": VGG16,
    "vgg19": VGG19,
    "resnet18": resnet18,
    "resnet34": resnet34,
    "resnet50": resnet50,
    "resnet101": resnet101,
    "resnet152": resnet152,
    "seresnet18": seresnet18,
    "seresnet34": seresnet34,
    "seresnet50": seresnet50,
    "seresnet101": seresnet101,
    "seresnet152": seresnet152,
    # GroupNorm in place of every BatchNorm ("resnet50_gn": get_model strips "_" and "-")
    "resnet18gn": resnet18_gn,
    "resnet34gn": resnet34_gn,
    "resnet50gn": resnet50_gn,
    "resnet101gn": resnet101_gn,
    "resnet152gn": resnet152_gn,
}
# the Squeeze-and-Excitation models under their "resnetNN_se" spelling too (get_model strips "_" and "-")
_REGISTRY.update({"resnet" + k[len("seresnet"):] + "se": v for k, v in list(_REGISTRY.items()) if k.startswith("seresnet")})
# cardinality and width: a grouped 3x3 conv2 (ResNeXt) or a doubled one (Wide ResNet) in every Bottleneck
_REGISTRY.update({
    "resnext5032x4d": resnext50_32x4d,
    "resnext10132x8d": resnext101_32x8d,
    "resnext10164x4d": resnext101_64x4d,
    "seresnext5032x4d": seresnext50_32x4d,
    "wideresnet502": wide_resnet50_2,
    "wideresnet1012": wide_resnet101_2,
})
# depthwise-separable: MobileNetV1 at width multipliers 1, 0.75, 0.5 and 0.25 ("mobilenet_v1_050" and
# "mobilenetv1_050" are one key: get_model strips "_" and "-")
_REGISTRY.update({
    "mobilenetv1": mobilenet_v1,
    "mobilenetv1075": mobilenet_v1_075,
    "mobilenetv1050": mobilenet_v1_050,
    "mobilenetv1025": mobilenet_v1_025,
})

# input shape (C, H, W) and number of classes per family
INPUT_SHAPES = {k: ((3, 32, 32), 10) if k.startswith("vgg") else ((3, 224, 224), 1000) for k in _REGISTRY}


def get_model(name: str, **kw):
    key = name.lower().replace("-", "").replace("_", "")
    if key not in _REGISTRY:
        raise ValueError(f"unknown model {name!r}; choose from {sorted(_REGISTRY)}")
    return _REGISTRY[key](**kw)


def list_models():
    return sorted(_REGISTRY)


__all__ = [
    "VGG", "VGG11", "VGG13", "VGG16", "VGG19", "cfg", "make_layers",
    "ResNet", "resnet18", "resnet34", "resnet50", "resnet101", "resnet152",
    "resnet18_gn", "resnet34_gn", "resnet50_gn", "resnet101_gn", "resnet152_gn",
    "SEModule", "seresnet18", "seresnet34", "seresnet50", "seresnet101", "seresnet152",
    "resnext50_32x4d", "resnext101_32x8d", "resnext101_64x4d", "seresnext50_32x4d", "wide_resnet50_2",
    "wide_resnet101_2",
    "MobileNetV1", "mobilenet_v1", "mobilenet_v1_075", "mobilenet_v1_050", "mobilenet_v1_025",
    "get_model", "list_models", "INPUT_SHAPES",
]
