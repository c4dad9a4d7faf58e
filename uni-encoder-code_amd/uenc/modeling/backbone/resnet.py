"""ResNet backbone on HIP kernels -- drop-in for the reference's `build_custom_resnet_backbone` (model/modeling/backbone/resnet.py).

Same class names, constructor arguments, parameter and buffer names (`stem.conv1.weight`, `stem.conv1.norm.{weight, bias, running_mean,
running_var, num_batches_tracked}`, `res2.0.conv1...`, `res3.0.shortcut...`), the same `forward(x) -> {"stem", "res2" .. "res5"}` contract
and `MODEL.RESNETS.*` / `MODEL.BACKBONE.FREEZE_AT` keys, registered in `BACKBONE_REGISTRY`.

Maps are channels-last (B, H, W, C).  Every convolution with its norm, the shortcut add and the ReLU that follow it is one autograd
node (`ops.ConvBnActFn`): the 7x7 stride-2 stem is a patch gather (csrc/resnet.hip) + MFMA GEMM, 3x3 convolutions are the patch-gather
GEMMs of the FPN / DiNAT paths, 1x1 convolutions plain GEMMs; BatchNorm statistics, the affine + residual + ReLU pass and its backward
are the kernels of csrc/resnet.hip.  A convolution's result stays fp32 up to its BatchNorm; a block's output (the residual stream) is
fp32, the maps inside a block are in the GEMM operand dtype.  `train()` normalises with batch statistics and updates the running ones
on the device, `eval()` and FrozenBatchNorm2d use the running ones.  Channel counts must be multiples of 8 (every stock width is).

Not built (each raises NotImplementedError naming its key): deformable blocks (DEFORM_ON_PER_STAGE), RES5_DILATION 2, NUM_GROUPS > 1,
a classification head (num_classes), and SyncBN statistics across more than one rank in training.
"""
import torch
import torch.nn as nn

from ... import ops
from ...d2 import BACKBONE_REGISTRY, Backbone, CNNBlockBase, Conv2d, ShapeSpec, get_norm

__all__ = ["ResNetBlockBase", "BasicBlock", "BottleneckBlock", "DeformBottleneckBlock", "BasicStem", "ResNet", "make_stage",
           "build_custom_resnet_backbone"]


def _world_size() -> int:
    dist = torch.distributed
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _conv_norm(conv, x, *, kind, residual=None, relu=False, out_dtype=ops.F32):
    """One Conv2d-with-norm holder (d2.Conv2d: weight, .norm) applied as a single fused node."""
    bn = conv.norm
    if bn is None or not hasattr(bn, "running_mean"):
        raise NotImplementedError(f"ResNet convolutions run with a BatchNorm (MODEL.RESNETS.NORM 'BN', 'SyncBN' or 'FrozenBN'), got {bn!r}")
    train = bn.training and isinstance(bn, nn.modules.batchnorm._BatchNorm)
    if train and isinstance(bn, nn.SyncBatchNorm) and _world_size() > 1:
        raise NotImplementedError("MODEL.RESNETS.NORM 'SyncBN' in training on more than one rank: the all-reduce of the batch statistics "
                                  "is a follow-up; use 'BN' or 'FrozenBN', or one rank")
    return ops.conv_bn_act(x, conv.weight, bn, kind=kind, stride=conv.stride[0], residual=residual, relu=relu, train=train,
                           out_dtype=out_dtype)


class BasicBlock(CNNBlockBase):
    """Two 3x3 convolutions and a projection shortcut where the channel count changes (ResNet-18 / 34)."""

    def __init__(self, in_channels, out_channels, *, stride=1, norm="BN"):
        super().__init__(in_channels, out_channels, stride)
        self.shortcut = None
        if in_channels != out_channels:
            self.shortcut = Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False, norm=get_norm(norm, out_channels))
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=3, stride=stride, padding=1, bias=False, norm=get_norm(norm, out_channels))
        self.conv2 = Conv2d(out_channels, out_channels, kernel_size=3, stride=1, padding=1, bias=False, norm=get_norm(norm, out_channels))
        for layer in (self.conv1, self.conv2, self.shortcut):
            if layer is not None:
                nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        """x (B, H, W, Cin) fp32 channels-last -> (B, Ho, Wo, Cout) fp32."""
        out = _conv_norm(self.conv1, x, kind=3, relu=True, out_dtype=ops.BF16)
        shortcut = x if self.shortcut is None else _conv_norm(self.shortcut, x, kind=1)
        return _conv_norm(self.conv2, out, kind=3, residual=shortcut, relu=True)


class BottleneckBlock(CNNBlockBase):
    """1x1 -> 3x3 -> 1x1 convolutions and a projection shortcut where the channel count changes (ResNet-50 / 101 / 152)."""

    def __init__(self, in_channels, out_channels, *, bottleneck_channels, stride=1, num_groups=1, norm="BN", stride_in_1x1=False, dilation=1):
        super().__init__(in_channels, out_channels, stride)
        if num_groups != 1:
            raise NotImplementedError(f"MODEL.RESNETS.NUM_GROUPS > 1 (grouped 3x3 convolutions) is not built (got {num_groups})")
        if dilation != 1:
            raise NotImplementedError(f"MODEL.RESNETS.RES5_DILATION 2 (dilated 3x3 convolutions) is not built (got dilation {dilation})")
        self.shortcut = None
        if in_channels != out_channels:
            self.shortcut = Conv2d(in_channels, out_channels, kernel_size=1, stride=stride, bias=False, norm=get_norm(norm, out_channels))
        stride_1x1, stride_3x3 = (stride, 1) if stride_in_1x1 else (1, stride)
        self.conv1 = Conv2d(in_channels, bottleneck_channels, kernel_size=1, stride=stride_1x1, bias=False,
                            norm=get_norm(norm, bottleneck_channels))
        self.conv2 = Conv2d(bottleneck_channels, bottleneck_channels, kernel_size=3, stride=stride_3x3, padding=1, bias=False,
                            norm=get_norm(norm, bottleneck_channels))
        self.conv3 = Conv2d(bottleneck_channels, out_channels, kernel_size=1, bias=False, norm=get_norm(norm, out_channels))
        for layer in (self.conv1, self.conv2, self.conv3, self.shortcut):
            if layer is not None:
                nn.init.kaiming_normal_(layer.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        out = _conv_norm(self.conv1, x, kind=1, relu=True, out_dtype=ops.BF16)
        out = _conv_norm(self.conv2, out, kind=3, relu=True, out_dtype=ops.BF16)
        shortcut = x if self.shortcut is None else _conv_norm(self.shortcut, x, kind=1)
        return _conv_norm(self.conv3, out, kind=1, residual=shortcut, relu=True)


class DeformBottleneckBlock(CNNBlockBase):
    """The deformable-convolution bottleneck of the reference: not built."""

    def __init__(self, in_channels, out_channels, **kwargs):
        raise NotImplementedError("MODEL.RESNETS.DEFORM_ON_PER_STAGE: DeformBottleneckBlock (deformable 3x3 convolutions) is not built")


class BasicStem(CNNBlockBase):
    """7x7 stride-2 convolution + norm + ReLU on the image; the max pooling that follows belongs to ResNet.forward."""

    def __init__(self, in_channels=3, out_channels=64, norm="BN"):
        super().__init__(in_channels, out_channels, 2)
        self.in_channels = in_channels
        self.conv1 = Conv2d(in_channels, out_channels, kernel_size=7, stride=2, padding=3, bias=False, norm=get_norm(norm, out_channels))
        nn.init.kaiming_normal_(self.conv1.weight, mode="fan_out", nonlinearity="relu")

    def forward(self, x):
        """x (B, 3, H, W) fp32 image -> (B, Ho, Wo, C) fp32 channels-last."""
        if x.shape[1] != 3:
            raise ValueError(f"BasicStem: the HIP patch gather takes 3-channel images, got {x.shape[1]} channels")
        return _conv_norm(self.conv1, x, kind="stem", relu=True)


class ResNet(Backbone):
    """stem -> max pooling -> up to four stages `res2` .. `res5` (child modules of those names, each an nn.Sequential of blocks).
    Attributes the callers of the reference rely on: `stem`, `stages`, `stage_names`, `num_classes`, `_out_features`,
    `_out_feature_channels`, `_out_feature_strides`."""

    _STAGE_OF = ("res2", "res3", "res4", "res5")

    def __init__(self, stem, stages, num_classes=None, out_features=None, freeze_at=0):
        super().__init__()
        if num_classes is not None:
            raise NotImplementedError("ResNet(num_classes=...): the classification head (avgpool + linear) is not built")
        self.stem, self.num_classes = stem, None
        if out_features is not None:
            # stages behind the deepest requested feature would hold parameters that never get a gradient: they are not kept
            deepest = max((self._STAGE_OF.index(f) + 1 for f in out_features if f in self._STAGE_OF), default=0)
            stages = stages[:deepest]
        self._out_feature_channels = {"stem": stem.out_channels}
        self._out_feature_strides = {"stem": stem.stride}
        stride = 2 * stem.stride                                # the pooling between the stem and res2 halves the map once more
        self.stages = []
        for name, blocks in zip(self._STAGE_OF, stages):
            if len(blocks) == 0 or not all(isinstance(b, CNNBlockBase) for b in blocks):
                raise ValueError(f"ResNet: stage {name} must be a non-empty list of CNNBlockBase blocks, got {blocks!r}")
            for b in blocks:
                stride *= b.stride
            self.add_module(name, nn.Sequential(*blocks))
            self.stages.append(getattr(self, name))
            self._out_feature_channels[name], self._out_feature_strides[name] = blocks[-1].out_channels, int(stride)
        self.stage_names = self._STAGE_OF[:len(self.stages)]
        self._out_features = list(out_features) if out_features is not None else [(("stem",) + self.stage_names)[-1]]
        unknown = [f for f in self._out_features if f not in self._out_feature_channels]
        if unknown or not self._out_features:
            raise ValueError(f"ResNet: out_features {self._out_features} must be a non-empty subset of {list(self._out_feature_channels)}")
        self.freeze(freeze_at)

    def forward(self, x):
        """x (N, 3, H, W) fp32 -> {name: (N, C, H', W')-shaped fp32 view of the channels-last map}."""
        if x.dim() != 4:
            raise ValueError(f"ResNet: the input must be an (N, C, H, W) image batch, got shape {tuple(x.shape)}")
        outputs = {}
        x = self.stem(x)
        if "stem" in self._out_features:
            outputs["stem"] = x.permute(0, 3, 1, 2)
        x = ops.max_pool3x3_s2(x)
        for name, stage in zip(self.stage_names, self.stages):
            x = stage(x)
            if name in self._out_features:
                outputs[name] = x.permute(0, 3, 1, 2)
        return outputs

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}

    def freeze(self, freeze_at=0):
        """Freeze the first `freeze_at` levels, counting the stem as level 1 and `res{k}` as level k: their parameters stop requiring a
        gradient and their BatchNorms become FrozenBatchNorm2d (each block's `freeze()`).  Returns self."""
        levels = [[self.stem]] + [list(stage) for stage in self.stages]
        for blocks in levels[:max(0, freeze_at)]:
            for block in blocks:
                block.freeze()
        return self

    @staticmethod
    def make_stage(block_class, num_blocks, *, in_channels, out_channels, **kwargs):
        """`num_blocks` blocks of `block_class`, the first taking `in_channels`, all giving `out_channels`.  A keyword `xx_per_block` is a
        list holding block i's value of the constructor argument `xx`; every other keyword goes to each block unchanged."""
        suffix = "_per_block"
        shared = {k: v for k, v in kwargs.items() if not k.endswith(suffix)}
        listed = {k[:-len(suffix)]: v for k, v in kwargs.items() if k.endswith(suffix)}
        for k, v in listed.items():
            if len(v) != num_blocks:
                raise ValueError(f"make_stage: {k}{suffix} has {len(v)} entries for {num_blocks} blocks")
            if k in shared:
                raise ValueError(f"make_stage: give either {k} or {k}{suffix}, not both")
        widths = [in_channels] + [out_channels] * (num_blocks - 1)
        return [block_class(in_channels=w, out_channels=out_channels, **shared, **{k: v[i] for k, v in listed.items()})
                for i, w in enumerate(widths)]

    @staticmethod
    def make_default_stages(depth, block_class=None, **kwargs):
        """The four stages of a stock depth (18, 34, 50, 101, 152): BasicBlock widths 64 .. 512 below 50, BottleneckBlock widths 256 .. 2048
        with a quarter of that in the bottleneck from 50 on; res3 .. res5 start with a stride-2 block.  `kwargs` go to every block."""
        deep = depth >= 50
        cls = block_class or (BottleneckBlock if deep else BasicBlock)
        stages, width_in = [], 64
        for level, count in enumerate(_BLOCKS_PER_STAGE[depth]):
            width_out = (256 if deep else 64) << level
            extra = dict(kwargs, bottleneck_channels=width_out // 4) if deep else dict(kwargs)
            stages.append(ResNet.make_stage(cls, count, in_channels=width_in, out_channels=width_out,
                                            stride_per_block=[1 if level == 0 else 2] + [1] * (count - 1), **extra))
            width_in = width_out
        return stages


_BLOCKS_PER_STAGE = {18: [2, 2, 2, 2], 34: [3, 4, 6, 3], 50: [3, 4, 6, 3], 101: [3, 4, 23, 3], 152: [3, 8, 36, 3]}

ResNetBlockBase = CNNBlockBase


def make_stage(*args, **kwargs):
    return ResNet.make_stage(*args, **kwargs)


@BACKBONE_REGISTRY.register()
def build_custom_resnet_backbone(cfg, input_shape):
    """A ResNet from `cfg.MODEL.RESNETS.*` and `cfg.MODEL.BACKBONE.FREEZE_AT`: DEPTH picks the block class and counts, STEM_OUT_CHANNELS and
    RES2_OUT_CHANNELS the first widths (doubling per stage, as does the bottleneck width NUM_GROUPS * WIDTH_PER_GROUP)."""
    r = cfg.MODEL.RESNETS
    # detectron2's DEFORM_* defaults are not among this shim's keys (tests/golden/cfg_cityscapes_swin_t.json pins the key set): absent = off
    if any(r.get("DEFORM_ON_PER_STAGE", [False] * 4)):
        raise NotImplementedError("MODEL.RESNETS.DEFORM_ON_PER_STAGE: DeformBottleneckBlock (deformable 3x3 convolutions) is not built")
    if r.RES5_DILATION not in (1, 2):
        raise ValueError(f"MODEL.RESNETS.RES5_DILATION must be 1 or 2, got {r.RES5_DILATION}")
    if r.RES5_DILATION == 2:
        raise NotImplementedError("MODEL.RESNETS.RES5_DILATION 2 (dilated res5) is not built")
    if r.NUM_GROUPS != 1:
        raise NotImplementedError(f"MODEL.RESNETS.NUM_GROUPS > 1 (grouped 3x3 convolutions) is not built (got {r.NUM_GROUPS})")
    if r.DEPTH not in _BLOCKS_PER_STAGE:
        raise ValueError(f"MODEL.RESNETS.DEPTH must be one of {sorted(_BLOCKS_PER_STAGE)}, got {r.DEPTH}")
    basic = r.DEPTH < 50
    if basic and r.RES2_OUT_CHANNELS != 64:
        raise ValueError(f"MODEL.RESNETS.RES2_OUT_CHANNELS must be 64 for R18 / R34 (BasicBlock has no bottleneck), got {r.RES2_OUT_CHANNELS}")
    block_kw = {"norm": r.NORM} if basic else {"norm": r.NORM, "stride_in_1x1": r.STRIDE_IN_1X1, "num_groups": r.NUM_GROUPS, "dilation": 1}
    stages, width_in = [], r.STEM_OUT_CHANNELS
    for level, count in enumerate(_BLOCKS_PER_STAGE[r.DEPTH]):
        width_out = r.RES2_OUT_CHANNELS << level
        if not basic:
            block_kw["bottleneck_channels"] = (r.NUM_GROUPS * r.WIDTH_PER_GROUP) << level
        stages.append(ResNet.make_stage(BasicBlock if basic else BottleneckBlock, count, in_channels=width_in, out_channels=width_out,
                                        stride_per_block=[1 if level == 0 else 2] + [1] * (count - 1), **block_kw))
        width_in = width_out
    stem = BasicStem(in_channels=input_shape.channels, out_channels=r.STEM_OUT_CHANNELS, norm=r.NORM)
    return ResNet(stem, stages, out_features=r.OUT_FEATURES, freeze_at=cfg.MODEL.BACKBONE.FREEZE_AT)
