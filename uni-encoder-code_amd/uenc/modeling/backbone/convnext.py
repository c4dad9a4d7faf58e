"""ConvNeXt backbone on HIP kernels -- drop-in for the reference's `D2ConvNeXt` (model/modeling/backbone/convnext.py).

Same class names, constructor arguments, parameter names and shapes (`downsample_layers.{0..3}.{0,1}`, `stages.{i}.{j}.{dwconv,norm,
pwconv1,pwconv2}`, `stages.{i}.{j}.gamma`, `norm{0..3}`), the same `forward(x) -> {"res2".."res5"}` contract, registered as `D2ConvNeXt`
in `BACKBONE_REGISTRY` with `cfg.MODEL.CONVNEXT.*` (config.add_convnext_config).

The residual stream is an fp32 channels-last map (B, H, W, C), as in the DiNAT path.  A Block is one autograd Function
(`ops.ConvNeXtBlockFn`): the fused 7x7 depthwise convolution + LayerNorm kernel (csrc/dwconv.hip), the bf16 MFMA GEMMs with GELU /
residual / DropPath epilogues, layer scale folded into the second GEMM's operand; the GELU-MLP branch (`ops._gelu_mlp_fwd` /
`ops._gelu_mlp_bwd`) is the one the Swin / DiNAT block body runs.  The 4x4 stride-4 stem is the K = 48 patch GEMM of
the Swin PatchEmbed, the 2x2 stride-2 downsample convolutions are a patch gather + GEMM (`ops.conv2x2_s2`); a `channels_first`
LayerNorm of a map that is stored channels-last is the ordinary row LayerNorm.  Stochastic depth is applied in training mode, one draw
per block and sample (`ops.drop_path_scales`).  The kernels need channel counts that are multiples of 8 (every stock width is).
"""
import torch
import torch.nn as nn

from ... import ops
from ...d2 import BACKBONE_REGISTRY, Backbone, ShapeSpec


class LayerNorm(nn.Module):
    """LayerNorm over the channels of a `channels_last` (..., C) tensor or a `channels_first` (B, C, H, W) map."""

    def __init__(self, normalized_shape, eps=1e-6, data_format="channels_last"):
        super().__init__()
        if data_format not in ("channels_last", "channels_first"):
            raise NotImplementedError
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps, self.data_format, self.normalized_shape = eps, data_format, (normalized_shape,)

    def forward(self, x, out_dtype=torch.float32):
        if self.data_format == "channels_last":
            return ops.layer_norm(x, self.weight, self.bias, out_dtype=out_dtype, eps=self.eps)
        # (B, C, H, W)-shaped; a channels-last stored map permutes for free
        return ops.layer_norm(x.permute(0, 2, 3, 1), self.weight, self.bias, out_dtype=out_dtype, eps=self.eps).permute(0, 3, 1, 2)


class Block(nn.Module):
    """x + drop_path(gamma * pwconv2(gelu(pwconv1(norm(dwconv(x)))))) on a channels-last fp32 map (B, H, W, C)."""

    def __init__(self, dim, drop_path=0.0, layer_scale_init_value=1e-6):
        super().__init__()
        if dim % 8 != 0:
            raise ValueError(f"ConvNeXt Block: dim must be a multiple of 8 for the HIP depthwise-convolution kernels (got {dim})")
        self.dwconv = nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.pwconv1 = nn.Linear(dim, 4 * dim)
        self.act = nn.GELU()
        self.pwconv2 = nn.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(layer_scale_init_value * torch.ones(dim)) if layer_scale_init_value > 0 else None
        self.drop_path_rate = float(drop_path)

    def params(self):
        return [self.dwconv.weight, self.dwconv.bias, self.norm.weight, self.norm.bias, self.pwconv1.weight, self.pwconv1.bias,
                self.pwconv2.weight, self.pwconv2.bias, self.gamma]

    def forward(self, x, dp=None):
        """x (B, H, W, C) fp32 residual stream.  dp: DropPath multipliers to use instead of a fresh draw (tests)."""
        if dp is None and self.training and self.drop_path_rate > 0.0:
            dp = ops.drop_path_scales(x.shape[0], self.drop_path_rate)
        return ops.convnext_block(x, self.params(), dp=dp, eps=self.norm.eps)


class _Stem(nn.Sequential):
    """4x4 stride-4 convolution as a K = 48 GEMM over patch rows + LayerNorm: (B, Cin, H, W) image -> (B, H/4, W/4, C) fp32."""

    def forward(self, x):
        conv, norm = self[0], self[1]
        B, Cin, H, W = x.shape
        ph, pw = conv.kernel_size
        Hh, Ww = H // ph, W // pw
        patches = x[:, :, :Hh * ph, :Ww * pw].reshape(B, Cin, Hh, ph, Ww, pw).permute(0, 2, 4, 1, 3, 5).reshape(B, Hh * Ww, Cin * ph * pw)
        y = ops.linear(patches, conv.weight, conv.bias, out_dtype=torch.float32)
        y = ops.layer_norm(y, norm.weight, norm.bias, out_dtype=torch.float32, eps=norm.eps)
        return y.view(B, Hh, Ww, conv.out_channels)


class _Downsample(nn.Sequential):
    """LayerNorm (to the GEMM operand dtype) + 2x2 stride-2 convolution as patch gather + GEMM, channels-last in and out."""

    def forward(self, x):
        norm, conv = self[0], self[1]
        h = ops.layer_norm(x, norm.weight, norm.bias, out_dtype=torch.bfloat16, eps=norm.eps)
        return ops.conv2x2_s2(h, conv.weight, conv.bias)


class ConvNeXt(nn.Module):
    def __init__(self, in_chans=3, depths=[3, 3, 9, 3], dims=[96, 192, 384, 768], drop_path_rate=0.0, layer_scale_init_value=1e-6,
                 out_indices=[0, 1, 2, 3]):
        super().__init__()
        bad = [d for d in dims if d % 8 != 0]
        if bad:
            raise ValueError(f"ConvNeXt: dims must be multiples of 8 for the HIP depthwise-convolution kernels (got {bad})")
        self.num_features = dims
        self.downsample_layers = nn.ModuleList()
        self.downsample_layers.append(_Stem(nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4),
                                            LayerNorm(dims[0], eps=1e-6, data_format="channels_first")))
        for i in range(3):
            self.downsample_layers.append(_Downsample(LayerNorm(dims[i], eps=1e-6, data_format="channels_first"),
                                                      nn.Conv2d(dims[i], dims[i + 1], kernel_size=2, stride=2)))
        rates = [r.item() for r in torch.linspace(0, drop_path_rate, sum(depths))]
        self.stages = nn.ModuleList()
        first = 0
        for i in range(4):
            self.stages.append(nn.Sequential(*[Block(dim=dims[i], drop_path=rates[first + j], layer_scale_init_value=layer_scale_init_value)
                                               for j in range(depths[i])]))
            first += depths[i]
        self.out_indices = out_indices
        for i in range(4):
            self.add_module(f"norm{i}", LayerNorm(dims[i], eps=1e-6, data_format="channels_first"))

    def forward_features(self, x):
        outs = {}
        for i in range(4):
            x = self.downsample_layers[i](x)
            x = self.stages[i](x)
            if i in self.out_indices:
                n = getattr(self, f"norm{i}")
                # (B, C, H, W)-shaped, stored channels-last: the 1x1 convs downstream read token rows directly
                outs[f"res{i + 2}"] = ops.layer_norm(x, n.weight, n.bias, out_dtype=torch.float32, eps=n.eps).permute(0, 3, 1, 2)
        return outs

    def forward(self, x):
        return self.forward_features(x)


@BACKBONE_REGISTRY.register()
class D2ConvNeXt(ConvNeXt, Backbone):
    def __init__(self, cfg, input_shape):
        c = cfg.MODEL.CONVNEXT
        super().__init__(in_chans=c.IN_CHANNELS, depths=c.DEPTHS, dims=c.DIMS, drop_path_rate=c.DROP_PATH_RATE,
                         layer_scale_init_value=c.LSIT, out_indices=c.OUT_INDICES)
        self._out_features = c.OUT_FEATURES
        self._out_feature_strides = {"res2": 4, "res3": 8, "res4": 16, "res5": 32}
        self._out_feature_channels = {f"res{i + 2}": self.num_features[i] for i in range(4)}

    def forward(self, x):
        assert x.dim() == 4, f"ConvNeXt takes an input of shape (N, C, H, W). Got {x.shape} instead!"
        y = super().forward(x)
        return {k: v for k, v in y.items() if k in self._out_features}

    def output_shape(self):
        return {name: ShapeSpec(channels=self._out_feature_channels[name], stride=self._out_feature_strides[name])
                for name in self._out_features}

    @property
    def size_divisibility(self):
        return 32
