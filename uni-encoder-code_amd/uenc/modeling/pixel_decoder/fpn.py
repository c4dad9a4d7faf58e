"""The plain FPN pixel decoders -- counterpart of reference model/modeling/pixel_decoder/fpn.py:23-315.

`build_pixel_decoder` (same dispatch and error as :23-35), `BasePixelDecoder` (:39-161), `TransformerEncoderOnly` (:164-202) and
`TransformerEncoderPixelDecoder` (:206-315): same registry names, constructor arguments, `from_config` keys and parameter names
(`adapter_{i}`, `layer_{i}`, `mask_features`, `input_proj`, `transformer.encoder.layers.{l}.{self_attn.in_proj_weight,
self_attn.in_proj_bias, self_attn.out_proj, linear1, linear2, norm1, norm2}`), same `forward_features(features) -> (mask_features,
transformer_encoder_features | None, multi_scale_features)` contract.

Every map stays a channels-last token matrix (B, H*W, C); what is returned are (B, C, H, W) views of those, which the predictor
consumes without copies.  Lateral 1x1 conv + GroupNorm is one node (GEMM + the GroupNorm kernels), the nearest-neighbour top-down merge a
HIP kernel (csrc/fpn_nearest.hip), the 3x3 output conv + GroupNorm + ReLU one node (patch gather + GEMM + GroupNorm kernels), `mask_features`
a 3x3 patch GEMM with its bias in the GEMM epilogue.  The DETR encoder on res5 runs on the query-tiled attention kernels
(csrc/attn_tiled.hip): res5 of a 1024 x 2048 image is 2048 tokens attending to themselves.  ATen remains for a GroupNorm shape outside
the kernels' domain and a non-GroupNorm `norm`, as in msdeformattn.py.
"""
import logging
from typing import Callable, Dict, Optional, Union

import torch
from torch import nn
from torch.nn import functional as F

from ... import ops
from ...d2 import SEM_SEG_HEADS_REGISTRY, Conv2d, ShapeSpec, configurable, get_norm
from ..transformer_decoder.oneformer_transformer_decoder import TransformerEncoder
from ..transformer_decoder.position_encoding import PositionEmbeddingSine
from .msdeformattn import _conv1x1_gn, _gn_tokens_ok, _tokens


def build_pixel_decoder(cfg, input_shape, depth_decoder=False):
    name = cfg.MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME if not depth_decoder else cfg.MODEL.SEM_SEG_HEAD.DEPTH_DECODER_NAME
    model = SEM_SEG_HEADS_REGISTRY.get(name)(cfg, input_shape)
    forward_features = getattr(model, "forward_features", None)
    if not callable(forward_features):
        raise ValueError(
            "Only SEM_SEG_HEADS with forward_features method can be used as pixel decoder. "
            f"Please implement forward_features for {name} to only return mask features.")
    return model


def _c2_xavier_fill(module: nn.Module) -> None:
    """fvcore.nn.weight_init.c2_xavier_fill."""
    nn.init.kaiming_uniform_(module.weight, a=1)
    if module.bias is not None:
        nn.init.constant_(module.bias, 0)


def _plain3x3(conv: nn.Conv2d) -> bool:
    return (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1
            and conv.in_channels % 8 == 0)


def _nchw(tok: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """(B, H*W, C) tokens -> the (B, C, H, W) view of the same memory."""
    return tok.reshape(tok.shape[0], H, W, -1).permute(0, 3, 1, 2)


def _output_conv(x_nhwc: torch.Tensor, conv: Conv2d) -> torch.Tensor:
    """3x3 conv (+ norm) + ReLU of an FPN level on a channels-last map (B, H, W, Cin) -> tokens (B, H*W, Cout)."""
    B, H, W, _ = x_nhwc.shape
    if not _plain3x3(conv):
        return _tokens(conv(x_nhwc.permute(0, 3, 1, 2).float()))
    if isinstance(conv.norm, nn.GroupNorm) and _gn_tokens_ok(conv.norm) and conv.bias is None and conv.activation is F.relu:
        return ops.conv3x3_group_norm(x_nhwc, conv.weight, conv.norm, relu=True, out_dtype=torch.bfloat16)
    z = ops.conv3x3(x_nhwc, conv.weight, conv.bias)                                  # patch gather + GEMM (bias in its epilogue)
    if conv.norm is not None:
        z = _tokens(conv.norm(_nchw(z, H, W)))
    return conv.activation(z) if conv.activation is not None else z


def _lateral_merge(x_tok: torch.Tensor, conv: Conv2d, prev_nhwc: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """cur_fpn + F.interpolate(y, size=(H, W), mode="nearest") (reference :149-151) -> tokens (B, H*W, C)."""
    gn = conv.norm
    if isinstance(gn, nn.GroupNorm) and _gn_tokens_ok(gn):
        return ops.linear_group_norm(x_tok, conv, gn, add_src=prev_nhwc, add_hw=(H, W), out_dtype=torch.bfloat16, merge="nearest")
    cur = _conv1x1_gn(x_tok, conv, gn, H, W)                                         # GEMM; the norm, if any, through ATen
    if cur.shape[-1] % 4 == 0:
        return ops.merge_nearest(cur.float(), prev_nhwc, (H, W), out_dtype=torch.bfloat16)
    up = F.interpolate(prev_nhwc.permute(0, 3, 1, 2).float(), size=(H, W), mode="nearest")
    return cur + _tokens(up)


@SEM_SEG_HEADS_REGISTRY.register()
class BasePixelDecoder(nn.Module):
    predicts_depth = False          # a segmentation pixel decoder: OneFormerHead does not build it for MODEL.SEM_SEG_HEAD.DEPTH_DECODER_NAME

    @configurable
    def __init__(self, input_shape: Dict[str, ShapeSpec], *, conv_dim: int, mask_dim: int, norm: Optional[Union[str, Callable]] = None):
        super().__init__()
        input_shape = sorted(input_shape.items(), key=lambda x: x[1].stride)
        self.in_features = [k for k, v in input_shape]                               # "res2" .. "res5"
        feature_channels = [v.channels for k, v in input_shape]
        lateral_convs, output_convs = [], []
        use_bias = norm == ""
        for idx, in_channels in enumerate(feature_channels):
            if idx == len(self.in_features) - 1:
                output_conv = Conv2d(in_channels, conv_dim, kernel_size=3, stride=1, padding=1, bias=use_bias,
                                     norm=get_norm(norm, conv_dim), activation=F.relu)
                _c2_xavier_fill(output_conv)
                self.add_module("layer_{}".format(idx + 1), output_conv)
                lateral_convs.append(None)
                output_convs.append(output_conv)
            else:
                lateral_conv = Conv2d(in_channels, conv_dim, kernel_size=1, bias=use_bias, norm=get_norm(norm, conv_dim))
                output_conv = Conv2d(conv_dim, conv_dim, kernel_size=3, stride=1, padding=1, bias=use_bias,
                                     norm=get_norm(norm, conv_dim), activation=F.relu)
                _c2_xavier_fill(lateral_conv)
                _c2_xavier_fill(output_conv)
                self.add_module("adapter_{}".format(idx + 1), lateral_conv)
                self.add_module("layer_{}".format(idx + 1), output_conv)
                lateral_convs.append(lateral_conv)
                output_convs.append(output_conv)
        # top-down order (from low to high resolution)
        self.lateral_convs = lateral_convs[::-1]
        self.output_convs = output_convs[::-1]
        self.mask_dim = mask_dim
        self.mask_features = Conv2d(conv_dim, mask_dim, kernel_size=3, stride=1, padding=1)
        _c2_xavier_fill(self.mask_features)
        self.oneformer_num_feature_levels = 3                                        # always use 3 scales

    @classmethod
    def from_config(cls, cfg, input_shape: Dict[str, ShapeSpec]):
        return {
            "input_shape": {k: v for k, v in input_shape.items() if k in cfg.MODEL.SEM_SEG_HEAD.IN_FEATURES},
            "conv_dim": cfg.MODEL.SEM_SEG_HEAD.CONVS_DIM,
            "mask_dim": cfg.MODEL.SEM_SEG_HEAD.MASK_DIM,
            "norm": cfg.MODEL.SEM_SEG_HEAD.NORM,
        }

    def _top(self, x: torch.Tensor):
        """The coarsest level's input to its output conv as a channels-last map, and the transformer-encoder feature (None here)."""
        return x.permute(0, 2, 3, 1), None

    def forward_features(self, features):
        multi_scale_features = []
        y, hw, encoder_features = None, None, None
        for idx, f in enumerate(self.in_features[::-1]):
            x = features[f].float()
            B, _, H, W = x.shape
            lateral_conv, output_conv = self.lateral_convs[idx], self.output_convs[idx]
            if lateral_conv is None:
                top, encoder_features = self._top(x)
                y = _output_conv(top, output_conv)
            else:
                cur = _lateral_merge(_tokens(x), lateral_conv, y.reshape(B, hw[0], hw[1], -1), H, W)
                y = _output_conv(cur.reshape(B, H, W, -1), output_conv)
            hw = (H, W)
            if len(multi_scale_features) < self.oneformer_num_feature_levels:
                multi_scale_features.append(_nchw(y, H, W))
        mf = self.mask_features
        if _plain3x3(mf) and mf.norm is None and mf.activation is None:
            out = _nchw(ops.conv3x3(y.reshape(B, hw[0], hw[1], -1), mf.weight, mf.bias), *hw)   # mask features stay channels-last in memory
        else:
            out = mf(_nchw(y, *hw).float())
        return out, encoder_features, multi_scale_features

    def forward(self, features, targets=None):
        logging.getLogger(__name__).warning("Calling forward() may cause unpredicted behavior of PixelDecoder module.")
        return self.forward_features(features)


class TransformerEncoderOnly(nn.Module):
    def __init__(self, d_model=512, nhead=8, num_encoder_layers=6, dim_feedforward=2048, dropout=0.1, activation="relu",
                 normalize_before=False):
        super().__init__()
        if normalize_before:
            raise NotImplementedError("MODEL.ONE_FORMER.PRE_NORM True (pre-norm encoder layers, transformer.py:216-234) is not implemented: "
                                      "every shipped config has MODEL.ONE_FORMER.PRE_NORM False")
        self.encoder = TransformerEncoder(num_encoder_layers, nn.LayerNorm(d_model) if normalize_before else None,
                                          layer_args=(d_model, nhead, dim_feedforward, dropout, activation, normalize_before))
        self._reset_parameters()
        self.d_model, self.nhead = d_model, nhead

    def _reset_parameters(self):
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, src, mask, pos_embed):
        """src, pos_embed: (B, H*W, C) channels-last tokens (the reference flattens NCHW to (HW, B, C)) -> (B, H*W, C) fp32."""
        if mask is not None:
            raise NotImplementedError("padding masks are not used on the segmentation path (pixel_decoder/fpn.py:297 passes None)")
        return self.encoder(src, pos_embed)


@SEM_SEG_HEADS_REGISTRY.register()
class TransformerEncoderPixelDecoder(BasePixelDecoder):
    @configurable
    def __init__(self, input_shape: Dict[str, ShapeSpec], *, transformer_dropout: float, transformer_nheads: int,
                 transformer_dim_feedforward: int, transformer_enc_layers: int, transformer_pre_norm: bool, conv_dim: int,
                 mask_dim: int, norm: Optional[Union[str, Callable]] = None):
        super().__init__(input_shape, conv_dim=conv_dim, mask_dim=mask_dim, norm=norm)
        input_shape = sorted(input_shape.items(), key=lambda x: x[1].stride)
        self.in_features = [k for k, v in input_shape]
        feature_channels = [v.channels for k, v in input_shape]
        in_channels = feature_channels[len(self.in_features) - 1]
        self.input_proj = Conv2d(in_channels, conv_dim, kernel_size=1)
        _c2_xavier_fill(self.input_proj)
        self.transformer = TransformerEncoderOnly(d_model=conv_dim, dropout=transformer_dropout, nhead=transformer_nheads,
                                                  dim_feedforward=transformer_dim_feedforward, num_encoder_layers=transformer_enc_layers,
                                                  normalize_before=transformer_pre_norm)
        self.pe_layer = PositionEmbeddingSine(conv_dim // 2, normalize=True)
        # the coarsest level's output conv now reads the encoder's conv_dim channels
        output_conv = Conv2d(conv_dim, conv_dim, kernel_size=3, stride=1, padding=1, bias=norm == "", norm=get_norm(norm, conv_dim),
                             activation=F.relu)
        _c2_xavier_fill(output_conv)
        delattr(self, "layer_{}".format(len(self.in_features)))
        self.add_module("layer_{}".format(len(self.in_features)), output_conv)
        self.output_convs[0] = output_conv

    @classmethod
    def from_config(cls, cfg, input_shape: Dict[str, ShapeSpec]):
        ret = super().from_config(cfg, input_shape)
        ret["transformer_dropout"] = cfg.MODEL.ONE_FORMER.DROPOUT
        ret["transformer_nheads"] = cfg.MODEL.ONE_FORMER.NHEADS
        ret["transformer_dim_feedforward"] = cfg.MODEL.ONE_FORMER.DIM_FEEDFORWARD
        ret["transformer_enc_layers"] = cfg.MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS     # a separate config
        ret["transformer_pre_norm"] = cfg.MODEL.ONE_FORMER.PRE_NORM
        return ret

    def _top(self, x: torch.Tensor):
        B, _, H, W = x.shape
        src = ops.linear(_tokens(x), self.input_proj.weight, self.input_proj.bias, out_dtype=torch.float32)
        memory = self.transformer(src, None, self.pe_layer.tokens(B, H, W, x.device))
        return memory.view(B, H, W, -1), _nchw(memory, H, W)
