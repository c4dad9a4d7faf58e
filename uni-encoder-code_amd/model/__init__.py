"""Import facade with the reference package's name: `from model import add_common_config, ...`

`train_net.py` / `demo/demo.py` of the reference do `from model import (add_common_config,
add_swin_config, add_uni_encoder_config, ...)` and rely on the import side effect of registering
`OneFormer`, `D2SwinTransformer`, `OneFormerHead`, `MSDeformAttnPixelDecoder` and the transformer
decoder (model/__init__.py:1-23, model/modeling/__init__.py:1-10).  Putting
`uni-encoder-code_amd/` on PYTHONPATH gives those drivers this implementation instead.
"""
import sys as _sys

from uenc.config import *  # noqa: F401,F403
from uenc.config import __all__ as _cfg_all
from uenc import modeling  # noqa: F401  (registers backbone / heads / decoder)
from uenc.oneformer_model import OneFormer  # noqa: F401
from uenc.evaluation import InstanceSegEvaluator  # noqa: F401  (train_net.py:55-56 imports it from `model`)

# `model.modeling` IS `uenc.modeling` (one object, also for the import system), so the reference's submodule imports resolve to the
# product's modules: `from model.modeling.matcher import HungarianMatcher` gives `uenc.modeling.matcher.HungarianMatcher`.
_sys.modules[__name__ + ".modeling"] = modeling
_sys.modules[__name__ + ".modeling.matcher"] = modeling.matcher
_sys.modules[__name__ + ".modeling.criterion"] = modeling.criterion
_sys.modules[__name__ + ".modeling.targets"] = modeling.targets
_sys.modules[__name__ + ".modeling.monodepth_loss"] = modeling.monodepth_loss
_sys.modules[__name__ + ".modeling.pixel_decoder"] = modeling.pixel_decoder
_sys.modules[__name__ + ".modeling.pixel_decoder.fpn"] = modeling.pixel_decoder.fpn
_sys.modules[__name__ + ".modeling.pixel_decoder.transdssl"] = modeling.pixel_decoder.transdssl
_sys.modules[__name__ + ".modeling.pose_decoder"] = modeling.pose_decoder
_sys.modules[__name__ + ".modeling.pose_decoder.resnet_like_pose_decoder"] = modeling.pose_decoder.resnet_like_pose_decoder
_sys.modules[__name__ + ".modeling.backbone"] = modeling.backbone
_sys.modules[__name__ + ".modeling.backbone.convnext"] = modeling.backbone.convnext
_sys.modules[__name__ + ".modeling.backbone.resnet"] = modeling.backbone.resnet

__all__ = list(_cfg_all) + ["OneFormer", "modeling", "InstanceSegEvaluator"]
