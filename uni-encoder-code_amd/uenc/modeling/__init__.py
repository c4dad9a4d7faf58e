from .backbone.swin import D2SwinTransformer
from .backbone.dinat import D2DiNAT
from .backbone.convnext import D2ConvNeXt
from .backbone.resnet import build_custom_resnet_backbone
from .pixel_decoder.msdeformattn import MSDeformAttnPixelDecoder
from .pixel_decoder.fpn import BasePixelDecoder, TransformerEncoderPixelDecoder, build_pixel_decoder
from .pixel_decoder.transdssl import TransDSSL
from .transformer_decoder.oneformer_transformer_decoder import ContrastiveMultiScaleMaskedTransformerDecoder
from .meta_arch.oneformer_head import OneFormerHead
from . import matcher
from .matcher import HungarianMatcher
from . import criterion
from .criterion import SetCriterion, build_criterion
from . import targets
from .targets import build_targets, targets_from_instances
from . import monodepth_loss
from .monodepth_loss import MonodepthLoss
