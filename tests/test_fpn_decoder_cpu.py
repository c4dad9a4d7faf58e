"""The FPN pixel decoders (uenc/modeling/pixel_decoder/fpn.py) without a GPU: the registry and the default config, state-dict names and
shapes against those the reference's classes have (stored in tests/golden/fpn_pixel_decoder.npz), a reference-layout checkpoint through
load_state_dict, the refusal of pre-norm, and the import facade."""
import pytest
import torch

import fpn_decoder_fixture as FX


@pytest.fixture(scope="module")
def Z():
    return FX.load()


def _net(case, **kw):
    import model  # noqa: F401
    from uenc.d2 import ShapeSpec
    from uenc.modeling.pixel_decoder import fpn
    return FX.build(fpn, case, ShapeSpec, **kw)


def _cfg(*extra):
    import model  # noqa: F401
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list(["MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead", "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"], *extra])
    return cfg


def _shapes():
    from uenc.d2 import ShapeSpec
    return {k: ShapeSpec(channels=c, stride=s) for k, (c, s, _, _) in FX.FEATURES.items()}


def test_default_config_builds_a_head():
    """MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME defaults to "BasePixelDecoder": a config that does not override it builds that class."""
    from uenc.d2 import build_sem_seg_head
    cfg = _cfg()
    assert cfg.MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME == "BasePixelDecoder"
    head = build_sem_seg_head(cfg, _shapes())
    dec = head.pixel_decoder
    assert type(dec).__name__ == "BasePixelDecoder" and dec.in_features == ["res2", "res3", "res4", "res5"]
    assert dec.mask_features.kernel_size == (3, 3) and dec.mask_features.bias is not None
    assert dec.mask_features.out_channels == cfg.MODEL.SEM_SEG_HEAD.MASK_DIM and dec.layer_4.in_channels == FX.FEATURES["res5"][0]


def test_from_config_keys_of_the_transformer_decoder():
    from uenc.d2 import build_sem_seg_head
    cfg = _cfg("MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "TransformerEncoderPixelDecoder", "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 3,
               "MODEL.ONE_FORMER.DIM_FEEDFORWARD", 512, "MODEL.ONE_FORMER.NHEADS", 8, "MODEL.ONE_FORMER.DROPOUT", 0.2)
    dec = build_sem_seg_head(cfg, _shapes()).pixel_decoder
    assert type(dec).__name__ == "TransformerEncoderPixelDecoder"
    layers = dec.transformer.encoder.layers
    assert len(layers) == 3 and layers[0].linear1.out_features == 512 and layers[0].self_attn.num_heads == 8
    assert layers[0].dropout_p == 0.2 and layers[0].self_attn.dropout == 0.2 and layers[0].self_attn.tiled
    assert dec.layer_4.in_channels == cfg.MODEL.SEM_SEG_HEAD.CONVS_DIM and dec.input_proj.in_channels == FX.FEATURES["res5"][0]


@pytest.mark.parametrize("case", FX.CASES)
def test_state_dict_is_the_reference_s(Z, case):
    sd = _net(case).state_dict()
    assert list(sd.keys()) == [str(n) for n in Z[case + "_names"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in Z[case + "_shapes"]]
    assert {"grad:" + k for k in sd} == {k[len(case) + 1:] for k in Z if k.startswith(case + "_grad:")}     # every entry is a parameter


@pytest.mark.parametrize("case", FX.CASES)
def test_reference_layout_checkpoint_round_trips(Z, case):
    from oracle import fill
    net = _net(case)
    sd = {str(n): fill.tensor_for("rt." + str(n), [int(v) for v in str(s).split(",")]) for n, s in zip(Z[case + "_names"], Z[case + "_shapes"])}
    net.load_state_dict(sd, strict=True)
    back = net.state_dict()
    assert list(back.keys()) == list(sd.keys()) and all(torch.equal(back[k], sd[k]) for k in sd)


def test_pre_norm_is_refused_naming_its_key():
    from uenc.modeling.pixel_decoder.fpn import build_pixel_decoder
    from uenc.modeling.transformer_decoder.oneformer_transformer_decoder import TransformerEncoderLayer
    for layers in (0, 2):
        cfg = _cfg("MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "TransformerEncoderPixelDecoder", "MODEL.ONE_FORMER.PRE_NORM", True,
                   "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", layers)
        with pytest.raises(NotImplementedError, match=r"MODEL\.ONE_FORMER\.PRE_NORM"):
            build_pixel_decoder(cfg, _shapes())
    with pytest.raises(NotImplementedError, match=r"MODEL\.ONE_FORMER\.PRE_NORM"):
        TransformerEncoderLayer(128, 4, normalize_before=True)


def test_class_transformer_still_refuses_encoder_layers():
    """ENC_LAYERS > 0 of the class transformer stays out of scope: TransformerEncoder without layer arguments refuses as before."""
    from uenc.modeling.transformer_decoder.oneformer_transformer_decoder import TransformerEncoder
    assert len(TransformerEncoder(0).layers) == 0
    with pytest.raises(NotImplementedError, match="ENC_LAYERS"):
        TransformerEncoder(2)


def test_facade_import():
    from model.modeling.pixel_decoder.fpn import BasePixelDecoder, TransformerEncoderPixelDecoder, build_pixel_decoder
    from uenc.d2 import SEM_SEG_HEADS_REGISTRY
    from uenc.modeling.pixel_decoder import fpn
    assert BasePixelDecoder is fpn.BasePixelDecoder and TransformerEncoderPixelDecoder is fpn.TransformerEncoderPixelDecoder
    assert build_pixel_decoder is fpn.build_pixel_decoder
    assert SEM_SEG_HEADS_REGISTRY.get("BasePixelDecoder") is BasePixelDecoder
    assert SEM_SEG_HEADS_REGISTRY.get("TransformerEncoderPixelDecoder") is TransformerEncoderPixelDecoder
    assert issubclass(TransformerEncoderPixelDecoder, BasePixelDecoder)
