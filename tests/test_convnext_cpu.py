"""D2ConvNeXt's drop-in surface without a GPU: registry, state-dict layout, output shapes, argument checks, the `model` facade, and the
stored fixture against the live reference (build container only)."""
import numpy as np
import pytest
import torch

import convnext_fixture as CF


def _cfg(**over):
    import model  # noqa: F401  registers the backbones
    from uenc.config import add_common_config, add_convnext_config
    from uenc.d2 import get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_convnext_config(cfg)
    opts = {"MODEL.BACKBONE.NAME": "D2ConvNeXt", "MODEL.CONVNEXT.DEPTHS": CF.NET["depths"], "MODEL.CONVNEXT.DIMS": CF.NET["dims"],
            "MODEL.CONVNEXT.DROP_PATH_RATE": 0.0, "MODEL.CONVNEXT.LSIT": 1.0, "MODEL.DEVICE": "cpu"}
    opts.update(over)
    cfg.merge_from_list([v for kv in opts.items() for v in kv])
    return cfg


def _build(**over):
    from uenc.d2 import BACKBONE_REGISTRY, ShapeSpec
    cfg = _cfg(**over)
    return BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=3))


@pytest.fixture(scope="module")
def Z():
    return CF.load()


def test_builds_through_the_registry():
    from uenc.modeling.backbone.convnext import D2ConvNeXt
    from uenc.d2 import Backbone
    m = _build()
    assert type(m) is D2ConvNeXt and isinstance(m, Backbone) and m.size_divisibility == 32


def test_state_dict_names_and_shapes_equal_the_reference(Z):
    sd = _build().state_dict()
    assert list(sd.keys()) == [str(n) for n in Z["net_names"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in Z["net_shapes"]]


def test_load_state_dict_strict(Z):
    m = _build()
    sd = {str(n): CF.tensor_for("net." + str(n), [int(v) for v in str(s).split(",")]) for n, s in zip(Z["net_names"], Z["net_shapes"])}
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m.stages[0][1].gamma, sd["stages.0.1.gamma"])


def test_output_shape_and_out_features():
    m = _build()
    o = m.output_shape()
    assert {k: (v.channels, v.stride) for k, v in o.items()} == {"res2": (40, 4), "res3": (80, 8), "res4": (160, 16), "res5": (320, 32)}
    m = _build(**{"MODEL.CONVNEXT.OUT_FEATURES": ["res3", "res5"]})
    assert list(m.output_shape()) == ["res3", "res5"]
    with pytest.raises(AssertionError, match=r"ConvNeXt takes an input of shape \(N, C, H, W\)"):
        m(torch.zeros(3, 64, 96))


def test_no_layer_scale_has_no_gamma():
    m = _build(**{"MODEL.CONVNEXT.LSIT": 0.0})
    assert m.stages[0][0].gamma is None and not any(k.endswith("gamma") for k in m.state_dict())


def test_channel_counts_must_be_multiples_of_8():
    from uenc.modeling.backbone.convnext import Block
    with pytest.raises(ValueError):
        _build(**{"MODEL.CONVNEXT.DIMS": [36, 72, 144, 288]})
    with pytest.raises(ValueError):
        Block(12)


def test_drop_path_rates_are_a_linspace():
    m = _build(**{"MODEL.CONVNEXT.DROP_PATH_RATE": 0.5})
    rates = [b.drop_path_rate for s in m.stages for b in s]
    np.testing.assert_allclose(rates, np.linspace(0, 0.5, 6), atol=1e-7)


def test_facade_import_path():
    import model  # noqa: F401
    from model.modeling.backbone.convnext import D2ConvNeXt
    from uenc.modeling.backbone import convnext
    assert D2ConvNeXt is convnext.D2ConvNeXt


def test_new_entry_points_refuse_bad_arguments():
    from uenc.capi import lib
    import ctypes
    assert lib.uenc_dwconv7_ln_fwd(None, None, None, None, None, None, None, 0, None, 1, 4, 4, 8, ctypes.c_float(1e-6), None) == -1
    assert lib.uenc_dwconv7_bwd_weight_workspace_bytes(2, 16, 24, 40) == 2 * 2 * 3 * 50 * 40 * 4
    assert lib.uenc_dwconv7_bwd_weight_workspace_bytes(2, 16, 24, 36) == 0        # C % 8 != 0


def test_fixture_equals_the_live_reference(Z):
    """The stored outputs are what the reference computes now (build container only)."""
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference checkout not present")
    ref_loader._install_stubs()
    import sys
    sys.modules.pop("model.modeling.backbone.convnext", None)      # the product's facade alias, if `model` was imported before (restored by conftest)
    mod = ref_loader._load("model.modeling.backbone.convnext", "modeling/backbone/convnext.py")
    net = mod.ConvNeXt(**CF.NET)
    CF.fill_module(net, "net.")
    with torch.no_grad():
        out = net(torch.from_numpy(Z["net_x"]))
    for k in ("res2", "res3", "res4", "res5"):
        assert CF.rel(out[k], Z["net_" + k]) <= 1e-6, k
    assert float(Z["net_rounding_out"]) < 1e-5 and float(Z["net_rounding_grad"]) < 1e-5
