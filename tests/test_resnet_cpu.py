"""The ResNet backbone's drop-in surface without a GPU: registry, config keys, state-dict layout, output shapes, freeze(), the keys that
are refused, the `model` facade, and the stored fixture's own figures."""
import json

import pytest
import torch

import resnet_fixture as RF


def _cfg(**over):
    import model  # noqa: F401  registers the backbones
    from uenc.d2 import get_cfg
    cfg = get_cfg()
    with open(RF.CFG_BASE) as f:
        base = json.load(f)["MODEL"]
    opts = {f"MODEL.{sec}.{k}": v for sec in ("BACKBONE", "RESNETS") for k, v in base[sec].items()}
    opts["MODEL.DEVICE"] = "cpu"
    opts.update(over)
    cfg.merge_from_list([v for kv in opts.items() for v in kv])
    return cfg


def _build(**over):
    from uenc.d2 import BACKBONE_REGISTRY, ShapeSpec
    cfg = _cfg(**over)
    return BACKBONE_REGISTRY.get(cfg.MODEL.BACKBONE.NAME)(cfg, ShapeSpec(channels=3))


@pytest.fixture(scope="module")
def Z():
    return RF.load()


def test_registry_and_facade_resolve_the_builder():
    import model  # noqa: F401
    from model.modeling.backbone.resnet import build_custom_resnet_backbone
    from uenc.d2 import BACKBONE_REGISTRY
    from uenc.modeling.backbone import resnet as R
    assert BACKBONE_REGISTRY.get("build_custom_resnet_backbone") is build_custom_resnet_backbone is R.build_custom_resnet_backbone
    for name in ("BasicStem", "BasicBlock", "BottleneckBlock", "ResNet", "make_stage", "ResNetBlockBase"):
        assert hasattr(R, name)


def test_base_config_builds_r18():
    from uenc.d2 import Backbone
    from uenc.modeling.backbone import resnet as R
    m = _build()                                               # (no DEFORM_* key in the config: deformable blocks are off)
    assert isinstance(_build(**{"MODEL.RESNETS.DEFORM_ON_PER_STAGE": [False] * 4}), R.ResNet)
    assert isinstance(m, R.ResNet) and isinstance(m, Backbone)
    assert [len(s) for s in m.stages] == [2, 2, 2, 2] and all(type(b) is R.BasicBlock for s in m.stages for b in s)
    assert isinstance(m.stem.conv1.norm, torch.nn.SyncBatchNorm) and all(p.requires_grad for p in m.parameters())
    sd = m.state_dict()
    assert sd["stem.conv1.weight"].shape == (64, 3, 7, 7) and sd["res5.1.conv2.weight"].shape == (512, 512, 3, 3)
    assert sd["res3.0.shortcut.weight"].shape == (128, 64, 1, 1) and "res2.0.shortcut.weight" not in sd
    assert sd["stem.conv1.norm.num_batches_tracked"].dtype == torch.int64 and len(sd) == 120


@pytest.mark.parametrize("which", RF.NETS)
def test_state_dict_names_and_shapes_equal_the_reference(Z, which):
    from uenc.modeling.backbone import resnet as R
    sd = RF.build(R, which).state_dict()
    assert list(sd.keys()) == [str(n) for n in Z[which + "_names"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in Z[which + "_shapes"]]


def test_output_shape_channels_and_strides():
    o = _build().output_shape()
    assert {k: (v.channels, v.stride) for k, v in o.items()} == {"stem": (64, 2), "res2": (64, 4), "res3": (128, 8), "res4": (256, 16),
                                                                 "res5": (512, 32)}
    m = _build(**{"MODEL.RESNETS.OUT_FEATURES": ["res2", "res3"]})
    assert list(m.output_shape()) == ["res2", "res3"] and m.stage_names == ("res2", "res3") and not hasattr(m, "res4")
    with pytest.raises(ValueError, match=r"must be an \(N, C, H, W\) image batch"):
        m(torch.zeros(3, 8, 8))


def test_r50_keys_build_bottleneck_blocks():
    from uenc.modeling.backbone import resnet as R
    m = _build(**{"MODEL.RESNETS.DEPTH": 50, "MODEL.RESNETS.RES2_OUT_CHANNELS": 256, "MODEL.RESNETS.NORM": "FrozenBN"})
    assert [len(s) for s in m.stages] == [3, 4, 6, 3] and all(type(b) is R.BottleneckBlock for s in m.stages for b in s)
    assert {k: v.channels for k, v in m.output_shape().items()} == {"stem": 64, "res2": 256, "res3": 512, "res4": 1024, "res5": 2048}
    b = m.res3[0]
    assert b.conv1.stride == (1, 1) and b.conv2.stride == (2, 2) and b.shortcut.stride == (2, 2) and b.conv2.weight.shape == (128, 128, 3, 3)
    assert _build(**{"MODEL.RESNETS.DEPTH": 50, "MODEL.RESNETS.RES2_OUT_CHANNELS": 256, "MODEL.RESNETS.STRIDE_IN_1X1": True}).res3[0].conv1.stride == (2, 2)
    assert "stem.conv1.norm.num_batches_tracked" not in m.state_dict()


def test_freeze_matches_the_reference(Z):
    from uenc.d2 import FrozenBatchNorm2d
    from uenc.modeling.backbone import resnet as R
    m = RF.build(R, "basic")
    assert m.freeze(2) is m
    assert [n for n, p in m.named_parameters() if p.requires_grad] == [str(n) for n in Z["frozen_trainable"]]
    sd = m.state_dict()
    assert list(sd.keys()) == [str(n) for n in Z["frozen_names"]]
    assert [",".join(str(s) for s in v.shape) for v in sd.values()] == [str(s) for s in Z["frozen_shapes"]]
    assert isinstance(m.res2[1].conv2.norm, FrozenBatchNorm2d) and isinstance(m.res3[0].conv1.norm, torch.nn.BatchNorm2d)
    assert isinstance(_build(**{"MODEL.BACKBONE.FREEZE_AT": 1}).stem.conv1.norm, FrozenBatchNorm2d)


def test_frozen_batchnorm_loads_with_and_without_the_batch_counter():
    from uenc.d2 import FrozenBatchNorm2d, get_norm
    f = get_norm("FrozenBN", 8)
    assert isinstance(f, FrozenBatchNorm2d) and f.eps == 1e-5 and sorted(n for n, _ in f.named_buffers()) == ["bias", "running_mean", "running_var", "weight"]
    assert not list(f.parameters())
    sd = torch.nn.BatchNorm2d(8).state_dict()
    sd["running_mean"] = torch.arange(8.0)
    f.load_state_dict(dict(sd), strict=True)                    # with num_batches_tracked
    sd.pop("num_batches_tracked")
    f.load_state_dict(dict(sd), strict=True)                    # and without
    assert torch.equal(f.running_mean, torch.arange(8.0))
    bn = torch.nn.BatchNorm2d(8).eval()
    bn.load_state_dict(f.state_dict(), strict=False)
    x = torch.randn(2, 8, 3, 3)
    assert torch.allclose(f(x), bn(x), atol=1e-6)


def test_get_norm_knows_the_batchnorms_and_refuses_the_rest():
    from uenc.d2 import get_norm
    assert type(get_norm("BN", 8)) is torch.nn.BatchNorm2d and type(get_norm("SyncBN", 8)) is torch.nn.SyncBatchNorm
    assert get_norm("", 8) is None and type(get_norm("GN", 32)) is torch.nn.GroupNorm
    for bad in ("LN", "nnSyncBN", "naiveSyncBN"):
        with pytest.raises(NotImplementedError):
            get_norm(bad, 8)


def test_unsupported_keys_raise_naming_the_key():
    from uenc.modeling.backbone import resnet as R
    r50 = {"MODEL.RESNETS.DEPTH": 50, "MODEL.RESNETS.RES2_OUT_CHANNELS": 256}
    with pytest.raises(NotImplementedError, match="DEFORM_ON_PER_STAGE"):
        _build(**r50, **{"MODEL.RESNETS.DEFORM_ON_PER_STAGE": [False, True, True, True]})
    with pytest.raises(NotImplementedError, match="DEFORM_ON_PER_STAGE"):
        R.DeformBottleneckBlock(64, 256, bottleneck_channels=64)
    with pytest.raises(NotImplementedError, match="RES5_DILATION"):
        _build(**r50, **{"MODEL.RESNETS.RES5_DILATION": 2})
    with pytest.raises(NotImplementedError, match="NUM_GROUPS"):
        _build(**r50, **{"MODEL.RESNETS.NUM_GROUPS": 32})
    with pytest.raises(NotImplementedError, match="num_classes"):
        R.ResNet(R.BasicStem(3, 16), [R.ResNet.make_stage(R.BasicBlock, 1, in_channels=16, out_channels=16)], num_classes=10)
    with pytest.raises(NotImplementedError, match="RES5_DILATION"):
        R.BottleneckBlock(64, 256, bottleneck_channels=64, dilation=2)


def test_fixture_self_checks(Z):
    with open(RF.CFG_BASE) as f:
        base = json.load(f)
    assert set(base) == {"MODEL"} and set(base["MODEL"]) == {"BACKBONE", "RESNETS"} and base["MODEL"]["RESNETS"]["DEPTH"] == 18
    assert tuple(Z["x"].shape) == RF.X
    for c in RF.CASES:
        assert float(Z[c + "_rounding_out"]) < 1e-5 and float(Z[c + "_rounding_grad"]) < 1e-5, c
        names = [str(n) for n in Z[c.split("_")[0] + "_names"]]
        params = [n for n in names if n.split(".")[-1] in ("weight", "bias")]
        for key in [f"out:{k}" for k in RF.OUTS] + ["loss"] + [f"grad:{n}" for n in params]:
            assert f"{c}_{key}" in Z, (c, key)
            e, cs = float(Z[f"{c}_env_err:{key}"]), float(Z[f"{c}_env_cos:{key}"])
            assert 0.0 <= e < 1.0 and 0.8 < cs <= 1.0 + 1e-12, (c, key, e, cs)
        for k in RF.OUTS:
            o = Z[f"{c}_out:{k}"]
            assert o.shape[0] == 2 and tuple(o.shape[2:]) == RF.SIZES[k]
        if c.endswith("train"):
            for n in names:
                if n.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked"):
                    assert f"{c}_buf:{n}" in Z
            assert int(Z[f"{c}_buf:stem.conv1.norm.num_batches_tracked"]) == 1
    assert not any("num_batches_tracked" in str(n) and str(n).startswith(("stem", "res2")) for n in Z["frozen_names"])
    assert any(str(n) == "res3.0.conv1.norm.num_batches_tracked" for n in Z["frozen_names"])
    assert all(f"frozen_grad:{n}" in Z for n in Z["frozen_trainable"]) and "frozen_grad:stem.conv1.weight" not in Z


def test_make_stage_and_default_stages():
    from uenc.modeling.backbone import resnet as R
    blocks = R.make_stage(R.BottleneckBlock, 3, in_channels=16, out_channels=64, bottleneck_channels=16, stride_per_block=[2, 1, 1], norm="BN")
    assert [(b.in_channels, b.out_channels, b.stride) for b in blocks] == [(16, 64, 2), (64, 64, 1), (64, 64, 1)]
    assert blocks[0].shortcut is not None and blocks[1].shortcut is None and blocks[0].conv2.stride == (2, 2)
    with pytest.raises(ValueError, match="stride_per_block has 2 entries for 3 blocks"):
        R.ResNet.make_stage(R.BasicBlock, 3, in_channels=16, out_channels=16, stride_per_block=[1, 1])
    with pytest.raises(ValueError, match="either stride or stride_per_block"):
        R.ResNet.make_stage(R.BasicBlock, 1, in_channels=16, out_channels=16, stride_per_block=[1], stride=1)
    for depth, counts, widths in ((34, [3, 4, 6, 3], [64, 128, 256, 512]), (50, [3, 4, 6, 3], [256, 512, 1024, 2048])):
        stages = R.ResNet.make_default_stages(depth, norm="FrozenBN")
        assert [len(s) for s in stages] == counts and [s[-1].out_channels for s in stages] == widths
        assert [s[0].stride for s in stages] == [1, 2, 2, 2] and all(b.stride == 1 for s in stages for b in s[1:])
        assert all(type(b) is (R.BasicBlock if depth < 50 else R.BottleneckBlock) for s in stages for b in s)
        if depth == 50:
            assert [s[0].conv2.weight.shape[0] for s in stages] == [64, 128, 256, 512]
        net = R.ResNet(R.BasicStem(3, 64, norm="FrozenBN"), stages)
        assert list(net.output_shape()) == ["res5"] and net.output_shape()["res5"].stride == 32
    with pytest.raises(ValueError, match="out_features"):
        R.ResNet(R.BasicStem(3, 16), [R.ResNet.make_stage(R.BasicBlock, 1, in_channels=16, out_channels=16)], out_features=["res3"])
    with pytest.raises(ValueError, match="non-empty list of CNNBlockBase"):
        R.ResNet(R.BasicStem(3, 16), [[]])
