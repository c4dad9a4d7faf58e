"""The oracle against the reference's own modules, on shapes the other fixtures do not hold: other window sizes, shifts and odd
feature maps.  The reference's inputs, parameter layouts and outputs are recorded in tests/golden/oracle_vs_reference.npz by
oracle/make_reference_golden.py; the parameter values are regenerated here from their names (oracle/fill.py), as they were there.
"""
import json

import pytest
import torch

from conftest import load_golden
from oracle import fill
from oracle import torch_ref as T


@pytest.fixture(scope="module")
def ref():
    g = load_golden("oracle_vs_reference")
    g["meta"] = json.loads(bytes(g.pop("meta_json").numpy()).decode())
    return g


def _state_dict(ref, tag):
    return fill.state_dict_for({k: tuple(s) for k, s in ref["meta"][tag]["param_shapes"].items()})


@pytest.mark.parametrize("C,nH,ws,H,W", [(32, 1, 4, 9, 11), (64, 2, 7, 14, 14), (64, 2, 12, 5, 30), (96, 3, 3, 6, 9)])
def test_basic_layer(ref, C, nH, ws, H, W):
    tag = f"basic_layer_{C}_{nH}_{ws}_{H}_{W}"
    sd = _state_dict(ref, tag)
    x, want = ref[tag + "_x"], ref[tag + "_out"]
    assert tuple(x.shape) == (2, H * W, C)
    with torch.no_grad():
        y = T.swin_block(x, sd, "backbone.layers.0.blocks.0", H, W, ws, 0, nH)
        y = T.swin_block(y, sd, "backbone.layers.0.blocks.1", H, W, ws, ws // 2, nH)
    torch.testing.assert_close(y, want, atol=2e-5, rtol=1e-5)


def test_relative_position_index(ref):
    for ws in (3, 7, 12):
        assert (ref[f"rpi_{ws}"].long() == T.relative_position_index(ws)).all()


def test_swin_with_padding_and_odd_merges(ref):
    cfg = T.SwinCfg(32, (2, 2, 2, 2), (1, 2, 4, 8), 5)
    sd = _state_dict(ref, "swin_odd")
    x = ref["swin_odd_x"]
    assert tuple(x.shape) == (1, 3, 70, 107)                                     # not a multiple of 4
    with torch.no_grad():
        got = T.swin_backbone(x, sd, cfg)
    assert sorted(got) == ref["meta"]["swin_odd"]["outputs"]
    for k in got:
        torch.testing.assert_close(got[k], ref[f"swin_odd_{k}"], atol=3e-5, rtol=1e-5)


def test_msdeform_core_matches_grid_sample_path(ref):
    shapes = [tuple(int(v) for v in s) for s in ref["msda_shapes"]]
    got = T.ms_deform_attn_core(ref["msda_value"], shapes, ref["msda_loc"], ref["msda_w"])
    torch.testing.assert_close(got, ref["msda_out"], atol=1e-5, rtol=1e-5)
