"""Shared by tools/make_fpn_decoder_golden.py and the FPN pixel-decoder tests: the cases of tests/golden/fpn_pixel_decoder.npz.

Both classes (`base` = BasePixelDecoder, `tenc` = TransformerEncoderPixelDecoder) with conv_dim = mask_dim = 128, norm "GN" (GroupNorm(32, 128)
is inside the GroupNorm kernels' domain), 4 heads (head_dim 32), dim_feedforward 256, 2 encoder layers, dropout 0.1 (eval mode in the
golden), on B = 2 feature maps res2 (16, 26, 50), res3 (24, 13, 25), res4 (40, 7, 13), res5 (48, 4, 7): odd sizes, so the nearest-merge
ratios are non-integer.  Parameters are not stored: both sides regenerate them from the state-dict name (oracle/fill.py, prefix
"fpn_decoder/<case>.").  Inputs are multiples of 1/64 in [-2, 2).
"""
import os

import numpy as np
import torch

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fpn_pixel_decoder.npz")
CASES = ["base", "tenc"]
B, CONV_DIM, MASK_DIM, NHEADS, DIM_FF, ENC_LAYERS, DROPOUT, NORM = 2, 128, 128, 4, 256, 2, 0.1, "GN"
FEATURES = {"res2": (16, 4, 26, 50), "res3": (24, 8, 13, 25), "res4": (40, 16, 7, 13), "res5": (48, 32, 4, 7)}   # channels, stride, H, W
# An output with more than OUT_CAP values is stored as every n-th channel, a gradient with more than GRAD_CAP as every n-th row (n = the
# smallest step that gets it under the cap).  The envelope figures are taken on the stored part.  One cap for both: the 3x3 kernels
# (128 x 1152) keep 4 rows.  With a single row (a cap of 1024, which the first version of this file had) the figure of `layer_4.weight` was that
# of ONE output channel over 56 tokens, 22 of them active, one with a pre-activation of 0.013 that the envelope's own rounding moves to
# 0.008: whether that one ReLU flips decided a 7 % against 2 % figure (tests/resnet_fixture.py notes the same effect).
OUT_CAP, GRAD_CAP = 4096, 4096


def build(mod, case: str, shape_spec, norm=NORM, conv_dim=CONV_DIM, dropout=DROPOUT, enc_layers=ENC_LAYERS):
    """The case's decoder from the module `mod` (the reference's pixel_decoder/fpn.py or uenc.modeling.pixel_decoder.fpn: same constructors)."""
    shp = {k: shape_spec(channels=c, stride=s) for k, (c, s, _, _) in FEATURES.items()}
    if case == "base":
        return mod.BasePixelDecoder(shp, conv_dim=conv_dim, mask_dim=MASK_DIM, norm=norm)
    return mod.TransformerEncoderPixelDecoder(shp, transformer_dropout=dropout, transformer_nheads=NHEADS, transformer_dim_feedforward=DIM_FF,
                                              transformer_enc_layers=enc_layers, transformer_pre_norm=False, conv_dim=conv_dim,
                                              mask_dim=MASK_DIM, norm=norm)


def fill_module(module, case: str) -> None:
    fill.fill_module(module, f"fpn_decoder/{case}.")


def inputs():
    out = {}
    for k, (c, _, h, w) in FEATURES.items():
        rng = fill._rng("fpn_decoder/input/" + k)
        out[k] = torch.from_numpy((rng.integers(-128, 128, (B, c, h, w)) / 64.0).astype(np.float32))
    return out


def quantities(mask_features, encoder_features, multi_scale):
    """{"out:<k>": tensor} of one forward_features result, in a fixed order: ms0..ms2 (coarse to fine), mask, and enc where there is one."""
    q = {f"out:ms{i}": t for i, t in enumerate(multi_scale)}
    q["out:mask"] = mask_features
    if encoder_features is not None:
        q["out:enc"] = encoder_features
    return q


def loss_of(q):
    return sum(t.float().square().mean() if t.dtype != torch.float64 else t.square().mean() for k, t in q.items() if k.startswith("out:"))


def step(numel: int, cap: int) -> int:
    return max(1, -(-int(numel) // cap))


def sub_out(t):
    """The stored part of an output (B, C, H, W): every n-th channel."""
    return t[:, ::step(t.numel(), OUT_CAP)]


def sub_grad(t):
    """The stored part of a parameter gradient: every n-th row."""
    return t[::step(t.numel(), GRAD_CAP)]


def stored(key, t):
    return sub_out(t) if key.startswith("out:") else (sub_grad(t) if key.startswith("grad:") else t)


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def cos(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).detach().double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
