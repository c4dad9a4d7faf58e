"""BasePixelDecoder and TransformerEncoderPixelDecoder (uenc/modeling/pixel_decoder/fpn.py) against tests/golden/fpn_pixel_decoder.npz:
what the reference's own pixel_decoder/fpn.py computes on the cases of tests/fpn_decoder_fixture.py (tools/make_fpn_decoder_golden.py).

Bars (relative L2 error; the project's, tests/test_resnet_gpu.py:4-8).  fp32 "exact" mode: 1e-4 for outputs and loss, 1e-3 for every stored
gradient (the reference's own fp32 rounding on these cases is below 1e-5, stored in the file).  Product mode: 1.5 * env + 2e-2 per quantity,
env being the same quantity's error in the reference run with bf16-rounded parameters and Conv2d / Linear inputs, and for gradients
cosine >= env_cos - 0.01.  The figures go to `record_parity("fpn_decoder/...")`.

Training mode (dropout 0.1) of one TransformerEncoderLayer is compared with a float64 restatement of reference transformer.py:196-214 that is
fed the layer's recorded keep-masks (dropout1, the FFN's inner dropout, dropout2) and the attention kernels' keep-mask restated by
`uenc.attention.keep_mask_reference`: the same bars, the product-mode envelope taken from the restatement itself with bf16-rounded
parameters and Linear inputs.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import fpn_decoder_fixture as FX
from conftest import record_parity

pytestmark = pytest.mark.gpu
rel, cos = FX.rel, FX.cos


@pytest.fixture(scope="module")
def U():
    import model  # noqa: F401
    import uenc
    return uenc


@pytest.fixture(scope="module")
def Z():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in FX.load().items()}


@pytest.fixture()
def exact():
    from uenc import ops
    ops.set_exact(True)
    yield
    ops.set_exact(False)


def _net(case, **kw):
    from uenc.d2 import ShapeSpec
    from uenc.modeling.pixel_decoder import fpn
    net = FX.build(fpn, case, ShapeSpec, **kw)
    FX.fill_module(net, case)
    return net.cuda()


def _run(Z, case, net=None, train=False):
    net = _net(case) if net is None else net
    net.train(train)
    x = {k: Z["x:" + k].cuda() for k in FX.FEATURES}
    mf, enc, ms = net.forward_features(x)
    full = FX.quantities(mf, enc, ms)
    sizes = [FX.FEATURES[k][2:] for k in ("res5", "res4", "res3")]
    for i, t in enumerate(ms):
        assert tuple(t.shape) == (FX.B, FX.CONV_DIM) + sizes[i] and t.stride(1) == 1, i                  # channels-last views
    assert tuple(mf.shape) == (FX.B, FX.MASK_DIM) + FX.FEATURES["res2"][2:] and mf.stride(1) == 1 and mf.dtype == torch.float32
    assert (enc is None) == (case == "base")
    loss = FX.loss_of(full)
    loss.backward()
    torch.cuda.synchronize()
    q = {k: FX.sub_out(v.detach().float()) for k, v in full.items()}
    q["loss"] = loss.detach()
    for n, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        q["grad:" + n] = FX.sub_grad(p.grad)
    return q, full, net


@pytest.mark.parametrize("case", FX.CASES)
def test_decoder_exact(U, Z, exact, case):
    q, _, _ = _run(Z, case)
    figs = {k: rel(v, Z[f"{case}_{k}"]) for k, v in q.items()}
    print({k: f"{v:.2e}" for k, v in figs.items()})
    record_parity("fpn_decoder/exact/" + case, **figs)
    assert set(figs) == {k[len(case) + 1:] for k in Z if k.startswith(case + "_out:") or k.startswith(case + "_grad:")} | {"loss"}
    for k, v in figs.items():
        assert q[k].shape == Z[f"{case}_{k}"].shape, k
        assert v <= (1e-3 if k.startswith("grad:") else 1e-4), (k, v)


@pytest.mark.parametrize("case", FX.CASES)
def test_decoder_product(U, Z, case):
    q, _, _ = _run(Z, case)
    figs = {k: rel(v, Z[f"{case}_{k}"]) for k, v in q.items()}
    coss = {k: cos(v, Z[f"{case}_{k}"]) for k, v in q.items() if k.startswith("grad:")}
    env = {k: float(Z[f"{case}_env_err:{k}"]) for k in figs}
    print({k: (f"{figs[k]:.3g}", f"env {env[k]:.3g}") for k in figs})
    record_parity("fpn_decoder/bf16/" + case, **figs, **{"cos:" + k: v for k, v in coss.items()}, **{"env:" + k: v for k, v in env.items()},
                  **{"env_cos:" + k: float(Z[f"{case}_env_cos:{k}"]) for k in coss})
    for k in figs:
        assert figs[k] <= 1.5 * env[k] + 2e-2, (k, figs[k], env[k])
        if k.startswith("grad:"):
            assert coss[k] >= float(Z[f"{case}_env_cos:{k}"]) - 0.01, (k, coss[k])


def test_training_without_dropout_equals_eval_bit_for_bit(U, Z):
    """Every output bit for bit; the parameter gradients to 1e-6 (some weight-gradient GEMMs add split partials atomically)."""
    net = _net("tenc", dropout=0.0)
    _, ev, _ = _run(Z, "tenc", net)
    g_eval = {n: p.grad.clone() for n, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    _, tr, _ = _run(Z, "tenc", net, train=True)
    for k in ev:
        assert torch.equal(ev[k], tr[k]), k
    for n, p in net.named_parameters():
        assert rel(p.grad, g_eval[n]) <= 1e-6, n


# ---- one encoder layer in training mode against float64 ------------------------------------------------------------------------------
def _layer64(P, src, pos, H, p, attn_keep, masks, rnd=lambda t: t):
    """reference transformer.py:196-214 (forward_post) in float64, batch-first; masks = keep-masks of dropout1, the FFN's inner dropout,
    dropout2; rnd: rounding of parameters and Linear inputs (identity, or to bf16 for the envelope)."""
    lin = lambda x, w, b: rnd(x) @ rnd(w).t() + rnd(b)
    E = src.shape[-1]
    W, bias = P["self_attn.in_proj_weight"], P["self_attn.in_proj_bias"]
    qk = src + pos
    q, k, v = lin(qk, W[:E], bias[:E]), lin(qk, W[E:2 * E], bias[E:2 * E]), lin(src, W[2 * E:], bias[2 * E:])
    heads = lambda t: t.view(t.shape[0], t.shape[1], H, E // H).transpose(1, 2)
    a = torch.softmax(heads(q) @ heads(k).transpose(-1, -2) / math.sqrt(E // H), -1) * (attn_keep.double() / (1.0 - p))
    o = (a @ heads(v)).transpose(1, 2).reshape(src.shape)
    h = lin(o, P["self_attn.out_proj.weight"], P["self_attn.out_proj.bias"])
    x = F.layer_norm(src + h * masks[0].double() / (1.0 - p), (E,), P["norm1.weight"], P["norm1.bias"])
    f = torch.relu(lin(x, P["linear1.weight"], P["linear1.bias"])) * masks[1].double() / (1.0 - p)
    f = lin(f, P["linear2.weight"], P["linear2.bias"])
    return F.layer_norm(x + f * masks[2].double() / (1.0 - p), (E,), P["norm2.weight"], P["norm2.bias"])


def _ste_bf16(t):
    """Round to bf16, gradient passed straight through (what a bf16-operand GEMM with fp32 master weights does)."""
    return t + (t.bfloat16().to(t.dtype) - t).detach()


@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_encoder_layer_training_with_dropout(U, mode):
    from oracle import fill
    from uenc import ops
    from uenc.attention import keep_mask_reference
    from uenc.modeling.transformer_decoder.oneformer_transformer_decoder import TransformerEncoderLayer
    B, L, E, H, p = 2, 70, 128, 4, 0.1                      # 70 tokens: a second, ragged query tile and key block
    layer = TransformerEncoderLayer(E, H, 256, p).cuda().train()
    fill.fill_module(layer, "fpn_decoder/train_layer.")
    g = torch.Generator().manual_seed(5)
    src0, pos, dout = (torch.randn(B, L, E, generator=g).cuda() for _ in range(3))
    src = src0.clone().requires_grad_(True)
    torch.manual_seed(11)
    ops.set_exact(mode == "exact")
    try:
        out = layer(src, pos)
        out.backward(dout)
        torch.cuda.synchronize()
    finally:
        ops.set_exact(False)
    assert len(layer._masks) == 3 and layer.self_attn.last_seed is not None
    keep = keep_mask_reference(B, H, L, L, p, layer.self_attn.last_seed).cuda()
    assert 0.85 < float(keep.double().mean()) < 0.95 and all(0.85 < float(m.double().mean()) < 0.95 for m in layer._masks)

    def ref(rnd):
        P = {n: q.detach().double().requires_grad_(True) for n, q in layer.named_parameters()}
        s64 = src0.double().requires_grad_(True)
        o = _layer64(P, s64, pos.double(), H, p, keep, layer._masks, rnd)
        o.backward(dout.double())
        r = {"out": o.detach(), "grad:src": s64.grad}
        r.update({"grad:" + n: q.grad for n, q in P.items()})
        return r
    want = ref(lambda t: t)
    got = {"out": out.detach(), "grad:src": src.grad}
    got.update({"grad:" + n: q.grad for n, q in layer.named_parameters()})
    figs = {k: rel(got[k], want[k]) for k in want}
    if mode == "exact":
        bars = {k: (1e-3 if k.startswith("grad:") else 1e-4) for k in want}
    else:
        envq = ref(_ste_bf16)
        bars = {k: 1.5 * rel(envq[k], want[k]) + 2e-2 for k in want}
    print({k: (f"{figs[k]:.3g}", f"bar {bars[k]:.3g}") for k in figs})
    record_parity(f"fpn_decoder/train_layer/{mode}", **figs, **{"bar:" + k: v for k, v in bars.items()})
    for k in figs:
        assert figs[k] <= bars[k], (k, figs[k], bars[k])


# ---- the ATen arms: no norm, and a GroupNorm outside the kernels' domain -------------------------------------------------------------
def _base_torch(net, x):
    """BasePixelDecoder.forward_features restated with ATen on NCHW maps (reference pixel_decoder/fpn.py:138-156) on the module's weights."""
    ms, y = [], None
    for idx, f in enumerate(net.in_features[::-1]):
        lat, outc = net.lateral_convs[idx], net.output_convs[idx]
        if lat is None:
            y = outc(x[f])
        else:
            cur = lat(x[f])
            y = outc(cur + F.interpolate(y, size=cur.shape[-2:], mode="nearest"))
        if len(ms) < 3:
            ms.append(y)
    return net.mask_features(y), ms


@pytest.mark.parametrize("norm", ["", "GN"])
def test_aten_fallback_arms(U, Z, exact, norm):
    """conv_dim 64: GroupNorm(32, 64) has 2 channels per group (outside `_gn_tokens_ok`); norm "": biased convolutions without a norm.
    Both run the GEMMs, the patch gather and the nearest merge on HIP and the rest through ATen; fp32 mode against the ATen restatement."""
    from uenc.modeling.pixel_decoder.msdeformattn import _gn_tokens_ok
    net = _net("base", norm=norm, conv_dim=64)
    assert net.adapter_1.norm is None if norm == "" else not _gn_tokens_ok(net.adapter_1.norm)
    assert (net.adapter_1.bias is not None) == (norm == "")
    x = {k: Z["x:" + k].cuda() for k in FX.FEATURES}
    mf, enc, ms = net.forward_features(x)
    loss = FX.loss_of(FX.quantities(mf, enc, ms))
    loss.backward()
    got = {n: p.grad.clone() for n, p in net.named_parameters()}
    net.zero_grad(set_to_none=True)
    mf_t, ms_t = _base_torch(net.double(), {k: v.double() for k, v in x.items()})
    FX.loss_of(FX.quantities(mf_t, None, ms_t)).backward()
    figs = {"out:mask": rel(mf, mf_t), **{f"out:ms{i}": rel(a, b) for i, (a, b) in enumerate(zip(ms, ms_t))}}
    figs.update({"grad:" + n: rel(got[n], p.grad) for n, p in net.named_parameters()})
    record_parity("fpn_decoder/fallback/" + (norm or "none"), **figs)
    for k, v in figs.items():
        assert v <= (1e-3 if k.startswith("grad:") else 1e-4), (k, v)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["BasePixelDecoder", "TransformerEncoderPixelDecoder"])
def test_full_model_with_each_decoder(U, name):
    import json

    import resnet_fixture as RF
    from oracle import fill, torch_ref as T
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    base = json.load(open(RF.CFG_BASE))["MODEL"]
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", base["BACKBONE"]["NAME"], "MODEL.BACKBONE.FREEZE_AT", 0,
        "MODEL.RESNETS.DEPTH", base["RESNETS"]["DEPTH"], "MODEL.RESNETS.RES2_OUT_CHANNELS", base["RESNETS"]["RES2_OUT_CHANNELS"],
        "MODEL.RESNETS.NORM", "BN", "MODEL.RESNETS.STRIDE_IN_1X1", base["RESNETS"]["STRIDE_IN_1X1"],
        "MODEL.RESNETS.OUT_FEATURES", ["res2", "res3", "res4", "res5"], "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", name, "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 2, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    assert type(m.sem_seg_head.pixel_decoder).__name__ == name
    fill.fill_module(m)
    RF.fill_module(m.backbone, "full.")
    m.eval()
    g = torch.Generator().manual_seed(0)
    batch = [{"left_image": torch.randint(0, 256, (3, 64, 96), generator=g).float(), "task": t, "type": "segmentation"}
             for t in ("The task is panoptic", "The task is semantic")]
    out, _ = m.forward_features(batch)
    T.synthetic_loss(out).backward()
    torch.cuda.synchronize()
    assert out["pred_logits"].shape == (2, 150, 20) and out["pred_masks"].shape == (2, 150, 16, 24)
    assert bool(torch.isfinite(out["pred_logits"]).all()) and bool(torch.isfinite(out["pred_masks"].float()).all())
    for n, p in m.sem_seg_head.pixel_decoder.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
