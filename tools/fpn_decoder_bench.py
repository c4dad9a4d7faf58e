"""The FPN pixel decoders on one GPU: the HIP path against the same module tree run through ATen (F.conv2d, F.group_norm, F.interpolate,
F.scaled_dot_product_attention, F.layer_norm), the latter once in fp32 and once under bf16 autocast, legs alternating in one fresh
process; device time by events, median / min / max.

  (a) BasePixelDecoder and TransformerEncoderPixelDecoder (conv_dim 256, GN, 8 heads, dim_feedforward 2048, 6 encoder layers, eval mode),
      forward + backward at the feature shapes of a 2 x 1024 x 2048 batch: Swin-L (192 / 384 / 768 / 1536 channels) and R50 (256 / 512 /
      1024 / 2048), maps 256x512, 128x256, 64x128, 32x64;
  (b) the attention core alone at B = 2, H = 8, L = 2048 (res5 of that image attending to itself): uenc_attn_tiled forward and forward +
      backward against F.scaled_dot_product_attention in bf16 and fp32, with the achieved share of the bf16 MFMA roof from the
      algorithmic FLOPs (forward 4 L^2 d per head, backward 10 L^2 d) and of the HBM roof from the algorithmic bytes.

    python tools/fpn_decoder_bench.py --iters 10 --warmup 3 [--out profiles/fpn_decoder_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    sys.path.insert(0, p)

HBM_ROOF = 8.0e12
MFMA_BF16_ROOF = 2.5e15          # dense bf16 MFMA peak of one MI355X
BACKBONES = {"swin_l": (192, 384, 768, 1536), "r50": (256, 512, 1024, 2048)}
MAPS = ((256, 512), (128, 256), (64, 128), (32, 64))


def timed(legs, iters, warmup):
    times = {k: [] for k in legs}
    for i in range(warmup + iters):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
    return {k: {"median": statistics.median(t), "min": min(t), "max": max(t)} for k, t in times.items()}


def _aten_encoder_layer(l, src, pos):
    """TransformerEncoderLayer (post-norm, eval) through ATen on (B, L, E) tokens, sharing the layer's parameters."""
    a = l.self_attn
    E, H = a.embed_dim, a.num_heads
    qk = src + pos
    q, k = F.linear(qk, a.in_proj_weight[:2 * E], a.in_proj_bias[:2 * E]).chunk(2, -1)
    v = F.linear(src, a.in_proj_weight[2 * E:], a.in_proj_bias[2 * E:])
    heads = lambda t: t.view(t.shape[0], t.shape[1], H, E // H).transpose(1, 2)
    o = F.scaled_dot_product_attention(heads(q), heads(k), heads(v)).transpose(1, 2).reshape(src.shape)
    src = F.layer_norm(src + F.linear(o, a.out_proj.weight, a.out_proj.bias), (E,), l.norm1.weight, l.norm1.bias)
    h = F.linear(F.relu(F.linear(src, l.linear1.weight, l.linear1.bias)), l.linear2.weight, l.linear2.bias)
    return F.layer_norm(src + h, (E,), l.norm2.weight, l.norm2.bias)


def aten_decoder(net, feats):
    """forward_features of either decoder as an ATen composition on NCHW maps (channels-last stored), sharing `net`'s parameters."""
    ms, y, enc = [], None, None
    for idx, f in enumerate(net.in_features[::-1]):
        x = feats[f]
        lat, outc = net.lateral_convs[idx], net.output_convs[idx]
        if lat is None:
            if hasattr(net, "transformer"):
                t = net.input_proj(x)
                B, C, H, W = t.shape
                tok = t.flatten(2).transpose(1, 2)
                pos = net.pe_layer.tokens(B, H, W, x.device)
                for l in net.transformer.encoder.layers:
                    tok = _aten_encoder_layer(l, tok, pos)
                enc = x = tok.transpose(1, 2).reshape(B, C, H, W)
            y = outc(x)
        else:
            cur = lat(x)
            y = outc(cur + F.interpolate(y, size=cur.shape[-2:], mode="nearest"))
        if len(ms) < 3:
            ms.append(y)
    return net.mask_features(y), enc, ms


def _loss(mf, enc, ms):
    return sum(t.float().square().mean() for t in [mf, *ms] + ([enc] if enc is not None else []))


def bench_decoder(name, backbone, iters, warmup):
    from uenc.d2 import ShapeSpec
    from uenc.modeling.pixel_decoder import fpn
    chans = BACKBONES[backbone]
    shp = {f"res{i + 2}": ShapeSpec(channels=c, stride=4 * 2 ** i) for i, c in enumerate(chans)}
    torch.manual_seed(0)
    if name == "BasePixelDecoder":
        net = fpn.BasePixelDecoder(shp, conv_dim=256, mask_dim=256, norm="GN")
    else:
        net = fpn.TransformerEncoderPixelDecoder(shp, transformer_dropout=0.1, transformer_nheads=8, transformer_dim_feedforward=2048,
                                                 transformer_enc_layers=6, transformer_pre_norm=False, conv_dim=256, mask_dim=256, norm="GN")
    net = net.cuda().eval()
    feats = {f"res{i + 2}": torch.randn(2, c, *MAPS[i], device="cuda").contiguous(memory_format=torch.channels_last)
             for i, c in enumerate(chans)}

    def zero():
        for p in net.parameters():
            p.grad = None

    def hip():
        zero()
        _loss(*net.forward_features(feats)).backward()

    def t32():
        zero()
        _loss(*aten_decoder(net, feats)).backward()

    def t16():
        zero()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = aten_decoder(net, feats)
        _loss(*out).backward()
    return {"decoder": name, "backbone": backbone, "channels": list(chans), "image": [2, 1024, 2048],
            "fwd_bwd_ms": timed({"hip": hip, "aten_fp32": t32, "aten_bf16_autocast": t16}, iters, warmup)}


def bench_core(iters, warmup):
    from uenc import ops
    B, H, L, D = 2, 8, 2048, 32
    E = H * D
    torch.manual_seed(0)
    qkv = torch.randn(B, L, 3 * E, device="cuda").to(torch.bfloat16).requires_grad_(True)
    dout = torch.randn(B, L, E, device="cuda").to(torch.bfloat16)
    q4 = [t.detach().view(B, L, H, D).transpose(1, 2).contiguous().requires_grad_(True) for t in qkv.detach().chunk(3, -1)]
    q32 = [t.detach().float().requires_grad_(True) for t in q4]
    d4 = dout.view(B, L, H, D).transpose(1, 2).contiguous()

    def hip(bwd):
        def run():
            qkv.grad = None
            o = ops.attention_tiled(qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:], H)
            if bwd:
                o.backward(dout)
        return run

    def sdpa(ts, g, bwd):
        def run():
            for t in ts:
                t.grad = None
            o = F.scaled_dot_product_attention(*ts)
            if bwd:
                o.backward(g)
        return run
    kt = timed({"hip_fwd": hip(False), "hip_fwd_bwd": hip(True), "sdpa_bf16_fwd": sdpa(q4, d4, False), "sdpa_bf16_fwd_bwd": sdpa(q4, d4, True),
                "sdpa_fp32_fwd": sdpa(q32, d4.float(), False), "sdpa_fp32_fwd_bwd": sdpa(q32, d4.float(), True)}, iters, warmup)
    flops_f, flops_b = 4.0 * B * H * L * L * D, 10.0 * B * H * L * L * D
    bytes_f = B * H * (4 * L * D * 2 + 4 * L)                                     # q, k, v read, out written (bf16), lse written
    bytes_b = B * H * (5 * L * D * 2 + 4 * L + L * D * 4 + 2 * L * D * 2)         # q, k, v, out, dout, lse read; dq fp32, dk, dv bf16 written
    bwd_ms = kt["hip_fwd_bwd"]["median"] - kt["hip_fwd"]["median"]
    kt["hip_fwd"].update(share_of_mfma_roof=flops_f / (kt["hip_fwd"]["median"] * 1e-3) / MFMA_BF16_ROOF,
                         share_of_hbm_roof=bytes_f / (kt["hip_fwd"]["median"] * 1e-3) / HBM_ROOF)
    kt["hip_bwd_by_difference"] = {"median": bwd_ms, "share_of_mfma_roof": flops_b / (bwd_ms * 1e-3) / MFMA_BF16_ROOF,
                                   "share_of_hbm_roof": bytes_b / (bwd_ms * 1e-3) / HBM_ROOF}
    return {"shape": {"B": B, "H": H, "L": L, "head_dim": D}, "ms": kt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-decoders", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fpn_decoder_bench.py measures on the GPU"
    import model  # noqa: F401
    out = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "attention_core": bench_core(a.iters, a.warmup)}
    if not a.no_decoders:
        out["decoders"] = [bench_decoder(n, b, max(3, a.iters // 2), 2)
                           for n in ("BasePixelDecoder", "TransformerEncoderPixelDecoder") for b in BACKBONES]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
