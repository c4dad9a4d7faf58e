"""ConvNeXt on one GPU: the HIP path against the torch composition (F.conv2d(groups=C) channels-last, F.layer_norm, nn.Linear, F.gelu),
the latter once in fp32 and once under bf16 autocast, legs alternating in one fresh process; device time by events, median / min / max.

  (a) one ConvNeXt-L block, forward + backward, at the stage-1 (2 x 256 x 512 x 192) and stage-3 (2 x 64 x 128 x 768) shapes, and the
      three depthwise-convolution kernels alone with their achieved bytes/s from the algorithmic byte counts of DESIGN.md
      (forward 10 N, backward-data 22 N, backward-weight 8 N bytes for N = B H W C elements) against the 8 TB/s HBM roof;
  (b) the whole ConvNeXt-L backbone, forward + backward, at 2 x 3 x 1024 x 2048 (--no-backbone skips it).

    python tools/convnext_bench.py --iters 10 --warmup 3 [--out profiles/convnext_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    sys.path.insert(0, p)

HBM_ROOF = 8.0e12


class TorchBlock(nn.Module):
    """The block as a torch composition on an NCHW-shaped, channels-last stored map."""

    def __init__(self, blk):
        super().__init__()
        self.b = blk

    def forward(self, x):
        b = self.b
        y = F.conv2d(x, b.dwconv.weight, b.dwconv.bias, padding=3, groups=x.shape[1]).permute(0, 2, 3, 1)
        y = F.layer_norm(y, (y.shape[-1],), b.norm.weight, b.norm.bias, b.norm.eps)
        y = F.linear(F.gelu(F.linear(y, b.pwconv1.weight, b.pwconv1.bias)), b.pwconv2.weight, b.pwconv2.bias)
        if b.gamma is not None:
            y = b.gamma * y
        return x + y.permute(0, 3, 1, 2)


def torch_net(net, x):
    """The backbone as a torch composition sharing `net`'s parameters."""
    outs = []
    for i in range(4):
        ds = net.downsample_layers[i]
        if i == 0:
            x = F.conv2d(x, ds[0].weight, ds[0].bias, stride=4).permute(0, 2, 3, 1)
            x = F.layer_norm(x, (x.shape[-1],), ds[1].weight, ds[1].bias, 1e-6).permute(0, 3, 1, 2)
        else:
            x = F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), ds[0].weight, ds[0].bias, 1e-6).permute(0, 3, 1, 2)
            x = F.conv2d(x, ds[1].weight, ds[1].bias, stride=2)
        for blk in net.stages[i]:
            x = TorchBlock(blk)(x)
        n = getattr(net, f"norm{i}")
        outs.append(F.layer_norm(x.permute(0, 2, 3, 1), (x.shape[1],), n.weight, n.bias, 1e-6))
    return outs


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


def bench_block(shape, iters, warmup):
    from uenc import kernels as K
    from uenc.modeling.backbone.convnext import Block
    B, H, W, C = shape
    torch.manual_seed(0)
    blk = Block(C, layer_scale_init_value=1.0).cuda()
    tb = TorchBlock(blk)
    x = torch.randn(B, H, W, C, device="cuda")
    dout = torch.randn(B, H, W, C, device="cuda")
    xn, dn = x.permute(0, 3, 1, 2), dout.permute(0, 3, 1, 2)

    def hip():
        xi = x.clone().requires_grad_(True)
        blk(xi).backward(dout)

    def t32():
        xi = xn.clone().requires_grad_(True)
        tb(xi).backward(dn)

    def t16():
        xi = xn.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            o = tb(xi)
        o.backward(dn)
    res = {"shape": list(shape), "block_fwd_bwd_ms": timed({"hip": hip, "torch_fp32": t32, "torch_bf16_autocast": t16}, iters, warmup)}
    # the three new kernels alone
    p = [t.detach() for t in (blk.dwconv.weight, blk.dwconv.bias, blk.norm.weight, blk.norm.bias)]
    y, h, st = K.dwconv7_ln_fwd(x, *p)
    dh = torch.randn(B, H, W, C, device="cuda").to(K.adt())
    dx, dy = K.dwconv7_ln_bwd_data(dh, y, st, p[2], p[0], dout=dout)
    dw, db = torch.zeros_like(p[0]), torch.zeros_like(p[1])
    N = x.numel()
    kt = timed({"dwconv7_ln_fwd": lambda: K.dwconv7_ln_fwd(x, *p),
                "dwconv7_ln_bwd_data": lambda: K.dwconv7_ln_bwd_data(dh, y, st, p[2], p[0], dout=dout),
                "dwconv7_bwd_weight": lambda: K.dwconv7_bwd_weight(dy, x, dw, db),
                "torch_dwconv_ln_fwd_fp32": lambda: F.layer_norm(F.conv2d(xn, blk.dwconv.weight.detach(), p[1], padding=3, groups=C).permute(0, 2, 3, 1),
                                                                 (C,), p[2], p[3], 1e-6)}, iters, warmup)
    nbytes = {"dwconv7_ln_fwd": 10 * N, "dwconv7_ln_bwd_data": 22 * N, "dwconv7_bwd_weight": 8 * N}
    for k, nb in nbytes.items():
        kt[k]["algorithmic_bytes"] = nb
        kt[k]["TB_per_s"] = nb / (kt[k]["median"] * 1e-3) / 1e12
        kt[k]["share_of_hbm_roof"] = nb / (kt[k]["median"] * 1e-3) / HBM_ROOF
    res["kernels_ms"] = kt
    return res


def bench_backbone(iters, warmup):
    from uenc.modeling.backbone.convnext import ConvNeXt
    torch.manual_seed(0)
    net = ConvNeXt(3, [3, 3, 27, 3], [192, 384, 768, 1536], drop_path_rate=0.0, layer_scale_init_value=1.0).cuda()
    x = torch.randn(2, 3, 1024, 2048, device="cuda")
    xc = x.contiguous(memory_format=torch.channels_last)

    def zero():
        for p in net.parameters():
            p.grad = None

    def hip():
        zero()
        sum(v.float().square().mean() for v in net(x).values()).backward()

    def t32():
        zero()
        sum(v.square().mean() for v in torch_net(net, xc)).backward()

    def t16():
        zero()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = torch_net(net, xc)
        sum(v.float().square().mean() for v in outs).backward()
    return {"shape": [2, 3, 1024, 2048], "model": "ConvNeXt-L", "fwd_bwd_ms": timed({"hip": hip, "torch_fp32": t32, "torch_bf16_autocast": t16}, iters, warmup)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-backbone", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "convnext_bench.py measures on the GPU"
    import model  # noqa: F401
    out = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "blocks": [bench_block(s, a.iters, a.warmup) for s in ((2, 256, 512, 192), (2, 64, 128, 768))]}
    if not a.no_backbone:
        out["backbone"] = bench_backbone(max(3, a.iters // 2), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
