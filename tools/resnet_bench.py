"""ResNet on one GPU: the HIP path against the same module tree run through ATen (F.conv2d channels-last, F.batch_norm, F.relu,
F.max_pool2d), the latter once in fp32 and once under bf16 autocast, legs alternating in one fresh process; device time by events,
median / min / max.

  (a) the R18 and R50 backbones of `build_custom_resnet_backbone` ("BN", all five outputs), forward + backward at 2 x 3 x 1024 x 2048, in
      eval mode and in train mode (--no-r50 / --no-backbone skip);
  (b) each kernel of csrc/resnet.hip alone at the R18 stem's shapes (image 2 x 3 x 1024 x 2048, map 2 x 512 x 1024 x 64), with the achieved
      bytes/s from its algorithmic bytes (every operand read once, every result written once) against the 8 TB/s HBM roof.

    python tools/resnet_bench.py --iters 10 --warmup 3 [--out profiles/resnet_bench.json]
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


def _cbn(conv, x, relu=False, res=None):
    n = conv.norm
    x = F.conv2d(x, conv.weight, None, conv.stride, conv.padding)
    if hasattr(n, "num_batches_tracked"):
        x = F.batch_norm(x, n.running_mean, n.running_var, n.weight, n.bias, n.training, n.momentum, n.eps)
    else:
        x = n(x)
    if res is not None:
        x = x + res
    return F.relu(x) if relu else x


def torch_resnet(net, x):
    """The backbone as an ATen composition sharing `net`'s parameters and buffers (NCHW-shaped, channels-last stored)."""
    outs = {"stem": _cbn(net.stem.conv1, x, relu=True)}
    x = F.max_pool2d(outs["stem"], 3, 2, 1)
    for name, stage in zip(net.stage_names, net.stages):
        for b in stage:
            sc = x if b.shortcut is None else _cbn(b.shortcut, x)
            h = _cbn(b.conv1, x, relu=True)
            if hasattr(b, "conv3"):
                h = _cbn(b.conv2, h, relu=True)
                x = _cbn(b.conv3, h, relu=True, res=sc)
            else:
                x = _cbn(b.conv2, h, relu=True, res=sc)
        outs[name] = x
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


def bench_backbone(depth, iters, warmup):
    from uenc.d2 import ShapeSpec, get_cfg
    from uenc.modeling.backbone.resnet import build_custom_resnet_backbone
    cfg = get_cfg()
    cfg.merge_from_list(["MODEL.BACKBONE.FREEZE_AT", 0, "MODEL.RESNETS.DEPTH", depth, "MODEL.RESNETS.NORM", "BN", "MODEL.RESNETS.RES2_OUT_CHANNELS",
                         64 if depth < 50 else 256, "MODEL.RESNETS.STRIDE_IN_1X1", False, "MODEL.RESNETS.OUT_FEATURES",
                         ["stem", "res2", "res3", "res4", "res5"]])
    torch.manual_seed(0)
    net = build_custom_resnet_backbone(cfg, ShapeSpec(channels=3)).cuda()
    x = torch.randn(2, 3, 1024, 2048, device="cuda")
    xc = x.contiguous(memory_format=torch.channels_last)

    def zero():
        for p in net.parameters():
            p.grad = None

    def hip():
        zero()
        sum(v.square().mean() for v in net(x).values()).backward()

    def t32():
        zero()
        sum(v.square().mean() for v in torch_resnet(net, xc).values()).backward()

    def t16():
        zero()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            outs = torch_resnet(net, xc)
        sum(v.float().square().mean() for v in outs.values()).backward()
    res = {"shape": [2, 3, 1024, 2048], "model": f"R{depth}"}
    for mode in ("eval", "train"):
        net.train(mode == "train")
        res[mode + "_fwd_bwd_ms"] = timed({"hip": hip, "aten_fp32": t32, "aten_bf16_autocast": t16}, iters, warmup)
    return res


def bench_kernels(iters, warmup):
    from uenc import kernels as K
    B, H, W, C = 2, 512, 1024, 64
    torch.manual_seed(0)
    img = torch.randn(B, 3, 2 * H, 2 * W, device="cuda")
    x = torch.randn(B * H * W, C, device="cuda")                       # a convolution's fp32 result
    gamma, beta = torch.rand(C, device="cuda") + 0.5, torch.randn(C, device="cuda")
    mean, var = K.bn_stats(x)
    y = K.bn_act_fwd(x, mean, var, gamma, beta, relu=True, out_dtype=torch.bfloat16)
    dy = torch.randn(B * H * W, C, device="cuda").to(torch.bfloat16)
    x4 = x.view(B, H, W, C)
    p, idx = K.maxpool3x3_s2_fwd(x4)
    dp = torch.randn_like(p)
    N, Mp = x.numel(), p.numel()
    rm, rv, nbt = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")
    legs = {"stem7x7_s2_patches": lambda: K.stem7x7_s2_patches(img),
            "maxpool3x3_s2_fwd": lambda: K.maxpool3x3_s2_fwd(x4),
            "maxpool3x3_s2_bwd": lambda: K.maxpool3x3_s2_bwd(dp, idx, H, W),
            "bn_stats": lambda: K.bn_stats(x, rm, rv, nbt),
            "bn_act_fwd": lambda: K.bn_act_fwd(x, mean, var, gamma, beta, relu=True, out_dtype=torch.bfloat16),
            "bn_act_bwd_reduce_apply": lambda: K.bn_act_bwd(dy, y, x, mean, var, gamma, relu=True, train=True, dx_dtype=torch.bfloat16),
            "aten_batch_norm_relu_fwd_fp32": lambda: F.relu(F.batch_norm(x4.permute(0, 3, 1, 2), None, None, gamma, beta, True)),
            "aten_max_pool2d_fwd_fp32": lambda: F.max_pool2d(x4.permute(0, 3, 1, 2), 3, 2, 1)}
    kt = timed(legs, iters, warmup)
    nbytes = {"stem7x7_s2_patches": img.numel() * 4 + B * H * W * 152 * 2, "maxpool3x3_s2_fwd": 4 * N + 5 * Mp, "maxpool3x3_s2_bwd": 5 * Mp + 4 * N,
              "bn_stats": 4 * N, "bn_act_fwd": 4 * N + 2 * N,
              "bn_act_bwd_reduce_apply": (2 + 2 + 4) * N + (2 + 2 + 4 + 2) * N}
    for k, nb in nbytes.items():
        kt[k]["algorithmic_bytes"] = nb
        kt[k]["TB_per_s"] = nb / (kt[k]["median"] * 1e-3) / 1e12
        kt[k]["share_of_hbm_roof"] = nb / (kt[k]["median"] * 1e-3) / HBM_ROOF
    return {"map": [B, H, W, C], "image": [B, 3, 2 * H, 2 * W], "kernels_ms": kt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-backbone", action="store_true")
    ap.add_argument("--no-r50", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "resnet_bench.py measures on the GPU"
    import model  # noqa: F401
    out = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "kernels": bench_kernels(a.iters, a.warmup)}
    if not a.no_backbone:
        out["backbones"] = [bench_backbone(d, max(3, a.iters // 2), 2) for d in ([18] if a.no_r50 else [18, 50])]
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
