"""The differentiable depth and pose decoders of the sequence branch on one GPU: the HIP training path against the same module tree run
through ATen (nn.Conv2d, nn.BatchNorm2d, F.interpolate, F.softmax), the latter once in fp32 and once under bf16 autocast, legs alternating
in one process; device time by events, median / min / max.

  (a) TransDSSL and ResNetLike (train mode), forward + backward at the Swin-T feature shapes of a 192 x 512 frame, B = 3 (the
      sequence branch's training size, INPUT.DEPTH_CROP.SIZE of the reference's config);
  (b) the three kernel pairs of csrc/depth_head.hip alone at the largest maps of that size and of a 1024 x 2048 frame, B = 2 (256
      channels at half resolution for the upsample and the gate, 32 bins at full resolution for the head), forward and backward, against
      the ATen composition in fp32 and in bf16, with the share of the HBM roof from the algorithmic bytes (every operand read once,
      every result written once).  The time is that of the CALL -- the wrapper's output allocations and two launches inside one event
      window -- so for the sub-0.1 ms pairs the share is a lower bound on what the kernels themselves reach.
The decoders are NOT timed at 1024 x 2048: the one attempt wrote nothing for seven minutes in its first leg and was ended, and which leg
stalled is unknown (the hip leg keeps about 64 GB of saved bf16 patch matrices at that size -- `saved_patch_bytes` -- and the ATen fp32
leg runs first-call convolutions on 4 M-pixel 256-channel maps).  Every leg now reports each iteration as it ends, and a leg that runs out of
memory is recorded as such while the others go on.

    python tools/sequence_train_bench.py --iters 10 --warmup 3 [--out profiles/sequence_train_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

HBM_ROOF = 8.0e12
DECODER_SIZE = (3, 192, 512)
KERNEL_SIZES = ((3, 192, 512), (2, 1024, 2048))
SWIN_T_CH, STRIDES = (96, 192, 384, 768), (4, 8, 16, 32)


def saved_patch_bytes(B, H, W):
    """bf16 patch matrices (rows x 9 Cin) the depth decoder's 3x3 convolutions save for the backward: four 256-channel convolutions per
    two-input fusion block (two in refinenet4), at 1/32 .. 1/2 resolution, and a 256- and a 128-channel one per head at 1/8 .. 1/1."""
    rows = lambda s: B * (H // s) * (W // s)
    blocks = 2 * rows(32) + 4 * (rows(16) + rows(8) + rows(4) + rows(2))
    heads = sum(rows(s) for s in (8, 4, 2, 1))
    return 2 * 9 * (256 * blocks + (256 + 128) * heads)


def timed(legs, iters, warmup, tag=""):
    times, failed = {k: [] for k in legs}, {}
    for i in range(warmup + iters):
        for k, fn in legs.items():
            if k in failed:
                continue
            try:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
            except torch.OutOfMemoryError:
                failed[k] = "out of memory"
                torch.cuda.empty_cache()
                continue
            print(f"  [{tag}] {k} iteration {i}: {e0.elapsed_time(e1):.3f} ms", file=sys.stderr, flush=True)
            if i >= warmup:
                times[k].append(e0.elapsed_time(e1))
    out = {k: {"median": statistics.median(t), "min": min(t), "max": max(t)} for k, t in times.items() if t}
    out.update({k: {"error": v} for k, v in failed.items()})
    return out


def features(B, H, W, mult):
    g = torch.Generator(device="cuda").manual_seed(3)
    return {f"res{i + 2}": torch.randn(B, H // s, W // s, c * mult, device="cuda", generator=g).permute(0, 3, 1, 2).requires_grad_(True)
            for i, (c, s) in enumerate(zip(SWIN_T_CH, STRIDES))}


def decoder_legs(which, B, H, W):
    import sequence_train_fixture as SF          # the ATen walkers of the two module trees
    from oracle import fill
    from uenc import ops
    from uenc.modeling.pixel_decoder.transdssl import TransDSSL
    from uenc.modeling.pose_decoder.resnet_like_pose_decoder import ResNetLike
    m = TransDSSL(None, None) if which == "depth" else ResNetLike()
    fill.fill_module(m, "sem_seg_head.depth_decoder." if which == "depth" else "pose_decoder.")
    m.cuda().train()
    f = features(B, H, W, 1 if which == "depth" else 2)

    def scalar(out):
        return sum(v.float().sum() for v in (out.values() if isinstance(out, dict) else out))

    def hip():
        ops.begin_step()
        scalar(m.forward_features(f) if which == "depth" else m(f)).backward()
        ops.flush_wgrads()

    def aten(autocast):
        def run():
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                out = SF.aten_depth(m, f) if which == "depth" else SF.aten_pose(m, f)
            scalar(out).backward()
        return run
    return {"hip": hip, "aten_fp32": aten(False), "aten_bf16_autocast": aten(True)}


def kernel_legs(B, H, W):
    """name -> (legs, algorithmic bytes of the hip leg)."""
    from uenc import kernels as K
    g = torch.Generator(device="cuda").manual_seed(4)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)
    h, w, C, D = H // 2, W // 2, 256, 32
    out = {}
    # upsample: (B, h/2, w/2, C) -> (B, h, w, C)
    x, dy = r(B, h // 2, w // 2, C), r(B, h, w, C)
    xn = x.permute(0, 3, 1, 2).requires_grad_(True)
    up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
    def aten_up(dt):
        xx, dd = xn.detach().to(dt).requires_grad_(True), dy.permute(0, 3, 1, 2).to(dt)
        return lambda: up(xx).backward(dd)
    nb = 4 * (x.numel() + dy.numel())
    out["upsample2x_ac fwd+bwd"] = ({"hip": lambda: (K.upsample2x_ac_fwd(x), K.upsample2x_ac_bwd(dy)), "aten_fp32": aten_up(torch.float32),
                                     "aten_bf16": aten_up(torch.bfloat16)}, 2 * nb)
    # gate on (B * h * w, C)
    a, b, z, dg, dres = (r(B * h * w, C) for _ in range(5))
    def hip_gate():
        res, gg = K.softmax_gate_fwd(a, b, z)
        K.softmax_gate_bwd(dg, dres, z, res)
    def aten_gate(dt):
        aa, bb, zz = (t.to(dt).requires_grad_(True) for t in (a, b, z))
        d1, d2 = dg.to(dt), dres.to(dt)
        def run():
            res = aa + bb
            gg = res * F.softmax(zz, dim=-1)
            torch.autograd.backward([gg, res], [d1, d2])
        return run
    out["softmax_gate fwd+bwd"] = ({"hip": hip_gate, "aten_fp32": aten_gate(torch.float32), "aten_bf16": aten_gate(torch.bfloat16)},
                                   4 * a.numel() * (5 + 6))                       # fwd: 3 in, 2 out; bwd: 4 in, 2 out
    # head on (B * H * W, D)
    zz, grid, dd = r(B * H * W, D), torch.linspace(0.01, 1.0, D, device="cuda"), r(B * H * W)
    def aten_head(dt):
        zt = zz.to(dt).requires_grad_(True)
        return lambda: (F.softmax(zt.float(), dim=-1) * grid).sum(-1).backward(dd)
    out["soft_att_depth fwd+bwd"] = ({"hip": lambda: (K.soft_att_depth_fwd(zz, grid), K.soft_att_depth_bwd(dd, zz, grid)),
                                      "aten_fp32": aten_head(torch.float32), "aten_bf16": aten_head(torch.bfloat16)},
                                     4 * (zz.numel() * 3 + 2 * dd.numel()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequence_train_bench.json"))
    args = ap.parse_args()
    import model  # noqa: F401
    res = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "warmup": args.warmup, "unit": "ms", "hbm_roof_bytes_per_s": HBM_ROOF,
           "decoders": {}, "kernels": {}}
    B, H, W = DECODER_SIZE
    tag = f"{H}x{W}_B{B}"
    res["saved_patch_matrix_bytes"] = {tag: saved_patch_bytes(B, H, W), "1024x2048_B2 (not run)": saved_patch_bytes(2, 1024, 2048)}
    for which in ("depth", "pose"):
        r = timed(decoder_legs(which, B, H, W), args.iters, args.warmup, f"{which} {tag}")
        res["decoders"][f"{which}/{tag}"] = r
        print(which, tag, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    for B, H, W in KERNEL_SIZES:
        tag = f"{H}x{W}_B{B}"
        for name, (legs, nbytes) in kernel_legs(B, H, W).items():
            r = timed(legs, args.iters, args.warmup, f"{name} {tag}")
            if "median" in r.get("hip", {}):
                r["algorithmic_bytes"] = nbytes
                r["hip_share_of_hbm_roof_by_call_time"] = nbytes / (r["hip"]["median"] * 1e-3) / HBM_ROOF
            res["kernels"][f"{name}/{tag}"] = r
            print(name, tag, json.dumps(r), flush=True)
            del legs
            torch.cuda.empty_cache()
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
