"""MonodepthLoss forward + backward, full flag set, at the reference's training crop (192 x 512, 3 images) on one GPU: the fused kernel path
against the module's torch composition (the reference's op sequence), alternating the two legs in one process.  Prints one JSON line:
median / min / max device ms per leg, the kernel launches of one call of each leg (torch profiler), and whether the difference exceeds the
spread measured in this same run.

    python tools/monodepth_bench.py --iters 20 --warmup 5 [--out profiles/monodepth_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    sys.path.insert(0, p)


def make_inputs(B, H, W, dev):
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.rand(*s, generator=g)
    outputs, leaves = {}, []

    def leaf(t):
        t = t.to(dev).requires_grad_(True)
        leaves.append(t)
        return t

    for s in range(4):
        h, w = H >> s, W >> s
        outputs[("disp", 0, s)] = leaf(0.1 + 0.5 * r(B, 1, h, w))
        for f in (-1, 1):
            outputs[("complete_flow", f, s)] = leaf(0.05 * (r(B, 3, h, w) - 0.5))
            outputs[("motion_mask", f, s)] = leaf(r(B, 1, h, w))
            outputs[("motion_prob", f, s)] = leaf(2 * r(B, 1, h, w) - 1)
    for f in (-1, 1):
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, :3, 3] = 0.1 * f * (r(B, 3) - 0.3)
        T[:, 0, 2], T[:, 2, 0] = 0.03 * f, -0.03 * f
        outputs[("cam_T_cam", 0, f)] = leaf(T)
    K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    inv_K = torch.linalg.inv(K)
    imgs = {f: r(B, 3, H, W).to(dev) for f in (-1, 0, 1)}
    targets = [dict({("color", f, 0): imgs[f][b] for f in imgs}, K=K.to(dev), inv_K=inv_K.to(dev)) for b in range(B)]
    return outputs, targets, leaves


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "monodepth_bench.py measures on the GPU"
    import model  # noqa: F401
    from uenc.modeling.monodepth_loss import MonodepthLoss
    B, H, W, dev = 3, 192, 512, "cuda"
    ns = types.SimpleNamespace
    cfg = ns(SOLVER=ns(IMS_PER_BATCH=B), DATASETS=ns(TRAIN=("kitti",)), INPUT=ns(DEPTH_CROP=ns(SIZE=(H, W))), MODEL=ns(DEVICE=dev))
    flags = dict(bool_MotMask=True, bool_CmpFlow=True, bool_automask=True, move_Depth=True, move_CmpFlow=True, move_MotMask=True,
                 step=40000, phrage="finetune")
    outputs, targets, leaves = make_inputs(B, H, W, dev)
    legs = {name: MonodepthLoss(cfg, **flags, impl=name) for name in ("torch", "kernels")}
    g = torch.Generator(device=dev).manual_seed(1)
    noise = list(torch.randn(4, B, 2, H, W, generator=g, device=dev))
    ground = [torch.randint(0, int(0.4 * (H >> s)) * (W >> s), (B, 500), generator=g, device=dev) for s in range(4)]

    def call(name):
        loss = legs[name](dict(outputs), targets, tie_noise=noise, ground_samples=ground)["loss_monodepth"]
        return loss, torch.autograd.grad(loss, leaves)

    res = {name: call(name) for name in legs}
    torch.cuda.synchronize()
    lt, lk = float(res["torch"][0]), float(res["kernels"][0])
    worst = max(float((x - y).norm() / y.norm().clamp(min=1e-30)) for x, y in zip(res["kernels"][1], res["torch"][1]))
    times = {name: [] for name in legs}
    for i in range(a.warmup + a.iters):
        for name in legs:                                  # alternate the legs
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(name)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    launches = {}
    for name in legs:
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            call(name)
            torch.cuda.synchronize()
        launches[name] = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    out = {"shape": {"B": B, "H": H, "W": W, "flags": "full"}, "iters": a.iters, "warmup": a.warmup, "launches": launches,
           "loss": {"torch": lt, "kernels": lk}, "worst_grad_rel_l2_kernels_vs_torch": worst}
    for name, t in times.items():
        out[name + "_ms"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    spread = max(out[n + "_ms"]["max"] - out[n + "_ms"]["min"] for n in legs)
    out["spread_ms"] = spread
    out["kernels_faster_by_more_than_spread"] = out["torch_ms"]["median"] - out["kernels_ms"]["median"] > spread
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
