"""The optimizer step on the Swin-L OneFormer's real parameter set (shapes only, random gradients with a few NaN / inf planted), one GPU:

  (a) the reference's composition on torch -- torch.nan_to_num per parameter, clip_grad_norm_ over all of them, torch.optim.AdamW --
      in its foreach and its fused mode (the faster one is the baseline);
  (b) uenc.optim.FusedAdamW.step();

each with separate gradient tensors and with the flat layout of uenc.dp.GradBuckets.  Per leg: median / min / max device time per step
(events around the step), host enqueue time, kernel launches per step (counted by the profiler in one extra step), and the achieved
bytes/s against the traffic floor of 28 bytes per parameter for the update plus 4 for the norm.  One JSON line per leg.

    python tools/optim_bench.py --steps 30 --warmup 5
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

MAX_NORM = 0.01


def swin_l_shapes():
    from oracle import torch_ref as T
    return [tuple(s) for k, s in T.model_param_shapes(T.ModelCfg(swin=T.SWIN_L)).items() if "relative_position_index" not in k]


def make_params(shapes, dev):
    g = torch.Generator(device=dev).manual_seed(0)
    mod = torch.nn.Module()
    for i, s in enumerate(shapes):
        mod.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(s, device=dev, generator=g) * 0.02))
    return mod, [getattr(mod, f"p{i}") for i in range(len(shapes))]


def fill_grads(params, seed):
    g = torch.Generator(device=params[0].device).manual_seed(seed)
    for k, p in enumerate(params):
        p.grad.copy_(torch.randn(p.shape, device=p.device, generator=g) * 1e-3)
    params[3].grad.view(-1)[0] = float("nan")
    params[17].grad.view(-1)[-1] = float("inf")
    params[101].grad.view(-1)[5] = -float("inf")


def measure(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        step()
        b.record()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        dev_ms.append(a.elapsed_time(b))
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    return dev_ms, host_ms, launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: needs the GPU (a CPU run measures nothing of it)")
    from uenc.dp import GradBuckets
    from uenc.optim import FusedAdamW
    dev = torch.device("cuda", 0)
    shapes = swin_l_shapes()
    n_par = sum(int(torch.Size(s).numel()) for s in shapes)
    floor_bytes = 32 * n_par
    results = {}
    for layout in ("separate", "flat"):
        legs = [("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True)), ("fused_adamw", None)]
        for name, kw in legs:
            mod, params = make_params(shapes, dev)
            gb = None
            if layout == "flat":
                gb = GradBuckets(mod, listen_ops=False)           # points every .grad at its slice of the flat buffer
            else:
                for p in params:
                    p.grad = torch.zeros_like(p)
            fill_grads(params, 1)
            if kw is None:
                opt = FusedAdamW(params, lr=1e-4, weight_decay=0.05, max_grad_norm=MAX_NORM)
                step = opt.step
            else:
                opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.05, **kw)

                def step(opt=opt, params=params):
                    for p in params:
                        torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)
                    torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                    opt.step()
            dev_ms, host_ms, launches = measure(step, args.steps, args.warmup)
            med = statistics.median(dev_ms)
            rec = {"tool": "optim_bench", "layout": layout, "leg": name, "tensors": len(shapes), "parameters": n_par, "steps": args.steps,
                   "device_ms": {"median": round(med, 3), "min": round(min(dev_ms), 3), "max": round(max(dev_ms), 3)},
                   "host_enqueue_ms_median": round(statistics.median(host_ms), 3), "kernel_launches": launches,
                   "floor_bytes": floor_bytes, "achieved_TBps_vs_floor": round(floor_bytes / (med * 1e-3) / 1e12, 3)}
            print(json.dumps(rec), flush=True)
            results[(layout, name)] = med
            if gb is not None:
                gb.close()
            del opt, step, params, mod, gb
            torch.cuda.empty_cache()
    for layout in ("separate", "flat"):
        base = min(results[(layout, "torch_foreach")], results[(layout, "torch_fused")])
        print(json.dumps({"tool": "optim_bench", "layout": layout, "torch_best_ms": round(base, 3), "fused_adamw_ms": round(results[(layout, "fused_adamw")], 3),
                          "speedup": round(base / results[(layout, "fused_adamw")], 2)}), flush=True)
        if not results[(layout, "fused_adamw")] < base:
            raise SystemExit(f"optim_bench: FusedAdamW is not faster than torch's composition in the {layout} layout")


if __name__ == "__main__":
    main()
