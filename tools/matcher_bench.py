"""Matching at Swin-L head shapes: Q 150, mask logits 256 x 512 (targets 1024 x 2048), P 12 544, batch 2, 10 heads, T 20 and 60.

Three legs over the same inputs and points, one `match_all` (= 20 problems) each:
  (a) torch   the reference's composition restated with torch ops on the same GPU (two grid_samples, two BCE maps, three einsums,
              softmax, gather), a copy of each cost matrix and scipy, per head and image as the reference calls its matcher;
  (b) host    uenc_match_cost, one copy of all matrices, scipy per problem;
  (c) device  uenc_match_cost + uenc_lsap_solve, nothing read back.
Per leg: device time between two events and host wall time (call until results are usable on the host side: (a), (b) return CPU
indices; (c) is timed to the end of a synchronize), median and range over --iters calls, and the number of GPU kernel launches of one
call (torch.profiler).  Prints one JSON line.

    python tools/matcher_bench.py [--iters 20] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_inputs(args, dev):
    g = torch.Generator().manual_seed(0)
    Q, C1, h, w = args.queries, args.classes + 1, args.height // 4, args.width // 4
    heads = [{"pred_logits": torch.randn(args.batch, Q, C1, generator=g).to(dev), "pred_masks": (torch.randn(args.batch, Q, h, w, generator=g) * 3).to(dev)}
             for _ in range(args.heads)]
    targets = []
    for b in range(args.batch):
        T = args.targets[b % len(args.targets)]
        masks = torch.zeros(T, args.height, args.width, dtype=torch.bool)
        for t in range(T):                               # random boxes: segments with an extent, cheap to draw
            y0, x0 = int(torch.randint(0, args.height // 2, (1,), generator=g)), int(torch.randint(0, args.width // 2, (1,), generator=g))
            dy, dx = int(torch.randint(8, args.height // 2, (1,), generator=g)), int(torch.randint(8, args.width // 2, (1,), generator=g))
            masks[t, y0:y0 + dy, x0:x0 + dx] = True
        targets.append({"labels": torch.randint(0, args.classes, (T,), generator=g).to(dev), "masks": masks.to(dev)})
    points = torch.rand(args.heads, args.batch, args.points, 2, generator=g).to(dev)
    return dict(heads[0], aux_outputs=heads[1:]), targets, points


def torch_leg(matcher, outputs, targets, points):
    """The reference's composition, per head and image, with torch ops on the GPU and scipy on the host."""
    from uenc.modeling.matcher import linear_sum_assignment_with_nan
    heads = [outputs] + list(outputs["aux_outputs"])
    res = []
    for i, hd in enumerate(heads):
        per = []
        for b in range(hd["pred_logits"].shape[0]):
            C = matcher._cost_torch(hd["pred_logits"][b], hd["pred_masks"][b], targets[b]["masks"], targets[b]["labels"], points[i][b])
            r, c = linear_sum_assignment_with_nan(C.cpu().numpy())
            per.append((torch.as_tensor(r, dtype=torch.int64), torch.as_tensor(c, dtype=torch.int64)))
        res.append(per)
    return res


def measure(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(e0.elapsed_time(e1))
    stat = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa: E731
    return {"event_ms": stat(dev_ms), "wall_ms": stat(wall_ms)}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--small", action="store_true", help="a few seconds on any GPU: 64 x 96 images, 400 points")
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    args.queries, args.classes, args.heads, args.batch, args.targets = 150, 133, 10, 2, (20, 60)
    args.height, args.width, args.points = (64, 96, 400) if args.small else (1024, 2048, 12544)

    import model  # noqa: F401
    from uenc.modeling.matcher import HungarianMatcher
    dev = torch.device("cuda")
    outputs, targets, points = make_inputs(args, dev)
    m = HungarianMatcher(2.0, 5.0, 5.0, num_points=args.points)
    legs = {"torch": lambda: torch_leg(m, outputs, targets, points),
            "host": lambda: m.match_all(outputs, targets, point_coords=points, solver="host"),
            "device": lambda: m.match_all(outputs, targets, point_coords=points, solver="device")}
    ref = legs["torch"]()
    agree = {}
    for name in ("host", "device"):
        got = legs[name]()
        agree[name] = sum(torch.equal(a.cpu(), b) for hg, hr in zip(got, ref) for pg, pr in zip(hg, hr) for a, b in zip(pg, pr))
    result = {"bench": "matcher", "shape": {k: getattr(args, k) for k in ("queries", "classes", "heads", "batch", "targets", "height", "width", "points")},
              "problems": args.heads * args.batch, "index_tensors_equal_to_torch_leg": agree, "index_tensors": 2 * args.heads * args.batch}
    for name, fn in legs.items():
        result[name] = measure(fn, args.iters)
        if not args.no_launch_count:
            result[name]["gpu_kernel_launches"] = launches(fn)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
