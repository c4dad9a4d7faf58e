"""The set criterion at Swin-L head shapes: batch 2, Q 150, 19 classes, mask logits 256 x 512 (targets 1024 x 2048), 10 heads, 20 targets per
image, P 12 544 points with oversample ratio 3.0 and importance ratio 0.75 (M 37 632, 9 408 + 3 136).

Legs, all on the same inputs, indices and injected point draws, forward + backward each (gradients to every head's pred_masks / pred_logits):
  torch     the composition of the criterion's arithmetic with torch ops on the same GPU (SetCriterion._forward_torch: gathers, grid_sample
            twice per head, top-k, BCE, dice, cross entropy, autograd), given the indices
  hip       csrc/criterion.hip through SetCriterion, given the indices
  hip_all   match_all(solver="device") + the criterion + backward, nothing read back
The torch and hip legs alternate inside one loop.  Parts of the hip leg (point logits + top-k + gather, the forward kernel, the stable sort
of the tap keys, the backward kernel with its zero fill, the class loss) are timed on their own the same way.  Device time between two
events, median / min / max over --iters; the losses and gradients of both legs are compared at this shape.  Prints one JSON line.

    python tools/criterion_bench.py [--iters 15] [--small] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_inputs(a, dev):
    g = torch.Generator().manual_seed(0)
    h, w = a.height // 4, a.width // 4
    heads = [{"pred_logits": torch.randn(a.batch, a.queries, a.classes + 1, generator=g).to(dev).requires_grad_(True),
              "pred_masks": (torch.randn(a.batch, a.queries, h, w, generator=g) * 3).to(dev).requires_grad_(True)} for _ in range(a.heads)]
    targets = []
    for b in range(a.batch):
        masks = torch.zeros(a.targets, a.height, a.width, dtype=torch.bool)
        for t in range(a.targets):                       # random boxes: segments with an extent, cheap to draw
            y0, x0 = int(torch.randint(0, a.height // 2, (1,), generator=g)), int(torch.randint(0, a.width // 2, (1,), generator=g))
            dy, dx = int(torch.randint(8, a.height // 2, (1,), generator=g)), int(torch.randint(8, a.width // 2, (1,), generator=g))
            masks[t, y0:y0 + dy, x0:x0 + dx] = True
        targets.append({"labels": torch.randint(0, a.classes, (a.targets,), generator=g).to(dev), "masks": masks.to(dev)})
    return heads, targets


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def stat(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-300))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--small", action="store_true", help="a few seconds on any GPU: 64 x 96 images, 400 points, 3 heads")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    a.queries, a.classes, a.batch, a.targets = 150, 19, 2, 20
    a.height, a.width, a.points, a.heads = (64, 96, 400, 3) if a.small else (1024, 2048, 12544, 10)

    import model  # noqa: F401
    from uenc import kernels as K
    from uenc.modeling.criterion import SetCriterion, _flat
    from uenc.modeling.matcher import HungarianMatcher, _mask_bytes
    if not torch.cuda.is_available():
        raise SystemExit("criterion_bench needs the GPU")
    dev = torch.device("cuda")
    heads, targets = make_inputs(a, dev)
    outputs = dict(heads[0], aux_outputs=heads[1:])
    base = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    weights = dict(base)
    for i in range(a.heads - 1):
        weights.update({f"{k}_{i}": v for k, v in base.items()})
    crit = SetCriterion(a.classes, HungarianMatcher(2.0, 5.0, 5.0, num_points=a.points), weights, 0.1, ["labels", "masks"], a.points, 3.0, 0.75).to(dev)
    M, n_unc, n_rnd = crit.point_counts()
    N = a.batch * min(a.queries, a.targets)
    g = torch.Generator().manual_seed(1)
    draws = {"oversampled": torch.rand(a.heads, N, M, 2, generator=g).to(dev), "random": torch.rand(a.heads, N, n_rnd, 2, generator=g).to(dev)}
    mpts = torch.rand(a.heads, a.batch, a.points, 2, generator=g).to(dev)
    indices = crit.matcher.match_all(outputs, targets, point_coords=mpts, solver="device")
    leaves = [v for hd in heads for v in hd.values()]

    def grads():
        out = [v.grad for v in leaves]
        for v in leaves:
            v.grad = None
        return out

    def leg_torch():
        per = crit._forward_torch(heads, targets, indices, draws["oversampled"], draws["random"], float(a.batch * a.targets), N)
        losses = dict(per[0])
        for i, r in enumerate(per[1:]):
            losses.update({f"{k}_{i}": v for k, v in r.items()})
        crit.weighted_sum(losses).backward()
        return losses

    def leg_hip():
        losses = crit(outputs, targets, indices=indices, point_draws=draws)
        crit.weighted_sum(losses).backward()
        return losses

    def leg_hip_all():
        idx = crit.matcher.match_all(outputs, targets, point_coords=mpts, solver="device")
        losses = crit(outputs, targets, indices=idx, point_draws=draws)
        crit.weighted_sum(losses).backward()
        return losses

    # agreement of the two legs at this shape
    lt = {k: float(v.detach()) for k, v in leg_torch().items()}
    gt = grads()
    lh = {k: float(v.detach()) for k, v in leg_hip().items()}
    gh = grads()
    parity = {"loss_max_rel": max(abs(lh[k] - lt[k]) / max(abs(lt[k]), 1e-30) for k in lt),
              "grad_masks_max_rel_l2": max(rel(x, y) for x, y in zip(gh[1::2], gt[1::2])),
              "grad_logits_max_rel_l2": max(rel(x, y) for x, y in zip(gh[0::2], gt[0::2]))}

    legs = {"torch": leg_torch, "hip": leg_hip, "hip_all": leg_hip_all}
    for fn in legs.values():                             # warm-up of every leg
        for _ in range(2):
            fn()
            grads()
    times = {k: [] for k in legs}
    for _ in range(a.iters):
        for name, fn in legs.items():                    # alternating
            ms, _ = timed(fn)
            grads()
            times[name].append(ms)

    # the parts of the hip leg
    call = K.CritCall([hd["pred_masks"].detach() for hd in heads], [hd["pred_logits"].detach() for hd in heads],
                      [_mask_bytes(t["masks"]) for t in targets], [t["labels"] for t in targets])
    row = _flat([p[0] for head in indices for p in head], dev)
    col = _flat([p[1] for head in indices for p in head], dev)
    R = a.heads * N
    over, rnd = draws["oversampled"].view(R, M, 2), draws["random"].view(R, n_rnd, 2)
    ones = torch.ones(a.heads, device=dev)
    points = crit._select_hip(call, row, draws["oversampled"], draws["random"])
    _, _, unit, keys = K.crit_mask_loss_fwd(call, row, col, points)
    skeys, order = torch.sort(keys, dim=1, stable=True)
    parts = {"point_logits": lambda: K.crit_point_logits(call, row, over),
             "select_points(point_logits+topk+gather+cat)": lambda: crit._select_hip(call, row, draws["oversampled"], draws["random"]),
             "mask_loss_fwd": lambda: K.crit_mask_loss_fwd(call, row, col, points),
             "stable_sort": lambda: torch.sort(keys, dim=1, stable=True),
             "mask_loss_bwd(zero fill+kernel)": lambda: K.crit_mask_loss_bwd(call, row, points, unit, skeys, order, ones, ones, 1.0 / (a.batch * a.targets)),
             "class_loss": lambda: K.crit_class_loss(call, row, col, 0.1)}
    ptimes = {k: [] for k in parts}
    for fn in parts.values():
        fn()
    for _ in range(a.iters):
        for name, fn in parts.items():
            ptimes[name].append(timed(fn)[0])

    med = {k: statistics.median(v) for k, v in times.items()}
    result = {"bench": "criterion", "shape": {k: getattr(a, k) for k in ("queries", "classes", "heads", "batch", "targets", "height", "width", "points")},
              "pairs_per_head": N, "oversampled_points": M, "kept_by_uncertainty": n_unc, "iters": a.iters,
              "event_ms": {k: stat(v) for k, v in times.items()}, "hip_parts_event_ms": {k: stat(v) for k, v in ptimes.items()},
              "torch_over_hip": round(med["torch"] / med["hip"], 3),
              "stable_sort_share_of_hip": round(statistics.median(ptimes["stable_sort"]) / med["hip"], 3),
              "hip_vs_torch_at_this_shape": parity,
              "saved_for_backward_mib": round((unit.numel() * 4 + keys.numel() * 4 + points.numel() * 4) / 2 ** 20, 1),
              "sort_transient_mib": round((skeys.numel() * 4 + order.numel() * 8) / 2 ** 20, 1),
              "peak_memory_mib": round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
