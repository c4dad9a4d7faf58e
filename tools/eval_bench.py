"""The segmentation evaluators per 1024 x 2048 image, counting on the host against counting on the device (csrc/evalstats.hip).

  SemSegEvaluator.process    N = 19: (host) argmax on the GPU, int64 label map to the CPU, numpy bincount; (device) uenc_eval_confusion on
                             the (19, H, W) scores, ground truth uploaded as int32
  PanopticEvaluator.process  about 40 ground-truth and 40 predicted segments: (host) id map to the CPU, numpy unique + bincount + the
                             matching loop; (device) uenc_eval_pq_intersect + uenc_eval_pq_match, ground truth uploaded as int32

Legs alternate in one process; each call is timed with the host clock around the call and a device synchronise (`wall_ms`: the calls hold
host work and copies, which device events alone would miss) and, for the device legs, also without the synchronise (`issue_ms`: what
`inference_on_dataset` waits for before it loads the next batch).  Medians, minima and maxima over --iters after --warmup.  The three
kernels are timed alone with device events, with their algorithmic bytes (confusion: (C + 1) * 4 B per pixel, intersect: 8 B per pixel)
over the median as a share of the 8 TB/s HBM roof.  Before timing, both paths' results are compared for equality at the timed size.

    python tools/eval_bench.py --iters 10 --warmup 3 [--out profiles/eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    sys.path.insert(0, p)

HBM_ROOF = 8e12
THINGS = list(range(11, 19))


def annotation(rs, H, W, n_seg):
    """Nearest-site regions on a 16 x coarser grid, blown up: piecewise constant like a real panoptic map; one region is void (0), one
    listed segment is a crowd."""
    h, w = H // 16, W // 16
    yy, xx = np.mgrid[0:h, 0:w]
    cells = rs.choice(h * w, size=n_seg + 1, replace=False)
    d = (yy[None] - (cells // w)[:, None, None]) ** 2 + (xx[None] - (cells % w)[:, None, None]) ** 2
    cls = rs.randint(0, 19, n_seg)
    ids = [int(c) * 1000 + k if c >= 11 else 50 + k for k, c in enumerate(cls)]
    site = d.argmin(0)
    pan = np.ascontiguousarray(np.repeat(np.repeat(np.array(ids + [0], dtype=np.int32)[site], 16, 0), 16, 1))
    segs = [{"id": i, "category_id": int(c), "iscrowd": int(k == 3)} for k, (i, c) in enumerate(zip(ids, cls))]
    # the prediction: the same regions under ids 1.., moved by a few pixels, two regions merged into void, some classes wrong
    pred_ids = np.array([k + 1 if k % 17 else 0 for k in range(n_seg)] + [0], dtype=np.int32)
    pred = np.ascontiguousarray(np.roll(np.repeat(np.repeat(pred_ids[site], 16, 0), 16, 1), (5, -9), (0, 1)))
    info = [{"id": int(p), "isthing": bool(cls[k] >= 11), "category_id": int(cls[k] if k % 7 else (cls[k] + 1) % 19)}
            for k, p in enumerate(pred_ids[:-1]) if p]
    sem = np.full((h, w), 255, dtype=np.int64)
    sem[site < n_seg] = cls[site[site < n_seg]]
    return pan, segs, pred, info, np.repeat(np.repeat(sem, 16, 0), 16, 1)


def wall(legs, iters, warmup, sync=True):
    times = {k: [] for k in legs}
    for i in range(warmup + iters):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            if sync:
                torch.cuda.synchronize()
            if i >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    return {k: {"median": statistics.median(t), "min": min(t), "max": max(t)} for k, t in times.items()}


def events(legs, iters, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--segments", type=int, default=40)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench.py measures on the GPU"
    import model  # noqa: F401
    from uenc import kernels as K
    from uenc.evaluation import PQ_MAX_SEGMENTS, PanopticEvaluator, SemSegEvaluator
    torch.set_num_threads(1)
    rs = np.random.RandomState(0)
    H, W, N = a.height, a.width, a.classes
    pan, segs, pred, info, sem = annotation(rs, H, W, a.segments)
    pred_dev = torch.from_numpy(pred).cuda()
    onehot = torch.nn.functional.one_hot(torch.from_numpy(np.where(sem == 255, 0, sem)).cuda(), N).permute(2, 0, 1)
    scores = (torch.randn((N, H, W), device="cuda") + 3.0 * onehot).contiguous()
    inputs = [{"sem_seg_gt": sem, "pan_seg": pan, "segments_info": segs}]
    outputs = [{"sem_seg": scores, "panoptic_seg": (pred_dev, info)}]
    out = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "shape": [H, W], "classes": N,
           "segments": {"gt": len(segs), "pred": len(info)}, "unit": "ms"}

    for name, make in (("SemSegEvaluator.process", lambda acc: SemSegEvaluator(N, accumulate=acc)),
                       ("PanopticEvaluator.process", lambda acc: PanopticEvaluator(THINGS, 19, accumulate=acc))):
        evs = {acc: make(acc) for acc in ("host", "device")}
        results = {}
        for acc, ev in evs.items():                                      # the two paths agree at this size
            ev.process(inputs, outputs)
            results[acc] = ev.evaluate()
            ev.reset()
        assert results["host"] == results["device"], (name, results)
        legs = {acc: (lambda ev=ev: ev.process(inputs, outputs)) for acc, ev in evs.items()}
        res = {"identical_results": True, "result": next(iter(results["host"].values())), "wall_ms": wall(legs, a.iters, a.warmup)}
        for ev in evs.values():
            ev.reset()
        res["issue_ms"] = wall({"device": legs["device"]}, a.iters, a.warmup, sync=False)
        res["host_over_device"] = res["wall_ms"]["host"]["median"] / res["wall_ms"]["device"]["median"]
        out[name] = res

    # the three kernels alone (device events), tables as PanopticEvaluator packs them
    S = PQ_MAX_SEGMENTS
    table = np.zeros(5 * S + 4, dtype=np.int32)
    table[0:len(segs)], table[2 * S:2 * S + len(segs)] = [s["id"] for s in segs], [s["category_id"] for s in segs]
    table[3 * S:3 * S + len(segs)] = [s["iscrowd"] for s in segs]
    table[S:S + len(info)], table[4 * S:4 * S + len(info)] = [s["id"] for s in info], [s["category_id"] for s in info]
    table[5 * S:] = (len(segs), len(info), H, W)
    table = torch.from_numpy(table).cuda()
    gt_sem = torch.from_numpy(sem.astype(np.int32)).cuda()[None]
    gt_pan = torch.from_numpy(pan).cuda()[None]
    sizes = torch.tensor([[H, W]], dtype=torch.int32).cuda()
    conf = torch.zeros((N + 1, N + 1), dtype=torch.int64, device="cuda")
    inter = K.eval_pq_intersect(pred_dev[None], gt_pan, table)
    kt = events({"eval_confusion": lambda: K.eval_confusion(scores[None], gt_sem, sizes, conf, 255),
                 "eval_pq_intersect": lambda: K.eval_pq_intersect(pred_dev[None], gt_pan, table),
                 "eval_pq_match": lambda: K.eval_pq_match(inter, table, 19)}, a.iters, a.warmup)
    for k, nbytes in (("eval_confusion", (N + 1) * 4 * H * W), ("eval_pq_intersect", 8 * H * W)):
        kt[k]["algorithmic_bytes"] = nbytes
        kt[k]["TB_per_s"] = nbytes / (kt[k]["median"] * 1e-3) / 1e12
        kt[k]["share_of_8TBps_roof"] = nbytes / (kt[k]["median"] * 1e-3) / HBM_ROOF
    kt["eval_pq_intersect"]["note"] = "includes the zero-fill of the (1, 258, 258) matrix"
    kt["eval_pq_match"]["note"] = "one workgroup per image: latency, not bandwidth"
    out["kernels_event_ms"] = kt

    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
