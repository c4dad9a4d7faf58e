"""The depth evaluators per image, scoring on the host against scoring on the device (csrc/ext/depth_eval.hip), at the two sizes they meet:

  KITTI       192 x 640 disparity  -> 375 x 1242 ground truth (fp64, about 5 % of the pixels hit by the scan), Eigen crop
  Cityscapes  512 x 1024 disparity -> 1024 x 2048 ground truth (.npy, fp32), lower quarter cut, window [256:, 192:1856]

What is timed.  The host path only collects in `process` and scores in `evaluate`, so its cost per image is process + evaluate of that
one image (copy of the disparity to the host, CPU resize, masks, two medians, seven metrics); the device path's is `process` alone
(upload of the ground truth, uenc_depth_eval_pred, uenc_depth_eval_score), its `evaluate` is one read-back per dataset and is timed
apart.  KITTI's velodyne projection (`generate_depth_map`) is host work common to both paths and is replaced by a precomputed map;
Cityscapes reads its .npy from a temporary directory on both paths.  Legs alternate in one process; `wall_ms` is the host clock around
the call and a device synchronise, `issue_ms` the device leg without the synchronise; medians, minima and maxima over --iters after
--warmup.  The two kernels' entry points are timed alone with device events; a score is one memset and DEPTH_EVAL_LAUNCHES kernels, so the
time per launch is the median over their number.  Host memory: the bytes held in the evaluator and the growth of the process's resident
set after --images images on each path.  Before timing, both paths' results are compared at the timed size.

    python tools/depth_eval_bench.py --iters 10 --warmup 3 [--out profiles/depth_eval_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd")):
    sys.path.insert(0, p)


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


def resident_bytes():
    with open("/proc/self/statm") as f:
        return int(f.read().split()[1]) * os.sysconf("SC_PAGE_SIZE")


def held_bytes(ev):
    return sum(a.nbytes for pair in ev._pairs for a in pair)


def scene(rs, H, W, h, w, density, dtype):
    """A smooth depth field with noise; ground truth = the field where the scan hits, 0 elsewhere; the prediction = the field at the
    disparity's size under multiplicative log-normal noise (sigma 0.2) and half the scale, as a sigmoid disparity."""
    yy, xx = np.mgrid[0:H, 0:W]
    field = 5.0 + 70.0 * (1.0 - yy / H) ** 2 + 3.0 * np.sin(xx / 97.0)
    gt = np.where(rs.uniform(size=(H, W)) < density, field, 0.0).astype(dtype)
    ys, xs = ((np.arange(h) + 0.5) * H / h).astype(int), ((np.arange(w) + 0.5) * W / w).astype(int)
    depth = field[ys][:, xs] * np.exp(rs.normal(0.0, 0.2, (h, w))) * 0.5
    disp = np.ascontiguousarray((1.0 / depth - 0.01) / (10.0 - 0.01), dtype=np.float32)
    return gt, disp


def measure(name, evs, inputs, outputs, outputs_dev, a, K, gt, disp, window):
    from uenc.evaluation import disp_to_depth
    res = {}
    results = {}
    for acc, ev in evs.items():
        ev.reset()
        ev.process(inputs, outputs_dev if acc == "device" else outputs)
        results[acc] = ev.evaluate()["depth_error"]
        ev.reset()
    rel = {k: abs(results["device"][k] - results["host"][k]) / abs(results["host"][k]) for k in results["host"]}
    assert max(rel.values()) < 1e-3, (name, results)
    res["result"] = {acc: dict(r) for acc, r in results.items()}
    res["device_against_host_relative"] = rel

    def host_leg(ev=evs["host"]):
        ev.process(inputs, outputs_dev)              # the model leaves its outputs on the device on both paths
        ev.evaluate()
        ev.reset()
    dev = evs["device"]
    res["wall_ms"] = wall({"host": host_leg, "device": lambda: dev.process(inputs, outputs_dev)}, a.iters, a.warmup)
    n_dev = dev._dev_count
    res["device_evaluate_ms"] = wall({"evaluate": dev.evaluate}, a.iters, a.warmup)["evaluate"]
    res["device_evaluate_ms"]["rows_read_back"] = n_dev
    dev.reset()
    res["issue_ms"] = wall({"device": lambda: dev.process(inputs, outputs_dev)}, a.iters, a.warmup, sync=False)["device"]
    dev.reset()
    res["images_per_process_call"] = int(outputs[0]["disp_results"].shape[0]) if outputs[0]["disp_results"].dim() == 4 else 1
    res["host_over_device"] = res["wall_ms"]["host"]["median"] / res["wall_ms"]["device"]["median"]
    res["device_loses"] = bool(res["host_over_device"] < 1.0)

    # the kernels alone
    gt_dev = torch.from_numpy(np.ascontiguousarray(gt)).cuda()
    sd = disp_to_depth(torch.from_numpy(disp).cuda())[0].contiguous()
    H, W = gt_dev.shape
    rows = torch.zeros((1, K.DEPTH_EVAL_ROW), dtype=torch.float64, device="cuda")
    ws = K.depth_eval_ws(H, W, "cuda")
    pred = K.depth_eval_pred(sd, (H, W))
    kt = events({"depth_eval_pred": lambda: K.depth_eval_pred(sd, (H, W)),
                 "depth_eval_score": lambda: K.depth_eval_score(gt_dev, pred, window, 1e-3, 80, rows, 0, ws)}, a.iters, a.warmup)
    launches = K.DEPTH_EVAL_LAUNCHES[gt_dev.dtype]
    kt["depth_eval_pred"].update(launches=1, note="includes the allocation of the (H, W) output by the wrapper")
    kt["depth_eval_score"].update(launches=launches + 1, kernels=launches, memsets=1, ms_per_launch=kt["depth_eval_score"]["median"] / (launches + 1),
                                  window=list(window), window_pixels=(window[1] - window[0]) * (window[3] - window[2]), gt_dtype=str(gt_dev.dtype))
    res["kernels_event_ms"] = kt
    res["launches_per_image"] = launches + 2

    # host memory after a.images images
    mem = {}
    for acc, ev in evs.items():
        ev.reset()
        torch.cuda.synchronize()
        before = resident_bytes()
        calls = max(1, a.images // res["images_per_process_call"])
        for _ in range(calls):
            ev.process(inputs, outputs_dev)
        torch.cuda.synchronize()
        mem[acc] = {"images": calls * res["images_per_process_call"], "held_in_evaluator_bytes": held_bytes(ev),
                    "resident_set_growth_bytes": resident_bytes() - before,
                    "device_rows_bytes": 0 if ev._dev_rows is None else ev._dev_rows.numel() * 8}
        ev.reset()
    res["host_memory"] = mem
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "depth_eval_bench.py measures on the GPU"
    import model  # noqa: F401
    from uenc import kernels as K
    from uenc.evaluation import CityscapesDepthEvaluator, KITTIDepthEvaluator
    rs = np.random.RandomState(0)
    out = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "unit": "ms", "torch_threads": torch.get_num_threads(),
           "host_leg": "process + evaluate of the one image", "device_leg": "process"}

    # KITTI: the projection is common to both paths and replaced by a precomputed map
    gt, disp = scene(rs, 375, 1242, 192, 640, 0.05, np.float64)

    class Kitti(KITTIDepthEvaluator):
        @classmethod
        def generate_depth_map(cls, *args, **kw):
            return gt
    inputs = [{"calib_path": "", "velo_file": "", "file_name": "a/b/c/d.jpg"}]
    outputs = [{"disp_results": torch.from_numpy(disp)[None, None]}]
    outputs_dev = [{"disp_results": outputs[0]["disp_results"].cuda()}]
    crop = tuple(int(v) for v in KITTIDepthEvaluator._eigen_crop(375, 1242))
    out["kitti_192x640_to_375x1242"] = measure("kitti", {acc: Kitti("x", accumulate=acc) for acc in ("host", "device")}, inputs, outputs,
                                               outputs_dev, a, K, gt, disp, crop)

    # Cityscapes: the .npy beside the image, batch 1
    gt, disp = scene(rs, 1024, 2048, 512, 1024, 0.9, np.float32)
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "gt_depths", "berlin"))
        np.save(os.path.join(d, "gt_depths", "berlin", "berlin_000000_000019.npy"), gt)
        inputs = [{"file_name": d + "/leftImg8bit/test/berlin/berlin_000000_000019.png"}]
        outputs = [{"disp_results": torch.from_numpy(disp)[None, None]}]
        outputs_dev = [{"disp_results": outputs[0]["disp_results"].cuda()}]
        out["cityscapes_512x1024_to_1024x2048"] = measure(
            "cityscapes", {acc: CityscapesDepthEvaluator("x", accumulate=acc) for acc in ("host", "device")}, inputs, outputs, outputs_dev, a, K,
            gt[:768], disp, (256, 768, 192, 1856))

    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
