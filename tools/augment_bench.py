"""The training-time augmentation of one sample, finished on the host (PIL + numpy, the reference's method) against finished on the device
(csrc/augment.hip), upload included.

One synthetic 1024 x 2048 sample of the base configuration: four frames, a panoptic PNG, a label map, SSD colour on (every stage), crop
512 x 1024, at the shortest-edge choices 512, 1024 and 2048 (SEG_MIN_SIZE_TRAIN's range on Cityscapes).  The plan is fixed per size: the
crop window in the middle, no flip, so both legs do the same work every iteration.

  host     uenc.train_data.apply_plan_host: resize every full frame, crop, colour, pad.  Its colour stage is the numpy restatement of
           OpenCV's 8-bit HSV conversions, which is slower than cv2 itself would be: `host_without_colour` is the same leg with the
           colour augmentation off (PIL resize, crop, the label gathers), the part of the host cost that does not depend on that
  device   uenc.train_data.apply_plan_device: pack the tables and the untouched sources into one buffer, one upload, two launches,
           then a device synchronise (the host clock needs it; training does not wait there).  `device_pack_only` is the packing
           alone (the mapper does it, in a DataLoader worker when there are workers) and `device_upload_and_launch` what is left for
           the main process (`apply_plans`)

Legs alternate in one process; each call is timed with the host clock around the call and a device synchronise.  Medians, minima and
maxima over --iters after --warmup.  The two kernels are timed alone with device events on a buffer that is already on the device, with
their algorithmic bytes (image: the window's source rectangle of every frame read once + 3 B per output pixel written; labels: the
distinct source pixels the window gathers, 3 + 1 B each, + 8 B per output pixel) over the median as a share of the 8 TB/s HBM roof.
Before timing, both paths' results are compared for equality at the timed size.

    python tools/augment_bench.py --iters 10 --warmup 2 [--out profiles/augment_bench.json]
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
H, W, CROP = 1024, 2048, (512, 1024)


def sample(rs):
    """Smooth frames (a coarse random field blown up, plus noise: PNG-like content, not white noise) and piecewise-constant annotations."""
    frames = []
    for _ in range(4):
        coarse = rs.randint(0, 256, (H // 32, W // 32, 3)).astype(np.float32)
        img = np.repeat(np.repeat(coarse, 32, 0), 32, 1) + rs.randint(-12, 13, (H, W, 3))
        frames.append(np.clip(img, 0, 255).astype(np.uint8))
    cells = rs.randint(0, 40, (H // 64, W // 64))
    cls = rs.randint(0, 19, 40)
    ids = np.array([int(c) * 1000 + k if c >= 11 else int(c) for k, c in enumerate(cls)])
    big = np.repeat(np.repeat(cells, 64, 0), 64, 1)
    pid = ids[big]
    pan = np.stack([pid & 255, (pid >> 8) & 255, (pid >> 16) & 255], -1).astype(np.uint8)
    return frames, pan, cls[big].astype(np.uint8)


def stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def wall(legs, iters, warmup):
    times = {k: [] for k in legs}
    for i in range(warmup + iters):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in times.items()}


def events(fn, iters, warmup):
    ts = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ts.append(a.elapsed_time(b))
    return stats(ts)


def algorithmic_bytes(plan, T):
    (h, w), (nh, nw), (x0, y0, cw, ch), (oh, ow) = plan.src_hw, plan.resized_hw, plan.crop, plan.out_hw
    cf, cc, _ = T.pil_bilinear_coeffs(w, nw)
    rf, rc, _ = T.pil_bilinear_coeffs(h, nh)
    rect = (int((rf + rc)[y0:y0 + ch].max()) - int(rf[y0:y0 + ch].min())) * (int((cf + cc)[x0:x0 + cw].max()) - int(cf[x0:x0 + cw].min()))
    image = 4 * (rect * 3 + 3 * oh * ow)
    rows = len(np.unique(T.pil_nearest_table(h, nh)[y0:y0 + ch]))
    cols = len(np.unique(T.pil_nearest_table(w, nw)[x0:x0 + cw]))
    labels = rows * cols * 4 + 8 * oh * ow
    return image, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench.py measures on the GPU; there is no CPU fallback"
    from uenc import kernels as K
    from uenc import train_data as T

    frames, pan, label = sample(np.random.RandomState(0))
    colour = T.ColourParams(12.5, True, 1.25, 0.8, 9, True)
    out = {"source": [H, W], "crop": list(CROP), "frames": 4, "colour": "brightness, contrast, saturation, hue", "sizes": {}}
    for size in (512, 1024, 2048):
        nh, nw = T.ResizeShortestEdge.get_output_shape(H, W, size, 4096)
        ch, cw = min(CROP[0], nh), min(CROP[1], nw)
        plan = T.AugPlan((H, W), (nh, nw), ((nw - cw) // 2, (nh - ch) // 2, cw, ch), False, (ch, cw), colour)
        host = T.apply_plan_host(plan, frames, pan, label)
        dev = T.apply_plan_device(plan, frames, pan, label, "cuda")
        torch.cuda.synchronize()
        equal = all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(host, dev))
        assert equal, f"size {size}: the device path differs from the host path"
        plain = T.AugPlan(plan.src_hw, plan.resized_hw, plan.crop, False, plan.out_hw, None)
        res = wall({"host": lambda: T.apply_plan_host(plan, frames, pan, label),
                    "host_without_colour": lambda: T.apply_plan_host(plain, frames, pan, label),
                    "device": lambda: T.apply_plan_device(plan, frames, pan, label, "cuda")}, args.iters, args.warmup)
        buf, off, meta = T.pack_plan(plan, frames, pan, label)
        res["device_pack_only"] = wall({"pack": lambda: T.pack_plan(plan, frames, pan, label)}, args.iters, args.warmup)["pack"]
        res["device_upload_and_launch"] = wall({"u": lambda: T.apply_packed(plan, buf, off, meta, "cuda")}, args.iters, args.warmup)["u"]
        dbuf = buf.cuda()
        b_img, b_lab = algorithmic_bytes(plan, T)
        for name, fn, nbytes in (("kernel_image", lambda: K.augment_image(dbuf, off, meta, plan), b_img),
                                 ("kernel_labels", lambda: K.augment_labels(dbuf, off, meta, plan), b_lab)):
            r = events(fn, args.kernel_iters, 5)
            r["algorithmic_bytes"] = nbytes
            r["share_of_hbm_roof"] = nbytes / HBM_ROOF / (r["median_ms"] * 1e-3)
            res[name] = r
        res["upload_bytes"] = int(buf.numel())
        res["resized"] = [nh, nw]
        res["equal"] = equal
        res["host_over_device"] = res["host"]["median_ms"] / res["device"]["median_ms"]
        out["sizes"][str(size)] = res
        print(size, json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
