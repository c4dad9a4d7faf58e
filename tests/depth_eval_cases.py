"""Shared cases of the depth-evaluation tests and a float64 numpy restatement of what csrc/ext/depth_eval.hip computes, written from the
specification of the two stages and not by calling the code under test (TEST INFRASTRUCTURE).

Stage 1 (`resize_f64`, `pred_f32`): bilinear taps at half-pixel centres, src = (dst + 0.5) * in / out - 0.5 clamped at 0, second tap
clamped at in - 1; coordinate, weights and the three lerps in float64 from the fp32 taps; one rounding to fp32; pred = 1.0f / that.
Stage 2 (`score_f64`): valid = inside the window and MIN < gt < MAX in gt's own precision; numpy's median (rank (n - 1) / 2 for odd n,
mean of ranks n / 2 - 1 and n / 2 for even n), the ground truth's in float64, the prediction's in fp32 as (a + b) * 0.5f;
p = clip(pred * med_gt / med_pred, MIN, MAX) and the seven metrics of `compute_errors` in float64."""
import os

import numpy as np

MIN_DEPTH, MAX_DEPTH = 1e-3, 80
THRESHOLDS = (1.25, 1.25 ** 2, 1.25 ** 3)

# (h, w) -> (H, W): upscale with a non-integer ratio, downscale, the fixture camera, identity, every tap clamped
PRED_SHAPES = [((5, 7), (13, 18)), ((33, 50), (16, 21)), ((12, 40), (40, 120)), ((9, 9), (9, 9)), ((1, 1), (4, 4))]


def _taps(out, inn):
    s = (np.arange(out, dtype=np.float64) + 0.5) * (np.float64(inn) / np.float64(out)) - 0.5
    s = np.maximum(s, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), inn - 1)
    return i0, np.minimum(i0 + 1, inn - 1), s - i0


def resize_f64(disp, H, W):
    """(h, w) fp32 -> (H, W) float64, not yet rounded."""
    assert disp.dtype == np.float32
    y0, y1, wy = _taps(H, disp.shape[0])
    x0, x1, wx = _taps(W, disp.shape[1])
    d = disp.astype(np.float64)
    top = d[y0][:, x0] * (1.0 - wx) + d[y0][:, x1] * wx
    bot = d[y1][:, x0] * (1.0 - wx) + d[y1][:, x1] * wx
    return top * (1.0 - wy)[:, None] + bot * wy[:, None]


def pred_f32(disp, H, W):
    """-> (resized disparity fp32, predicted depth fp32 = 1.0f / resized)."""
    r = resize_f64(disp, H, W).astype(np.float32)
    with np.errstate(divide="ignore"):
        return r, (np.float32(1.0) / r).astype(np.float32)


def ulp32(x):
    """The spacing of fp32 at |x|."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


def _median(v, acc):
    s = np.sort(v)
    n = len(s)
    a, b = s[(n - 1) // 2], s[n // 2]
    return acc(a) if n % 2 else (acc(a) + acc(b)) * acc(0.5)


def score_f64(gt, pred, window, lo=MIN_DEPTH, hi=MAX_DEPTH):
    """-> dict(row = the seven metrics, n, med_gt (float64), med_pred (fp32), counts = the three threshold counts).  pred is fp32 as the
    kernel takes it; float64 predictions (the reference's recorded pairs) are scored with their median in float64."""
    assert pred.dtype in (np.float32, np.float64) and gt.dtype in (np.float32, np.float64) and gt.shape == pred.shape
    r0, r1, c0, c1 = window
    inside = np.zeros(gt.shape, dtype=bool)
    inside[r0:r1, c0:c1] = True
    valid = inside & (gt > gt.dtype.type(lo)) & (gt < gt.dtype.type(hi))
    g, p = gt[valid], pred[valid]
    n = int(valid.sum())
    if n == 0:
        return dict(row=np.full(7, np.nan), n=0, med_gt=np.nan, med_pred=np.float32(np.nan), counts=np.zeros(3, dtype=np.int64))
    med_gt, med_pred = _median(g, np.float64), _median(p, pred.dtype.type)
    assert med_pred.dtype == pred.dtype
    g = g.astype(np.float64)
    q = np.clip(p.astype(np.float64) * (med_gt / np.float64(med_pred)), lo, hi)
    ratio = np.maximum(g / q, q / g)
    counts = np.array([int((ratio < t).sum()) for t in THRESHOLDS], dtype=np.int64)
    diff = g - q
    row = np.array([np.sum(np.abs(diff) / g) / n, np.sum(diff ** 2 / g) / n, np.sqrt(np.sum(diff ** 2) / n),
                    np.sqrt(np.sum((np.log(g) - np.log(q)) ** 2) / n), counts[0] / n, counts[1] / n, counts[2] / n])
    return dict(row=row, n=n, med_gt=med_gt, med_pred=med_pred, counts=counts)


def borderline_count(g, p, rel=1e-5):
    """Valid pixels whose ratio max(g / p, p / g) lies within relative `rel` of one of the three thresholds: the only pixels on which two
    correct computations of a1..a3 may disagree."""
    g, p = np.asarray(g, dtype=np.float64), np.asarray(p, dtype=np.float64)
    ratio = np.maximum(g / p, p / g)
    return int(sum(np.sum(np.abs(ratio - t) <= rel * t) for t in THRESHOLDS))


# ---- kernel-level score cases: name -> (gt, pred fp32, window) -----------------------------------------------------------------------------
def _sparse(shape, dtype, cells, fill=0.0):
    gt = np.full(shape, fill, dtype=dtype)
    for (r, c), v in cells:
        gt[r, c] = v
    return gt


def _noisy_pred(g, gt, sigma=0.2, scale=0.5):
    return (np.where(gt > 0, gt, 10.0) * np.exp(g.normal(0.0, sigma, gt.shape)) * scale).astype(np.float32)


def score_cases():
    g = np.random.default_rng(11)
    cases = {}
    small = (20, 30)
    full = (0, 20, 0, 30)
    pred_small = g.uniform(0.5, 40.0, small).astype(np.float32)
    cases["n0"] = (np.zeros(small, dtype=np.float32), pred_small, full)
    cases["n1"] = (_sparse(small, np.float32, [((3, 4), 7.5)]), pred_small, full)
    cases["n2"] = (_sparse(small, np.float64, [((3, 4), 7.5), ((19, 29), 31.25)]), pred_small, full)
    cases["n3"] = (_sparse(small, np.float32, [((0, 0), 2.0), ((10, 7), 60.0), ((19, 29), 5.5)]), pred_small, full)
    cases["even_middle_differs"] = (_sparse(small, np.float32, [((1, 1), 1.0), ((2, 9), 2.0), ((7, 3), 3.5), ((15, 20), 10.0)]), pred_small, full)
    cases["all_equal"] = (np.full((50, 60), 5.0, dtype=np.float32), np.full((50, 60), 2.5, dtype=np.float32), (0, 50, 0, 60))
    bits = (np.float32(8.0).view(np.uint32) + g.permutation(600).astype(np.uint32) % 256).astype(np.uint32)
    pbits = (np.float32(3.0).view(np.uint32) + g.permutation(600).astype(np.uint32) % 251).astype(np.uint32)
    cases["low_8_key_bits"] = (bits.view(np.float32).reshape(20, 30), pbits.view(np.float32).reshape(20, 30), full)
    below = 10.0 + g.permutation(600).astype(np.float64) * 2.0 ** -45          # fp32 spacing at 10 is 2^-20
    assert len(np.unique(below)) == 600 and len(np.unique(below.astype(np.float32))) == 1
    cases["f64_below_f32"] = (below.reshape(20, 30), pred_small, full)
    cases["duplicate_straddles"] = (_sparse(small, np.float32, [((0, 1), 1.0), ((0, 2), 2.0), ((5, 5), 3.0), ((9, 9), 3.0), ((11, 1), 4.0), ((12, 2), 5.0)]),
                                    _sparse(small, np.float32, [((0, 1), 2.0), ((0, 2), 7.0), ((5, 5), 7.0), ((9, 9), 1.0), ((11, 1), 7.0), ((12, 2), 9.0)], fill=4.0),
                                    full)
    for name, dt in (("big_f32", np.float32), ("big_f64", np.float64)):
        gt = g.uniform(0.0, 100.0, (320, 420))
        gt[g.uniform(size=gt.shape) < 0.4] = 0.0
        gt = gt.astype(dt)
        cases[name] = (gt, _noisy_pred(g, gt), (11, 311, 9, 409))              # 300 x 400: 59 workgroups
    gt = g.uniform(0.0, 100.0, (40, 50)).astype(np.float32)
    gt[g.uniform(size=gt.shape) < 0.3] = 0.0
    pred = _noisy_pred(g, gt)
    for name, win in (("top", (0, 10, 5, 45)), ("bottom", (30, 40, 5, 45)), ("left", (3, 37, 0, 7)), ("right", (3, 37, 43, 50)),
                      ("one_row", (17, 18, 3, 47)), ("one_column", (2, 38, 21, 22)), ("whole", (0, 40, 0, 50))):
        cases["window_" + name] = (gt, pred, win)
    for name, dt in (("bounds_f32", np.float32), ("bounds_f64", np.float64)):
        gt = g.uniform(1.0, 79.0, small).astype(dt)
        gt[0, :10], gt[1, :10] = dt(MIN_DEPTH), dt(MAX_DEPTH)                   # strict bounds: neither is valid
        gt[2, :5], gt[3, :5] = np.nextafter(dt(MIN_DEPTH), dt(1)), np.nextafter(dt(MAX_DEPTH), dt(0))       # the neighbours inside are
        cases[name] = (gt, pred_small, full)
    return cases


# ---- evaluator-level cases -------------------------------------------------------------------------------------------------------------------
def _inverse_affine(depth):
    """depth -> the sigmoid disparity `disp_to_depth` maps back to it."""
    return ((1.0 / depth - 0.01) / (10.0 - 0.01)).astype(np.float32)


def _low_res(depth, h, w):
    ys = ((np.arange(h) + 0.5) * depth.shape[0] / h).astype(int)
    xs = ((np.arange(w) + 0.5) * depth.shape[1] / w).astype(int)
    return np.ascontiguousarray(depth[ys][:, xs])


KITTI_SEEDS = (21, 22, 23)
CITYSCAPES_SEED = 31


def kitti_case(root):
    """The fixture calibration (40 x 120) with a dense scan, three noisy 12 x 40 predictions -> (inputs, outputs with CPU tensors)."""
    import torch
    from oracle.data_eval_inputs import kitti_calibration, velodyne_scan
    from uenc.evaluation import KITTIDepthEvaluator
    calib = kitti_calibration(str(root))
    velo = os.path.join(str(root), "scan.bin")
    velodyne_scan(n=200000, seed=5).tofile(velo)
    gt = KITTIDepthEvaluator.generate_depth_map(calib, velo, 2, True)
    filled = np.where(gt > 0, gt, 10.0)
    inputs, outputs = [], []
    for seed in KITTI_SEEDS:
        g = np.random.default_rng(seed)
        depth = _low_res(filled, 12, 40) * np.exp(g.normal(0.0, 0.2, (12, 40))) * 0.5
        inputs.append({"calib_path": calib, "velo_file": velo, "file_name": "a/b/c/d.jpg"})
        outputs.append({"disp_results": torch.from_numpy(_inverse_affine(depth))[None, None]})
    return inputs, outputs


def cityscapes_case(root, dtype):
    """A 352 x 1900 .npy ground truth (264 rows after the cut, 8 x 1664 pixels scored) and a 44 x 238 disparity with batch 2."""
    import torch
    g = np.random.default_rng(CITYSCAPES_SEED)
    gt = g.uniform(0.0, 100.0, (352, 1900))
    gt[g.uniform(size=gt.shape) < 0.2] = 0.0
    gt = gt.astype(dtype)
    d = os.path.join(str(root), "cityscapes")
    os.makedirs(os.path.join(d, "gt_depths", "berlin"), exist_ok=True)
    np.save(os.path.join(d, "gt_depths", "berlin", "berlin_000000_000019.npy"), gt)
    filled = np.where(gt[:264] > 0, gt[:264], 10.0).astype(np.float64)
    depth = np.stack([_low_res(filled, 44, 238) * np.exp(g.normal(0.0, 0.2, (44, 238))) * 0.5 for _ in range(2)])
    inputs = [{"file_name": os.path.join(d, "leftImg8bit/test/berlin/berlin_000000_000019.png").replace(os.sep, "/")}]
    outputs = [{"disp_results": torch.from_numpy(_inverse_affine(depth))[:, None]}]
    return inputs, outputs


def host_rows(ev):
    """Per image of a host-mode evaluator's pairs: (row of seven metrics, valid ground truth, scaled and clamped valid prediction): the
    arrays `compute_errors` received, taken where the evaluator hands them over."""
    out = []
    for pair in ev._pairs:
        got = {}

        def grab(g, p, got=got):
            got["g"] = g
            got["p"] = np.clip(p * (np.median(g) / np.median(p)), ev.MIN_DEPTH, ev.MAX_DEPTH)
            return type(ev)._scaled_errors(ev, g, p)
        ev._scaled_errors = grab
        try:
            row = np.asarray(ev._score(*pair), dtype=np.float64)
        finally:
            del ev._scaled_errors
        out.append((row, got["g"], got["p"]))
    return out


def kitti_window(h, w):
    return tuple(int(v) for v in np.array([0.40810811 * h, 0.99189189 * h, 0.03594771 * w, 0.96405229 * w]).astype(np.int32))
