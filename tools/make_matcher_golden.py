"""tests/golden/matcher.npz: what the REFERENCE's HungarianMatcher (model/modeling/matcher.py) computes on a dozen small problems.

Build container only (needs the reference checkout, oracle.ref_loader.REF_ROOT).  The reference's file is loaded by path and run as it
is; nothing of its text is restated.  Its one import that is not installed, detectron2's `point_sample`, gets a stand-in written here
(grid_sample at 2 * coords - 1, its documented semantics).  While its matcher runs,
  * `torch.rand` is wrapped so that the sampling points it draws are recorded (the values are torch's own, so a seeded product run can be
    checked to draw the same ones),
  * its `linear_sum_assignment_with_nan` is wrapped so that the cost matrix it hands to scipy is recorded.

Per problem p (one image of one call) the file holds
  p{p}_logits (Q, C+1) f32   p{p}_masks8 (Q, h, w) int8 = mask logits * 8 (the logits are multiples of 1/8)   p{p}_nan_at (3,) or empty: a
  planted NaN   p{p}_gt (T, 4h, 4w) uint8   p{p}_labels (T,) i64   p{p}_points (P, 2) f32   p{p}_cost (Q, T) f32 as handed to scipy (NaN still
  in it)   p{p}_row / p{p}_col: the reference's assignment
and for all of them: weights (n, 3) = cost_class, cost_mask, cost_dice; num_points (n,); call (n,) and image (n,): which matcher call and
image of it; seed (n,): the torch seed set before that call; stable (n,): the assignment is unchanged under 20 random perturbations of the
cost matrix of amplitude 2e-3 (uniform, per entry).

    python tools/make_matcher_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_loader import REF_ROOT  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "matcher.npz")
STABLE_AMPLITUDE, STABLE_TRIALS = 2e-3, 20


def _point_sample(input, point_coords, **kwargs):
    """Detectron2 point_sample for (N, P, 2) coordinates in [0, 1]^2."""
    return F.grid_sample(input, 2.0 * point_coords.unsqueeze(2) - 1.0, **kwargs).squeeze(3)


def load_reference_matcher():
    names = ["detectron2", "detectron2.projects", "detectron2.projects.point_rend", "detectron2.projects.point_rend.point_features"]
    saved = {n: sys.modules.get(n) for n in names}
    for n in names:
        sys.modules[n] = types.ModuleType(n)
    sys.modules[names[-1]].point_sample = _point_sample
    try:
        spec = importlib.util.spec_from_file_location("_reference_matcher", os.path.join(REF_ROOT, "model", "modeling", "matcher.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for n, m in saved.items():
            if m is None:
                del sys.modules[n]
            else:
                sys.modules[n] = m
    return mod


def discs(g, T, H, W):
    """T random discs as (T, H, W) uint8."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    cy, cx = torch.rand(T, generator=g) * H, torch.rand(T, generator=g) * W
    r = (0.08 + 0.22 * torch.rand(T, generator=g)) * min(H, W)
    return (((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2) <= r[:, None, None] ** 2).to(torch.uint8)


def make_problem(g, Q, T, C1, h, w):
    """Half of the targets get a query whose mask logits resemble them (pooled target * 8 - 4 + noise) and whose class logit favours
    their label; every other query is noise * 3.  Mask logits are rounded to multiples of 1/8 (stored as int8)."""
    gt = discs(g, T, 4 * h, 4 * w)
    labels = torch.randint(0, C1 - 1, (T,), generator=g)
    logits = torch.randn(Q, C1, generator=g)
    masks = torch.randn(Q, h, w, generator=g) * 3
    owners = torch.randperm(Q, generator=g)[:min(Q, (T + 1) // 2)]
    for t, q in enumerate(owners.tolist()):
        pooled = F.avg_pool2d(gt[t][None, None].float(), 4)[0, 0]
        masks[q] = pooled * 8 - 4 + torch.randn(h, w, generator=g)
        logits[q, labels[t]] += 3
    masks8 = (masks * 8).round().clamp(-127, 127).to(torch.int8)
    return logits, masks8, gt, labels


CALLS = [  # (weights class / mask / dice, num_points, Q, C+1, h, w, T per image, NaN planted in image 0)
    ((2.0, 5.0, 5.0), 400, 150, 20, 12, 20, (17, 40), False),
    ((2.0, 5.0, 5.0), 400, 100, 20, 12, 20, (5,), False),
    ((2.0, 5.0, 5.0), 400, 20, 20, 12, 20, (31,), False),
    ((2.0, 5.0, 5.0), 400, 150, 20, 12, 20, (1, 0), False),
    ((2.0, 5.0, 5.0), 400, 150, 20, 12, 20, (12,), True),
    ((2.0, 5.0, 5.0), 12544, 150, 20, 24, 40, (17,), False),
    ((4.0, 1.0, 0.5), 300, 150, 134, 12, 20, (25, 9), False),
    ((2.0, 5.0, 5.0), 333, 50, 20, 11, 19, (60, 8), False),
]


def main():
    ref = load_reference_matcher()
    g = torch.Generator().manual_seed(20240607)
    out, meta = {}, {k: [] for k in ("weights", "num_points", "call", "image", "seed", "stable")}
    p = 0
    for ci, (wts, P, Q, C1, h, w, Ts, plant) in enumerate(CALLS):
        probs = [make_problem(g, Q, T, C1, h, w) for T in Ts]
        masks = [m8.float() / 8 for _, m8, _, _ in probs]
        nan_at = None
        if plant:
            owner_free = 3
            nan_at = (owner_free, h // 2, w // 3)
            masks[0][nan_at] = float("nan")
        outputs = {"pred_logits": torch.stack([pr[0] for pr in probs]), "pred_masks": torch.stack(masks)}
        targets = [{"labels": pr[3], "masks": pr[2]} for pr in probs]
        matcher = ref.HungarianMatcher(cost_class=wts[0], cost_mask=wts[1], cost_dice=wts[2], num_points=P)

        points, costs = [], []
        real_rand, real_lsa = torch.rand, ref.linear_sum_assignment_with_nan

        def rand(*a, **k):
            r = real_rand(*a, **k)
            points.append(r.clone())
            return r

        def lsa(c):
            costs.append((c.detach().numpy() if torch.is_tensor(c) else np.asarray(c)).astype(np.float32, copy=True))
            return real_lsa(c)

        seed = 1000 + ci
        torch.manual_seed(seed)
        torch.rand, ref.linear_sum_assignment_with_nan = rand, lsa
        try:
            indices = matcher(outputs, targets)
        finally:
            torch.rand, ref.linear_sum_assignment_with_nan = real_rand, real_lsa
        assert len(points) == len(costs) == len(Ts)

        for b, T in enumerate(Ts):
            logits, m8, gt, labels = probs[b]
            row, col = indices[b][0].numpy(), indices[b][1].numpy()
            C = costs[b].reshape(Q, T)
            assert len(row) == min(Q, T)
            stable = T > 0
            if T > 0:
                from scipy.optimize import linear_sum_assignment
                clean = np.where(np.isnan(C), 100.0, C).astype(np.float64)
                rs = np.random.RandomState(7 + p)
                for _ in range(STABLE_TRIALS):
                    i2, j2 = linear_sum_assignment(clean + rs.uniform(-STABLE_AMPLITUDE, STABLE_AMPLITUDE, clean.shape))
                    stable &= bool(np.array_equal(i2, row) and np.array_equal(j2, col))
            out[f"p{p}_logits"] = logits.numpy()
            out[f"p{p}_masks8"] = m8.numpy()
            out[f"p{p}_nan_at"] = np.array(nan_at if (plant and b == 0) else [], dtype=np.int64)
            out[f"p{p}_gt"] = gt.numpy()
            out[f"p{p}_labels"] = labels.numpy().astype(np.int64)
            out[f"p{p}_points"] = points[b][0].numpy()
            out[f"p{p}_cost"] = C
            out[f"p{p}_row"], out[f"p{p}_col"] = row.astype(np.int64), col.astype(np.int64)
            for k, v in (("weights", wts), ("num_points", P), ("call", ci), ("image", b), ("seed", seed), ("stable", stable)):
                meta[k].append(v)
            print(f"problem {p}: call {ci} image {b}  Q {Q} T {T} P {P}  cost [{np.nanmin(C) if T else 0:.3f}, {np.nanmax(C) if T else 0:.3f}]"
                  f"  NaN {int(np.isnan(C).sum())}  stable {stable}")
            p += 1

    out["weights"] = np.array(meta["weights"], dtype=np.float64)
    for k in ("num_points", "call", "image", "seed"):
        out[k] = np.array(meta[k], dtype=np.int64)
    out["stable"] = np.array(meta["stable"], dtype=np.bool_)
    nonempty = [i for i in range(p) if out[f"p{i}_gt"].shape[0] > 0]
    n_stable = int(sum(out["stable"][i] for i in nonempty))
    print(f"{n_stable} of {len(nonempty)} non-empty problems stable at {STABLE_AMPLITUDE}")
    assert 2 * n_stable >= len(nonempty), "at least half of the non-empty problems must be stable"
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
