"""tests/golden/matcher.npz (tools/make_matcher_golden.py) as tensors, and the checks both matcher test files share."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "matcher.npz")
STABLE_AMPLITUDE = 2e-3          # the generator's perturbation amplitude


def load_problems():
    """One dict per problem: logits, masks (fp32, NaN planted where the fixture says), gt (uint8), labels, points, cost (the reference's
    matrix with NaN -> 100, float64), row / col (its assignment), weights, num_points, call, image, seed, stable."""
    z = np.load(GOLDEN, allow_pickle=False)
    out = []
    for p in range(len(z["stable"])):
        masks = torch.from_numpy(z[f"p{p}_masks8"]).float() / 8
        at = z[f"p{p}_nan_at"]
        if at.size:
            masks[tuple(int(a) for a in at)] = float("nan")
        cost = z[f"p{p}_cost"].astype(np.float64)
        out.append({"logits": torch.from_numpy(z[f"p{p}_logits"]), "masks": masks, "gt": torch.from_numpy(z[f"p{p}_gt"]),
                    "labels": torch.from_numpy(z[f"p{p}_labels"]), "points": torch.from_numpy(z[f"p{p}_points"]),
                    "cost_raw": cost, "cost": np.where(np.isnan(cost), 100.0, cost), "row": z[f"p{p}_row"], "col": z[f"p{p}_col"],
                    "weights": tuple(float(w) for w in z["weights"][p]), "num_points": int(z["num_points"][p]), "call": int(z["call"][p]),
                    "image": int(z["image"][p]), "seed": int(z["seed"][p]), "stable": bool(z["stable"][p]), "index": p})
    return out


def calls(problems):
    """The problems grouped by the matcher call they came from: [(outputs, targets, points (bs, P, 2), [problem, ...]), ...]."""
    groups = {}
    for pr in problems:
        groups.setdefault(pr["call"], []).append(pr)
    out = []
    for c in sorted(groups):
        ps = sorted(groups[c], key=lambda pr: pr["image"])
        outputs = {"pred_logits": torch.stack([pr["logits"] for pr in ps]), "pred_masks": torch.stack([pr["masks"] for pr in ps])}
        targets = [{"labels": pr["labels"], "masks": pr["gt"]} for pr in ps]
        out.append((outputs, targets, torch.stack([pr["points"] for pr in ps]), ps))
    return out


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def check_assignment(row, col, pr, e):
    """A valid assignment (distinct rows and columns, rows ascending, min(Q, T) long) whose total on the REFERENCE's matrix is at most the
    reference's total + 2 n e: an error of at most e per entry moves any assignment's total by at most n e, hence the optimum by at most
    twice that.  Returns the excess over the reference's total."""
    row, col = np.asarray(row), np.asarray(col)
    Q, T = pr["cost"].shape
    n = min(Q, T)
    assert row.shape == col.shape == (n,), (row.shape, col.shape, n)
    if n == 0:
        return 0.0
    assert row.dtype == np.int64 and col.dtype == np.int64
    assert (np.diff(row) > 0).all() and row.min() >= 0 and row.max() < Q
    assert len(set(col.tolist())) == n and col.min() >= 0 and col.max() < T
    total, ref_total = pr["cost"][row, col].sum(), pr["cost"][pr["row"], pr["col"]].sum()
    assert total <= ref_total + 2 * n * e + 1e-12, (pr["index"], total, ref_total, n, e)
    return float(total - ref_total)
