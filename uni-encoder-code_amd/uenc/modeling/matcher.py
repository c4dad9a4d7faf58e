"""Bipartite matching of predicted segments to ground-truth segments (reference model/modeling/matcher.py).

`HungarianMatcher` has the reference's constructor, `forward(outputs, targets)` and result: per image a pair of int64 index tensors
(queries ascending, matched target of each), `min(Q, T)` long.  On the GPU the work is two entry points of csrc/matcher.hip over a batch of
problems (problem = one prediction head of one image):

    uenc_match_cost   the cost matrix of `memory_efficient_forward` (matcher.py:126-171): prediction and target sampled at the same random
                      points, mask + dice + class terms, NaN -> 100
    uenc_lsap_solve   scipy's linear_sum_assignment on the device (`solver="device"`)

`match_all` runs the final head and every `aux_outputs` entry in ONE cost launch pair and one solver launch.  With `solver="device"` nothing
is read back and the host decides nothing from a value, so the call can be recorded in a stream capture; the indices are device tensors.
`solver="host"` copies all cost matrices once and runs scipy per problem, returning CPU tensors as the reference does.

One deviation, device solver only: the reference returns an EMPTY assignment when every entry of a cost matrix is NaN (matcher.py:31-32);
the device cannot make a result's shape depend on values, so there an all-NaN matrix is treated like any NaN (entries 100).

CPU inputs run the same formulas in plain torch + scipy.  Target masks are 0 / 1 (bool, uint8 or float), already padded to one size per
call.  The loss that uses the indices is uenc.modeling.criterion.SetCriterion (the reference ships none).
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

__all__ = ["HungarianMatcher", "batch_dice_loss", "batch_sigmoid_ce_loss", "linear_sum_assignment_with_nan", "point_sample", "NAN_COST"]

NAN_COST = 100.0                # what a NaN cost entry becomes (matcher.py:33-34)


def linear_sum_assignment_with_nan(cost_matrix):
    """scipy's linear_sum_assignment with the reference's NaN policy (matcher.py:19-36): an all-NaN matrix gives the empty assignment,
    single NaN entries become 100."""
    from scipy.optimize import linear_sum_assignment
    c = np.array(cost_matrix, dtype=np.float64, copy=True)
    if c.size:
        bad = np.isnan(c)
        if bad.all():
            c = np.empty((0, 0))
        elif bad.any():
            c[bad] = NAN_COST
    return linear_sum_assignment(c)


def point_sample(inp: torch.Tensor, point_coords: torch.Tensor, **kwargs) -> torch.Tensor:
    """(N, C, H, W) sampled at (N, P, 2) points in [0, 1] x [0, 1] -> (N, C, P): grid_sample at 2 p - 1 (Detectron2's point_sample for 3-D
    coordinates)."""
    return F.grid_sample(inp, 2.0 * point_coords.unsqueeze(2) - 1.0, **kwargs).squeeze(3)


def batch_dice_loss(inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Pairwise dice loss: inputs (N, P) logits, targets (M, P) in [0, 1] -> (N, M), 1 - (2 s.t + 1) / (sum s + sum t + 1), s = sigmoid."""
    s = inputs.sigmoid().flatten(1)
    inter = 2 * torch.einsum("nc,mc->nm", s, targets)
    total = s.sum(-1)[:, None] + targets.sum(-1)[None, :]
    return 1 - (inter + 1) / (total + 1)


def batch_sigmoid_ce_loss(inputs: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
    """Pairwise binary cross entropy with logits, averaged over the points: inputs (N, P), targets (M, P) -> (N, M)."""
    on = F.binary_cross_entropy_with_logits(inputs, torch.ones_like(inputs), reduction="none")      # softplus(-x)
    off = F.binary_cross_entropy_with_logits(inputs, torch.zeros_like(inputs), reduction="none")    # softplus(x)
    return (torch.einsum("nc,mc->nm", on, targets) + torch.einsum("nc,mc->nm", off, 1 - targets)) / inputs.shape[1]


def _f32c(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.float().contiguous()


def _mask_bytes(m: torch.Tensor) -> torch.Tensor:
    m = m.contiguous()
    if m.dtype == torch.bool:
        return m.view(torch.uint8)
    return m if m.dtype == torch.uint8 else m.to(torch.uint8)


class HungarianMatcher(nn.Module):
    """1-to-1 assignment of the best predictions to the targets; the other predictions stay unmatched (no-object).

    cost_class / cost_mask / cost_dice weigh the three terms of the matching cost, num_points is the number of random points at which
    masks are compared (MODEL.ONE_FORMER.TRAIN_NUM_POINTS).  `solver`: "device" | "host" | None (= "device" for GPU inputs)."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1, num_points: int = 0, solver: Optional[str] = None):
        super().__init__()
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"
        if solver not in (None, "device", "host"):
            raise ValueError(f'HungarianMatcher: solver must be "device", "host" or None, got {solver!r}')
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        self.num_points = num_points
        self.solver = solver

    # ---- points -----------------------------------------------------------------------------------------------------------------
    def _points(self, n_heads: int, bs: int, device, point_coords) -> List[List[torch.Tensor]]:
        """[head][image] -> (P, 2) fp32.  Drawn as the reference does when not given: one torch.rand(1, P, 2) per image and matcher
        call, the final head first, then the auxiliary heads in order (matcher.py:143)."""
        if point_coords is None:
            return [[torch.rand(1, self.num_points, 2, device=device)[0] for _ in range(bs)] for _ in range(n_heads)]
        pc = point_coords
        if torch.is_tensor(pc):
            if pc.dim() == 3:                             # (bs, P, 2): the same points for every head
                pc = [pc] * n_heads
            elif pc.dim() != 4:
                raise ValueError("point_coords: (bs, P, 2), (heads, bs, P, 2) or nested lists of (P, 2)")
        if len(pc) != n_heads or any(len(h) != bs for h in pc):
            raise ValueError(f"point_coords: expected {n_heads} heads x {bs} images")
        out = [[_f32c(torch.as_tensor(p).to(device)).reshape(-1, 2) for p in h] for h in pc]
        P = out[0][0].shape[0]
        if P < 1 or any(p.shape[0] != P for h in out for p in h):
            raise ValueError("point_coords: every problem of one call needs the same number (>= 1) of points")
        return out

    # ---- the cost matrix in torch (CPU inputs) --------------------------------------------------------------------------------------
    def _cost_torch(self, logits, masks, gt, labels, points) -> torch.Tensor:
        """(Q, T) cost of one problem with torch ops: the composition of matcher.py:128-170."""
        prob = logits.float().softmax(-1)
        cost_class = -prob[:, labels]
        x, t = masks.float()[:, None], gt.to(torch.float32)[:, None]
        pc = points[None]
        t = point_sample(t, pc.repeat(t.shape[0], 1, 1), align_corners=False).squeeze(1)
        x = point_sample(x, pc.repeat(x.shape[0], 1, 1), align_corners=False).squeeze(1)
        C = self.cost_mask * batch_sigmoid_ce_loss(x, t) + self.cost_class * cost_class + self.cost_dice * batch_dice_loss(x, t)
        return C.reshape(logits.shape[0], -1)

    # ---- matching -----------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def match_all(self, outputs, targets, point_coords=None, solver: Optional[str] = None):
        """The final head and every entry of outputs["aux_outputs"] against `targets`: [indices_final, indices_aux0, ...], each a list
        of (index_i, index_j) per image.  `point_coords` (keyword) fixes the sampling points: (bs, P, 2) shared by all heads,
        (heads, bs, P, 2), or nested lists."""
        heads = [outputs] + list(outputs.get("aux_outputs", []))
        lg0 = outputs["pred_logits"]
        bs, Q = lg0.shape[:2]
        if len(targets) != bs:
            raise ValueError(f"{len(targets)} targets for a batch of {bs}")
        solver = solver or self.solver
        if solver not in (None, "device", "host"):
            raise ValueError(f'solver must be "device", "host" or None, got {solver!r}')
        points = self._points(len(heads), bs, lg0.device, point_coords)
        if not lg0.is_cuda:
            if solver == "device":
                raise ValueError('solver="device" needs GPU inputs')
            return [[self._match_cpu(h["pred_logits"][b], h["pred_masks"][b], targets[b], points[i][b]) for b in range(bs)]
                    for i, h in enumerate(heads)]

        from .. import kernels as K
        gts = [_mask_bytes(t["masks"]) for t in targets]
        labs = [t["labels"].to(torch.int64).contiguous() for t in targets]
        Ts = [int(g.shape[0]) for g in gts]
        problems = []
        for i, h in enumerate(heads):
            lg, mk = _f32c(h["pred_logits"]), _f32c(h["pred_masks"])
            for b in range(bs):
                problems.append((lg[b], mk[b], points[i][b], gts[b], labs[b]))
        pTs = Ts * len(heads)
        if (solver or "device") == "device":
            cost = K.match_cost(problems, float(self.cost_class), float(self.cost_mask), float(self.cost_dice), NAN_COST)
            rows, cols, offs = K.lsap_solve(cost, pTs)
            flat = [(rows[offs[p]:offs[p + 1]], cols[offs[p]:offs[p + 1]]) for p in range(len(problems))]
        else:
            cost = K.match_cost(problems, float(self.cost_class), float(self.cost_mask), float(self.cost_dice), float("nan"))
            host = cost.cpu().numpy()                     # the one copy (and synchronisation) of host mode
            flat = []
            for p, T in enumerate(pTs):
                i, j = linear_sum_assignment_with_nan(host[p, :, :T])
                flat.append((torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)))
        return [flat[i * bs:(i + 1) * bs] for i in range(len(heads))]

    def _match_cpu(self, logits, masks, tgt, points) -> Tuple[torch.Tensor, torch.Tensor]:
        C = self._cost_torch(logits, masks, tgt["masks"], tgt["labels"], points)
        i, j = linear_sum_assignment_with_nan(C.numpy())
        return torch.as_tensor(i, dtype=torch.int64), torch.as_tensor(j, dtype=torch.int64)

    @torch.no_grad()
    def cost_matrices(self, outputs, targets, point_coords=None) -> List[torch.Tensor]:
        """The (Q, T) cost matrix of every image for ONE head (no aux_outputs), NaN entries already 100: what the solver is given.  For
        tests and diagnostics; GPU inputs run uenc_match_cost."""
        lg, mk = outputs["pred_logits"], outputs["pred_masks"]
        bs = lg.shape[0]
        points = self._points(1, bs, lg.device, point_coords)[0]
        if not lg.is_cuda:
            return [torch.nan_to_num(self._cost_torch(lg[b], mk[b], targets[b]["masks"], targets[b]["labels"], points[b]), nan=NAN_COST)
                    for b in range(bs)]
        from .. import kernels as K
        lg, mk = _f32c(lg), _f32c(mk)
        problems = [(lg[b], mk[b], points[b], _mask_bytes(targets[b]["masks"]), targets[b]["labels"].to(torch.int64).contiguous())
                    for b in range(bs)]
        cost = K.match_cost(problems, float(self.cost_class), float(self.cost_mask), float(self.cost_dice), NAN_COST)
        return [cost[b, :, :problems[b][3].shape[0]] for b in range(bs)]

    @torch.no_grad()
    def forward(self, outputs, targets, point_coords=None, solver: Optional[str] = None):
        """outputs: {"pred_logits": (bs, Q, C + 1), "pred_masks": (bs, Q, h, w)}; targets: per image {"labels": (T,), "masks": (T, H, W)}.
        Returns per image (index_i, index_j): the selected predictions in order and the target matched to each."""
        single = {"pred_logits": outputs["pred_logits"], "pred_masks": outputs["pred_masks"]}
        return self.match_all(single, targets, point_coords=point_coords, solver=solver)[0]

    memory_efficient_forward = forward

    def __repr__(self, _repr_indent=4):
        pad = " " * _repr_indent
        return "\n".join(["Matcher " + self.__class__.__name__, f"{pad}cost_class: {self.cost_class}", f"{pad}cost_mask: {self.cost_mask}",
                          f"{pad}cost_dice: {self.cost_dice}"])
