"""The set criterion: class loss plus point-sampled mask and dice losses of the matched (prediction, target) pairs, for the final head
and every `aux_outputs` entry.

The reference ships no criterion.py; this is the Mask2Former / OneFormer criterion its matcher header cites, configured by the keys the
reference does define (model/config.py:147-189: DEEP_SUPERVISION, NO_OBJECT_WEIGHT, CLASS_WEIGHT, DICE_WEIGHT, MASK_WEIGHT,
TRAIN_NUM_POINTS, OVERSAMPLE_RATIO, IMPORTANCE_SAMPLE_RATIO).  The two mask losses are the diagonal of the matcher's pairwise
`batch_sigmoid_ce_loss` / `batch_dice_loss` (matcher.py:38-85), sampled with `point_sample(align_corners=False)` as matcher.py:145-155.

Per head, with the pairs running over the images in order and within an image in the matcher's order (N = sum_b min(Q, T_b)):

    loss_ce    F.cross_entropy(logits, target classes, weights (1, ..., 1, eos_coef)); unmatched queries are the no-object class
    points     per pair, under no_grad: M = int(P oversample_ratio) uniform points, the int(importance_sample_ratio P) of them with the
               smallest |logit| kept, P - that many fresh uniform points appended
    loss_mask  sum_n mean_p bce_with_logits(x_p, t_p) / num_masks        x, t = the pair's logit map / target mask at its points
    loss_dice  sum_n (1 - (2 sum s t + 1) / (sum s + sum t + 1)) / num_masks,  s = sigmoid(x)

num_masks = max(sum_b T_b, 1) (averaged over the ranks when torch.distributed runs).  The losses come back UNWEIGHTED (`loss_ce`,
`loss_mask`, `loss_dice`, and `loss_*_{i}` for aux_outputs[i]); `weight_dict` holds the weights and `weighted_sum` applies them.

GPU inputs run csrc/criterion.hip, all heads per launch (uenc_crit_point_logits, uenc_crit_mask_loss_fwd / _bwd, uenc_crit_class_loss);
the kernels read the matcher's device index buffers, nothing is read back and the host decides nothing from a value, so matcher +
criterion + backward can be recorded in a stream capture.  CPU inputs run the same formulas as torch ops with autograd
(`_forward_torch`, which also runs on GPU tensors: the benchmark's baseline).  The contrastive loss needs the text encoder, which the
model does not have (`contrastive_logits` is None): asking for it raises.
"""
from typing import Dict, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from .matcher import HungarianMatcher, _f32c, _mask_bytes, point_sample

__all__ = ["SetCriterion", "build_criterion", "pad_targets"]


def pad_targets(targets, size):
    """Per-image target masks of differing (H_i, W_i) zero-padded at the bottom and right to size = (H, W): the matcher and the
    criterion take one padded size per call.  Labels (and any other key) are passed through."""
    H, W = int(size[0]), int(size[1])
    out = []
    for t in targets:
        m = t["masks"]
        if m.dim() != 3 or m.shape[1] > H or m.shape[2] > W:
            raise ValueError(f"pad_targets: masks {tuple(m.shape)} do not fit into {(H, W)}")
        padded = m.new_zeros((m.shape[0], H, W))
        padded[:, :m.shape[1], :m.shape[2]] = m
        out.append(dict(t, masks=padded))
    return out


def _flat(parts: Sequence[torch.Tensor], device) -> torch.Tensor:
    """Index tensors in pair order as ONE int64 device buffer: the matcher's own buffer when they are its consecutive slices (the device
    solver's result), otherwise a concatenation (and, for the host solver's CPU tensors, one upload)."""
    first = parts[0]
    if first.is_cuda and first.dtype == torch.int64:
        off, store = first.storage_offset(), first.untyped_storage().data_ptr()
        for p in parts:
            if p.dtype != torch.int64 or p.dim() != 1 or not p.is_contiguous() or p.untyped_storage().data_ptr() != store or p.storage_offset() != off:
                break
            off += p.numel()
        else:
            return first.as_strided((off - first.storage_offset(),), (1,))
    return torch.cat([p.to(torch.int64) for p in parts]).to(device)


class _MaskLossFn(torch.autograd.Function):
    """(loss_mask, loss_dice) of every head, (heads) each, from uenc_crit_mask_loss_fwd; the backward sorts the tap keys and runs
    uenc_crit_mask_loss_bwd."""

    @staticmethod
    def forward(ctx, call, row, col, points, inv_num_masks, *masks):
        from .. import kernels as K
        need = any(ctx.needs_input_grad[5:])
        loss, _, unit, keys = K.crit_mask_loss_fwd(call, row, col, points, need_grad=need)
        ctx.call, ctx.inv_num_masks = call, inv_num_masks
        if need:
            ctx.save_for_backward(row, points, unit, keys)
        per_head = loss.view(call.n_heads, call.N, 2).sum(1) * inv_num_masks
        return per_head[:, 0].contiguous(), per_head[:, 1].contiguous()

    @staticmethod
    def backward(ctx, gce, gdice):
        from .. import kernels as K
        row, points, unit, keys = ctx.saved_tensors
        skeys, order = torch.sort(keys, dim=1, stable=True)
        gm = K.crit_mask_loss_bwd(ctx.call, row, points, unit, skeys, order, _f32c(gce), _f32c(gdice), ctx.inv_num_masks)
        return (None,) * 5 + tuple(gm[i] if ctx.needs_input_grad[5 + i] else None for i in range(ctx.call.n_heads))


class _ClassLossFn(torch.autograd.Function):
    """loss_ce of every head, (heads), from uenc_crit_class_loss, which also leaves the gradient."""

    @staticmethod
    def forward(ctx, call, row, col, eos_coef, *logits):
        from .. import kernels as K
        loss, grad = K.crit_class_loss(call, row, col, eos_coef)
        ctx.call = call
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        grad, = ctx.saved_tensors
        c = ctx.call
        gl = (grad * g[:, None, None]).view(c.n_heads, c.bs, c.Q, c.C1)
        return (None,) * 4 + tuple(gl[i] if ctx.needs_input_grad[4 + i] else None for i in range(c.n_heads))


class SetCriterion(nn.Module):
    """num_classes: C (the no-object class is index C); matcher: a HungarianMatcher; weight_dict: loss name -> weight; eos_coef: the
    no-object class weight; losses: a subset of ("labels", "masks"); num_points / oversample_ratio / importance_sample_ratio: the
    point sampling (MODEL.ONE_FORMER.TRAIN_NUM_POINTS / OVERSAMPLE_RATIO / IMPORTANCE_SAMPLE_RATIO)."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio, importance_sample_ratio):
        super().__init__()
        losses = list(losses)
        if "contrastive" in losses:
            raise NotImplementedError("SetCriterion: the contrastive loss needs the text encoder, which this model does not have "
                                      "(contrastive_logits is None)")
        unknown = [name for name in losses if name not in ("labels", "masks")]
        if unknown:
            raise ValueError(f'SetCriterion: losses must come from ("labels", "masks"), got {unknown}')
        if num_points < 1 or oversample_ratio < 1 or not 0 <= importance_sample_ratio <= 1:
            raise ValueError("SetCriterion: num_points >= 1, oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1 are required")
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = dict(weight_dict)
        self.eos_coef = float(eos_coef)
        self.losses = losses
        self.num_points = int(num_points)
        self.oversample_ratio = oversample_ratio
        self.importance_sample_ratio = importance_sample_ratio
        empty_weight = torch.ones(num_classes + 1)
        empty_weight[-1] = self.eos_coef
        self.register_buffer("empty_weight", empty_weight)

    # ---- points -----------------------------------------------------------------------------------------------------------------------
    def point_counts(self):
        """(M oversampled, n_unc kept by uncertainty, n_rnd appended): the int() truncations of the upstream sampler."""
        M = int(self.num_points * self.oversample_ratio)
        n_unc = int(self.importance_sample_ratio * self.num_points)
        return M, n_unc, self.num_points - n_unc

    def _draws(self, n_heads: int, N: int, device, point_draws):
        """-> oversampled (heads, N, M, 2) or None when nothing is kept by uncertainty, random (heads, N, n_rnd, 2) or None when n_rnd = 0.
        Drawn with torch.rand on `device` when not given: per head the oversampled points first, then the random ones."""
        M, n_unc, n_rnd = self.point_counts()
        if point_draws is None:
            over, rnd = [], []
            for _ in range(n_heads):
                over.append(torch.rand(N, M, 2, device=device) if n_unc else None)
                rnd.append(torch.rand(N, n_rnd, 2, device=device) if n_rnd else None)
            return (torch.stack(over) if n_unc else None), (torch.stack(rnd) if n_rnd else None)
        over = _f32c(torch.as_tensor(point_draws["oversampled"]).to(device)) if n_unc else None
        rnd = _f32c(torch.as_tensor(point_draws["random"]).to(device)) if n_rnd else None
        if (over is not None and tuple(over.shape) != (n_heads, N, M, 2)) or (rnd is not None and tuple(rnd.shape) != (n_heads, N, n_rnd, 2)):
            raise ValueError(f"point_draws: oversampled {(n_heads, N, M, 2)} and random {(n_heads, N, n_rnd, 2)} are expected")
        return over, rnd

    def _select(self, over, logits, rnd):
        """The final points: of the oversampled ones (..., M, 2) the n_unc with the smallest |logit| (logits (..., M)), then the random
        ones (..., n_rnd, 2) -> (..., P, 2)."""
        n_unc = self.point_counts()[1]
        parts = []
        if n_unc:
            idx = torch.topk(-logits.abs(), n_unc, dim=-1).indices
            parts.append(torch.gather(over, -2, idx.unsqueeze(-1).expand(*idx.shape, 2)))
        if rnd is not None:
            parts.append(rnd)
        return torch.cat(parts, dim=-2).contiguous()

    def _select_torch(self, src, over, rnd):
        """One head with torch ops: src (N, 1, h, w), over (N, M, 2) or None, rnd (N, n_rnd, 2) or None -> (N, P, 2)."""
        logits = point_sample(src, over, align_corners=False).squeeze(1) if over is not None else None
        return self._select(over, logits, rnd)

    @torch.no_grad()
    def _select_hip(self, call, row, over, rnd):
        """All heads: uenc_crit_point_logits for the oversampled points, top-k and gather as device ops -> (heads * N, P, 2)."""
        from .. import kernels as K
        R = call.n_heads * call.N
        over = over.view(R, -1, 2) if over is not None else None
        logits = K.crit_point_logits(call, row, over) if over is not None else None
        return self._select(over, logits, rnd.view(R, -1, 2) if rnd is not None else None)

    @torch.no_grad()
    def select_points(self, outputs, targets, indices, point_draws=None) -> torch.Tensor:
        """The final sampling points (heads, N, P, 2) `forward` uses for these draws (N >= 1): for tests and diagnostics."""
        heads = [outputs] + list(outputs.get("aux_outputs", []))
        dev = outputs["pred_masks"].device
        Q = outputs["pred_masks"].shape[1]
        N = sum(min(Q, int(t["labels"].shape[0])) for t in targets)
        over, rnd = self._draws(len(heads), N, dev, point_draws)
        if dev.type == "cuda":
            from .. import kernels as K
            call = K.CritCall([_f32c(h["pred_masks"]) for h in heads], [None] * len(heads), [_mask_bytes(t["masks"]) for t in targets],
                              [t["labels"].to(torch.int64).contiguous() for t in targets])
            row = _flat([pair[0] for head in indices for pair in head], dev)
            return self._select_hip(call, row, over, rnd).view(len(heads), N, -1, 2)
        out = []
        for i, hd in enumerate(heads):
            b_idx = torch.cat([torch.full_like(qi, b) for b, (qi, _) in enumerate(indices[i])])
            src = hd["pred_masks"].float()[b_idx, torch.cat([qi for qi, _ in indices[i]])][:, None]
            out.append(self._select_torch(src, over[i] if over is not None else None, rnd[i] if rnd is not None else None))
        return torch.stack(out)

    # ---- the normaliser ---------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _num_masks(Ts, device) -> float:
        n = float(sum(Ts))
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            t = torch.tensor([n], dtype=torch.float32, device=device)
            dist.all_reduce(t)
            n = float(t) / dist.get_world_size()
        return max(n, 1.0)

    # ---- the formulas as torch ops (CPU inputs; on GPU tensors the benchmark's baseline) ------------------------------------------------------
    @staticmethod
    def pair_losses(x: torch.Tensor, t: torch.Tensor):
        """x (N, P) sampled logits, t (N, P) sampled targets -> (ce_n, dice_n), (N) each: the diagonal of the matcher's
        batch_sigmoid_ce_loss / batch_dice_loss."""
        ce = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(1)
        s = x.sigmoid()
        return ce, 1 - (2 * (s * t).sum(-1) + 1) / (s.sum(-1) + t.sum(-1) + 1)

    def _forward_torch(self, heads, targets, indices, over, rnd, num_masks, N):
        dev = heads[0]["pred_logits"].device
        bs, Q = heads[0]["pred_logits"].shape[:2]
        out = []
        for i, hd in enumerate(heads):
            idx = [(a.to(dev), b.to(dev)) for a, b in indices[i]]
            res = {}
            if "labels" in self.losses:
                target_classes = torch.full((bs, Q), self.num_classes, dtype=torch.int64, device=dev)
                for b, (qi, tj) in enumerate(idx):
                    target_classes[b, qi] = targets[b]["labels"].to(dev)[tj]
                res["loss_ce"] = F.cross_entropy(hd["pred_logits"].float().transpose(1, 2), target_classes, self.empty_weight.to(dev))
            if "masks" in self.losses and N == 0:
                res["loss_mask"] = res["loss_dice"] = hd["pred_masks"].float().sum() * 0
            elif "masks" in self.losses:
                b_idx = torch.cat([torch.full_like(qi, b) for b, (qi, _) in enumerate(idx)])
                src = hd["pred_masks"].float()[b_idx, torch.cat([qi for qi, _ in idx])][:, None]
                tgt = torch.cat([targets[b]["masks"].to(dev)[tj] for b, (_, tj) in enumerate(idx)]).to(torch.float32)[:, None]
                with torch.no_grad():
                    points = self._select_torch(src, over[i] if over is not None else None, rnd[i] if rnd is not None else None)
                    t = point_sample(tgt, points, align_corners=False).squeeze(1)
                x = point_sample(src, points, align_corners=False).squeeze(1)
                ce, dice = self.pair_losses(x, t)
                res["loss_mask"], res["loss_dice"] = ce.sum() / num_masks, dice.sum() / num_masks
            out.append(res)
        return out

    # ---- the HIP path ------------------------------------------------------------------------------------------------------------------
    def _forward_hip(self, heads, targets, indices, over, rnd, num_masks, N):
        from .. import kernels as K
        dev = heads[0]["pred_logits"].device
        n_heads = len(heads)
        want_masks, want_labels = "masks" in self.losses and N > 0, "labels" in self.losses
        masks = [_f32c(h["pred_masks"]) if want_masks else None for h in heads]
        logits = [_f32c(h["pred_logits"]) if want_labels else None for h in heads]
        call = K.CritCall(masks, logits, [_mask_bytes(t["masks"]) for t in targets], [t["labels"].to(torch.int64).contiguous() for t in targets])
        row = col = None
        if N:
            row = _flat([pair[0] for head in indices for pair in head], dev)
            col = _flat([pair[1] for head in indices for pair in head], dev)
        out = [{} for _ in heads]
        if want_labels:
            ce = _ClassLossFn.apply(call, row, col, self.eos_coef, *logits)
            for i in range(n_heads):
                out[i]["loss_ce"] = ce[i]
        if want_masks:
            points = self._select_hip(call, row, over, rnd)
            lm, ld = _MaskLossFn.apply(call, row, col, points, 1.0 / num_masks, *masks)
            for i in range(n_heads):
                out[i]["loss_mask"], out[i]["loss_dice"] = lm[i], ld[i]
        elif "masks" in self.losses:                     # no pair at all: exact zeros that still reach pred_masks, no launch
            for i, h in enumerate(heads):
                out[i]["loss_mask"] = out[i]["loss_dice"] = h["pred_masks"].float().sum() * 0
        return out

    def forward(self, outputs, targets, *, indices=None, point_draws=None) -> Dict[str, torch.Tensor]:
        """outputs: what model.forward_features(batch)[0] returns (pred_logits (bs, Q, C + 1), pred_masks (bs, Q, h, w), aux_outputs);
        targets: per image {"labels": (T,), "masks": (T, H, W) 0 / 1}, one padded size per call (pad_targets).  indices: the result of
        matcher.match_all (default: computed here); point_draws: {"oversampled": (heads, N, M, 2), "random": (heads, N, n_rnd, 2)}."""
        heads = [outputs] + list(outputs.get("aux_outputs", []))
        lg0 = outputs["pred_logits"]
        bs, Q = lg0.shape[:2]
        if len(targets) != bs:
            raise ValueError(f"{len(targets)} targets for a batch of {bs}")
        if indices is None:
            indices = self.matcher.match_all(outputs, targets)
        Ts = [int(t["labels"].shape[0]) for t in targets]
        N = sum(min(Q, T) for T in Ts)
        if len(indices) != len(heads) or any(len(head) != bs for head in indices) or any(
                qi.numel() != min(Q, Ts[b]) or tj.numel() != qi.numel() for head in indices for b, (qi, tj) in enumerate(head)):
            raise ValueError("indices: one (index_i, index_j) pair of min(Q, T) entries per head and image is expected")
        num_masks = self._num_masks(Ts, lg0.device)
        over, rnd = self._draws(len(heads), N, lg0.device, point_draws) if ("masks" in self.losses and N) else (None, None)
        run = self._forward_hip if lg0.is_cuda else self._forward_torch
        per_head = run(heads, targets, indices, over, rnd, num_masks, N)
        losses = dict(per_head[0])
        for i, res in enumerate(per_head[1:]):
            losses.update({f"{k}_{i}": v for k, v in res.items()})
        return losses

    def weighted_sum(self, losses: Dict[str, torch.Tensor]) -> torch.Tensor:
        """sum of weight_dict[k] * losses[k] over the keys weight_dict knows."""
        return sum(losses[k] * self.weight_dict[k] for k in losses if k in self.weight_dict)

    def __repr__(self):
        body = [f"matcher: {self.matcher.__repr__(_repr_indent=8)}", f"losses: {self.losses}", f"weight_dict: {self.weight_dict}",
                f"num_classes: {self.num_classes}", f"eos_coef: {self.eos_coef}", f"num_points: {self.num_points}",
                f"oversample_ratio: {self.oversample_ratio}", f"importance_sample_ratio: {self.importance_sample_ratio}"]
        return "\n".join(["Criterion " + self.__class__.__name__] + ["    " + line for line in body])


def build_criterion(cfg) -> SetCriterion:
    """The criterion of a config: MODEL.ONE_FORMER.{CLASS,MASK,DICE}_WEIGHT for the matcher and the weights (copied to every auxiliary
    head under DEEP_SUPERVISION), NO_OBJECT_WEIGHT, and the three point-sampling keys."""
    of = cfg.MODEL.ONE_FORMER
    matcher = HungarianMatcher(cost_class=of.CLASS_WEIGHT, cost_mask=of.MASK_WEIGHT, cost_dice=of.DICE_WEIGHT, num_points=of.TRAIN_NUM_POINTS)
    base = {"loss_ce": of.CLASS_WEIGHT, "loss_mask": of.MASK_WEIGHT, "loss_dice": of.DICE_WEIGHT}
    weight_dict = dict(base)
    if of.DEEP_SUPERVISION:
        for i in range(of.DEC_LAYERS - 1):
            weight_dict.update({f"{k}_{i}": v for k, v in base.items()})
    return SetCriterion(cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES, matcher=matcher, weight_dict=weight_dict, eos_coef=of.NO_OBJECT_WEIGHT,
                        losses=["labels", "masks"], num_points=of.TRAIN_NUM_POINTS, oversample_ratio=of.OVERSAMPLE_RATIO,
                        importance_sample_ratio=of.IMPORTANCE_SAMPLE_RATIO)
