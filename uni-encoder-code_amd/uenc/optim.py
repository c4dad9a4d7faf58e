"""The optimizer of the training loop: AdamW with the reference's full-model gradient clipping, as HIP kernels that read nothing from the
host -- so the step can be launched eagerly or recorded at the end of a captured training step (uenc.graphs.GraphedTrainStep).

The reference (tools/calc_throughput.py `build_optimizer`) wraps torch.optim.AdamW so that every step first replaces NaN / inf in every
gradient (`torch.nan_to_num(grad, nan=0, posinf=1e5, neginf=-1e5)`), then clips the norm over ALL gradients (`clip_grad_norm_`), then
updates.  `FusedAdamW.step()` is that composition in three entry points of csrc/optim.hip over one device table of segments:

    uenc_optim_advance       step count += 1 on the device, bias corrections of the new step
    uenc_optim_grad_sqnorm   norm of the sanitised gradients -> clip coefficient        (skipped when clipping is off)
    uenc_optim_adamw_step    one pass over parameter, gradient, exp_avg, exp_avg_sq of every tensor

The gradients are only read: after a step `param.grad` still holds the raw gradients of that step.

`build_optimizer(cfg, model)` restates the reference's parameter-group policy and returns a FusedAdamW.
"""
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from . import kernels as K

__all__ = ["FusedAdamW", "build_optimizer"]

_TILE = 4096                    # OPT_TILE of csrc/optim.hip
_MAX_GRID = 2048
_SEG = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("tile_begin", "<i8"), ("group", "<i4"), ("pad", "<i4")])
assert _SEG.itemsize == 56
_STATE = np.dtype([("step", "<i8"), ("norm", "<f8"), ("clip_coef", "<f4"), ("inv_bc1", "<f4"), ("inv_sqrt_bc2", "<f4"), ("pad", "<f4")])
assert _STATE.itemsize == 32


class FusedAdamW(torch.optim.Optimizer):
    """torch.optim.AdamW (no amsgrad, no maximize) preceded by nan_to_num on every gradient and, if `max_grad_norm` is given,
    `clip_grad_norm_(all parameters, max_grad_norm)`.

    `param_groups` are torch's: a scheduler that writes `group["lr"]` works unchanged (step() uploads the per-group lr / weight_decay
    array when it differs from what the device holds).  The moments live in flat fp32 buffers; `state[p]["exp_avg"]` / `["exp_avg_sq"]`
    are views of them and `state[p]["step"]` a tensor, so state_dict() / load_state_dict() interoperate with torch.optim.AdamW.
    Parameters whose `.grad` is None are skipped.  The kernels and uenc.dp.GradBuckets own the gradient storage: zero_grad() defaults
    to set_to_none=False.

    CUDA fp32 parameters run the HIP kernels.  CPU parameters, and the fp32 verification mode (UENC_EXACT), run torch's own
    nan_to_num / clip_grad_norm_ / functional AdamW instead."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None):
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"FusedAdamW: max_grad_norm must be positive or None, got {max_grad_norm}")
        # the group keys of this torch's AdamW (amsgrad, maximize, decoupled_weight_decay, ...), so that a state_dict of ours loaded into
        # torch.optim.AdamW configures it as AdamW
        defaults = dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(()))], lr=lr, betas=betas, eps=eps,
                                          weight_decay=weight_decay).defaults)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._chunks: List[torch.Tensor] = []       # flat moment storage (kept alive; state holds views)
        self._table = None                          # (device table, n, total_tiles, pointer signature, parameters in it)
        self._dstate = None                         # 32-byte device state block
        self._dgroups = None                        # (n_groups, 4) fp32 on the device
        self._groups_host = None                    # what _dgroups holds
        self._partials = None
        self._step_t = torch.zeros((), dtype=torch.float32)     # device path: the one step tensor every updated parameter's state shares
        self._pending_step: Optional[int] = None    # a step count to write to the device state (load_state_dict)

    # ---- which path -------------------------------------------------------------------------------------------------------------
    def _all_params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _on_device(self) -> bool:
        ps = self._all_params()
        return bool(ps) and all(p.is_cuda for p in ps) and not K.EXACT

    def zero_grad(self, set_to_none: bool = False):
        super().zero_grad(set_to_none=set_to_none)

    # ---- state ------------------------------------------------------------------------------------------------------------------
    def _alloc_moments(self, params: List[torch.Tensor], like: Optional[Dict[int, Dict[str, torch.Tensor]]] = None):
        """exp_avg / exp_avg_sq of `params` as views of one new flat buffer each (every view starts on a 16-byte boundary)."""
        if not params:
            return
        offs, total = [], 0
        for p in params:
            offs.append(total)
            total += -(-p.numel() // 4) * 4
        dev = params[0].device
        m = torch.zeros(total, dtype=torch.float32, device=dev)
        v = torch.zeros(total, dtype=torch.float32, device=dev)
        self._chunks += [m, v]
        for p, o in zip(params, offs):
            st = self.state[p]
            em, ev = m[o:o + p.numel()].view(p.shape), v[o:o + p.numel()].view(p.shape)
            if like is not None:
                em.copy_(like[id(p)]["exp_avg"])
                ev.copy_(like[id(p)]["exp_avg_sq"])
            st["exp_avg"], st["exp_avg_sq"] = em, ev

    def state_dict(self):
        sd = super().state_dict()
        # the shared step tensor of the device path leaves as one tensor per parameter (torch's load_state_dict keeps "step" tensors
        # as they are, and its AdamW increments each of them)
        sd["state"] = {k: {kk: (vv.clone() if kk == "step" and torch.is_tensor(vv) else vv) for kk, vv in st.items()}
                       for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW.load_state_dict during a stream capture")
        super().load_state_dict(state_dict)
        self._table = None
        self._groups_host = None
        loaded = [p for p in self._all_params() if len(self.state.get(p, {})) != 0]
        steps = [float(self.state[p]["step"]) for p in loaded]
        top = max(steps) if steps else 0.0
        if self._on_device():
            like = {id(p): {k: self.state[p][k] for k in ("exp_avg", "exp_avg_sq")} for p in loaded}
            self._chunks = []
            self._alloc_moments(loaded, like)
            self._step_t = torch.tensor(top, dtype=torch.float32)
            for p, s in zip(loaded, steps):
                self.state[p]["step"] = self._step_t if s == top else torch.tensor(s, dtype=torch.float32)
            self._pending_step = int(top)
        else:
            for p in loaded:                    # own tensors: the loaded ones may alias the optimizer the dict came from
                st = self.state[p]
                for k in ("exp_avg", "exp_avg_sq", "step"):
                    st[k] = st[k].clone()

    # ---- device tables ----------------------------------------------------------------------------------------------------------
    def _signature(self):
        return tuple((p.data_ptr(), -1 if p.grad is None else p.grad.data_ptr()) for g in self.param_groups for p in g["params"])

    def _hyper(self):
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise NotImplementedError("FusedAdamW: betas and eps are launch arguments, they must be the same in every parameter group")
            if g.get("amsgrad") or g.get("maximize"):
                raise NotImplementedError("FusedAdamW: amsgrad / maximize are not implemented")
        return float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])

    def _build_table(self, sig):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW: a parameter or gradient pointer changed (or no step ran yet), so the segment table has to be "
                               "rebuilt, and a stream capture is in progress -- run one optimizer step eagerly before capturing, and do "
                               "not re-point .grad (GradBuckets re-lays its buffer after the calibration step) afterwards")
        dev = self._all_params()[0].device
        cur = float(self._step_t)
        rows, used, fresh = [], [], []
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                st = self.state[p] if p in self.state else None
                if p.grad is None:
                    if st and st.get("step") is self._step_t:   # dropped out of the update: its own step count stays behind
                        st["step"] = self._step_t.clone()
                    continue
                if p.device != dev:
                    raise NotImplementedError("FusedAdamW: all parameters must live on one device")
                if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or not p.is_contiguous() or not p.grad.is_contiguous() \
                        or p.grad.is_sparse or p.grad.numel() != p.numel():
                    raise NotImplementedError(f"FusedAdamW: parameters and gradients must be dense contiguous fp32 (got {p.dtype} "
                                              f"{tuple(p.shape)}, grad {p.grad.dtype})")
                if not st:
                    if cur != 0:
                        raise NotImplementedError(f"FusedAdamW: a parameter {tuple(p.shape)} received its first gradient after {int(cur)} steps; "
                                                  "the device step count is shared by all parameters")
                    fresh.append(p)
                elif float(st["step"]) != cur:
                    raise NotImplementedError(f"FusedAdamW: a parameter {tuple(p.shape)} is at step {int(float(st['step']))}, the optimizer at "
                                              f"{int(cur)}; the device step count is shared by all parameters")
                used.append((p, gi))
        self._alloc_moments(fresh)
        tb = 0
        for p, gi in used:
            st = self.state[p]
            st["step"] = self._step_t
            rows.append((p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(), tb, gi, 0))
            tb += -(-(p.numel() + ((p.data_ptr() >> 2) & 3)) // _TILE)
        if not rows:
            self._table = (None, 0, 0, sig, [])
            return
        tab = torch.from_numpy(np.array(rows, dtype=_SEG).view(np.uint8).reshape(-1).copy()).to(dev)
        if self._partials is None or self._partials.device != dev:
            self._partials = torch.zeros(_MAX_GRID, dtype=torch.float64, device=dev)
        self._table = (tab, len(rows), tb, sig, [p for p, _ in used])

    def _write_state(self, step: int):
        dev = self._all_params()[0].device
        host = np.zeros(1, dtype=_STATE)
        host["step"], host["clip_coef"] = step, 1.0
        t = torch.from_numpy(host.view(np.uint8).reshape(-1).copy())
        if self._dstate is None or self._dstate.device != dev:
            self._dstate = t.to(dev)
        else:
            self._dstate.copy_(t)

    def sync_groups(self):
        """Upload the per-group {lr, weight_decay, 1 - lr * weight_decay} array if it differs from what the device holds (a scheduler
        wrote group["lr"]).  step() calls it; GraphedTrainStep.step() calls it before a replay, outside the graph."""
        vals = [(float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups]
        if vals == self._groups_host and self._dgroups is not None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("FusedAdamW: a learning rate or weight decay changed during a stream capture; the per-group array is "
                               "uploaded outside the graph")
        arr = np.array([(lr, wd, 1.0 - lr * wd, 0.0) for lr, wd in vals], dtype=np.float32)
        t = torch.from_numpy(arr)
        dev = self._all_params()[0].device
        if self._dgroups is None or self._dgroups.shape != t.shape or self._dgroups.device != dev:
            self._dgroups = t.to(dev)
        else:
            self._dgroups.copy_(t)
        self._groups_host = vals

    def _prepare(self):
        sig = self._signature()
        if self._table is None or self._table[3] != sig:
            self._build_table(sig)
        if self._dstate is None or self._pending_step is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdamW: the device state block has to be written and a stream capture is in progress -- run one "
                                   "optimizer step eagerly first")
            self._write_state(int(self._pending_step if self._pending_step is not None else float(self._step_t)))
            self._pending_step = None
        self.sync_groups()

    def mark_updated(self, steps: int = 1):
        """Host bookkeeping after the device updated the weights `steps` times (step() itself, or a graph replay that contains it): the
        shared step tensor advances and the parameters' versions are bumped, so that the bf16 operand cache (ops.CACHE) re-casts an
        operand it is asked for without an `ops.begin_step()` in between.  A begin_step() re-casts everything in its one launch and
        records the new versions, so a training loop pays nothing twice."""
        self._step_t += steps
        if self._table is not None and self._table[4]:
            torch.autograd.graph.increment_version(self._table[4])

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._on_device():
            self._step_torch()
            return loss
        from .capi import check, lib, stream_ptr
        b1, b2, eps = self._hyper()
        self._prepare()
        tab, n, tiles, _, _ = self._table
        if n == 0:
            return loss
        s = stream_ptr()
        check(lib.uenc_optim_advance(self._dstate.data_ptr(), b1, b2, s), "optim_advance")
        if self.max_grad_norm is not None:
            check(lib.uenc_optim_grad_sqnorm(tab.data_ptr(), n, tiles, self._partials.data_ptr(), self._partials.numel(),
                                             self._dstate.data_ptr(), self.max_grad_norm, s), "optim_grad_sqnorm")
        check(lib.uenc_optim_adamw_step(tab.data_ptr(), n, tiles, self._dgroups.data_ptr(), len(self.param_groups), self._dstate.data_ptr(),
                                        b1, b2, eps, s), "optim_adamw_step")
        if not torch.cuda.is_current_stream_capturing():        # a capture records the launches, nothing ran: replays are counted
            self.mark_updated()                                 # by whoever replays (GraphedTrainStep.step)
        return loss

    def device_state(self) -> Dict[str, Any]:
        """The device state block read back (a synchronisation: logging and tests): step count, total gradient norm of the last step,
        clip coefficient."""
        if self._dstate is None:
            return {"step": int(float(self._step_t)), "grad_norm": 0.0, "clip_coef": 1.0}
        rec = self._dstate.cpu().numpy().view(_STATE)[0]
        return {"step": int(rec["step"]), "grad_norm": float(rec["norm"]), "clip_coef": float(rec["clip_coef"])}

    def _step_torch(self):
        """The reference's composition on torch itself (CPU parameters, verification mode)."""
        from torch.optim.adamw import adamw as functional_adamw
        every = [p for p in self._all_params() if p.grad is not None]
        saved = [p.grad.clone() for p in every]                 # torch works in place; the raw gradients are put back below
        for p in every:
            torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)
        if self.max_grad_norm is not None and every:
            torch.nn.utils.clip_grad_norm_(every, self.max_grad_norm)
        for g in self.param_groups:
            ps = [p for p in g["params"] if p.grad is not None]
            if not ps:
                continue
            for p in ps:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif st["step"] is self._step_t:
                    st["step"] = self._step_t.clone()
            functional_adamw(ps, [p.grad for p in ps], [self.state[p]["exp_avg"] for p in ps], [self.state[p]["exp_avg_sq"] for p in ps], [],
                             [self.state[p]["step"] for p in ps], amsgrad=False, beta1=g["betas"][0], beta2=g["betas"][1], lr=g["lr"],
                             weight_decay=g["weight_decay"], eps=g["eps"], maximize=False)
        for p, s in zip(every, saved):
            p.grad.copy_(s)


_NORM_TYPES = (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm, torch.nn.GroupNorm,
               torch.nn.InstanceNorm1d, torch.nn.InstanceNorm2d, torch.nn.InstanceNorm3d, torch.nn.LayerNorm, torch.nn.LocalResponseNorm)


def param_groups(cfg, model) -> List[Dict[str, Any]]:
    """One group per trainable tensor, the reference's policy (tools/calc_throughput.py `build_optimizer`).  Four rules, applied in
    this order, a later one overriding an earlier one:
      lr           = SOLVER.BASE_LR, times SOLVER.BACKBONE_MULTIPLIER when the MODULE's name contains "backbone";
      weight decay = SOLVER.WEIGHT_DECAY,
                     0 when the PARAMETER's name contains "relative_position_bias_table" or "absolute_pos_embed",
                     SOLVER.WEIGHT_DECAY_NORM when the module is a normalisation layer,
                     SOLVER.WEIGHT_DECAY_EMBED when the module is an nn.Embedding.
    A tensor shared by several modules is taken where it is met first."""
    S = cfg.SOLVER
    base_lr, base_wd = float(S.BASE_LR), float(S.WEIGHT_DECAY)
    wd_norm = float(getattr(S, "WEIGHT_DECAY_NORM", 0.0))
    wd_embed = float(getattr(S, "WEIGHT_DECAY_EMBED", 0.0))
    mult = float(getattr(S, "BACKBONE_MULTIPLIER", 1.0))
    groups, seen = [], set()
    for mname, module in model.named_modules():
        for pname, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            lr = base_lr * mult if "backbone" in mname else base_lr
            wd = base_wd
            if "relative_position_bias_table" in pname or "absolute_pos_embed" in pname:
                wd = 0.0
            if isinstance(module, _NORM_TYPES):
                wd = wd_norm
            if isinstance(module, torch.nn.Embedding):
                wd = wd_embed
            groups.append({"params": [p], "lr": lr, "weight_decay": wd})
    return groups


def build_optimizer(cfg, model) -> FusedAdamW:
    """The optimizer the reference's trainer builds from SOLVER.*: per-tensor groups (`param_groups`), AdamW, and full-model gradient
    clipping when SOLVER.CLIP_GRADIENTS.ENABLED with CLIP_TYPE "full_model" and CLIP_VALUE > 0."""
    S = cfg.SOLVER
    kind = getattr(S, "OPTIMIZER", "ADAMW")
    if kind == "SGD":
        raise NotImplementedError('SOLVER.OPTIMIZER = "SGD" is not implemented (every shipped configuration trains with "ADAMW")')
    if kind != "ADAMW":
        raise NotImplementedError(f"SOLVER.OPTIMIZER = {kind!r}: no such optimizer type")
    clip = getattr(S, "CLIP_GRADIENTS", None)
    max_norm = None
    if clip is not None and clip.ENABLED:
        if clip.CLIP_TYPE != "full_model":
            raise NotImplementedError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE = {clip.CLIP_TYPE!r}: only \"full_model\" clipping is implemented "
                                      "(the per-parameter \"value\" / \"norm\" types are Detectron2's, not the reference's)")
        if float(clip.CLIP_VALUE) > 0.0:
            max_norm = float(clip.CLIP_VALUE)
    return FusedAdamW(param_groups(cfg, model), lr=float(S.BASE_LR), max_grad_norm=max_norm)
