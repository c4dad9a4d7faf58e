"""Capture one single-GPU training step of the product model as a HIP graph and replay it.

What one step launches is ~1500 kernels whose host-side enqueue costs about as long as the GPU work (BENCH_r03.json `host_enqueue_ms`).
A replay launches the recorded graph at once.  For the replay to compute what the eager step computes, nothing in the captured region may
depend on host decisions taken per step:

  * randomness -- the step runs under `ops.device_rng`: DropPath multipliers and dropout seeds are device tables that
    `uenc_step_rng_advance` rewrites at the start of every replay (it advances the step counter itself);
  * descriptor tables -- staged in a pinned host arena this object owns (`kernels.CAPTURE_ARENA`) and copied by the captured step;
  * inputs -- images and task-token ids live in static device buffers that `step()` refills before the replay.

The captured region: zero the gradients, `ops.begin_step(fresh_grads=True)` (operand re-cast + RNG advance), `model.forward_features`,
`loss_fn`, backward, the weight-gradient flush and, when an optimizer is given, its step (uenc.optim.FusedAdamW: step-count advance,
gradient norm, update -- all of it reads device state only; the per-group learning rates are uploaded by `step()` before the replay).
Post-processing and `upsample_masks` stay outside.  The graph is linear (one stream).
"""
from typing import Callable, List, Optional, Sequence

import torch

from . import kernels as K
from . import ops
from .capi import lib

__all__ = ["GraphedTrainStep"]

_ARENA_BYTES = 4 << 20


def _refuse_unsupported(model):
    if K.EXACT:
        raise RuntimeError("GraphedTrainStep: the fp32 exact mode (UENC_EXACT) cannot be captured; run it eagerly")
    if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        raise RuntimeError(f"GraphedTrainStep: data-parallel world size {torch.distributed.get_world_size()} > 1 -- the gradient all-reduce "
                           "is not captured; capture on a single GPU only")
    if ops._GRAD_LISTENER is not None:
        raise RuntimeError("GraphedTrainStep: a data-parallel gradient listener (uenc.dp) is installed; capture on a single GPU only")
    if lib.uenc_prof_active():
        raise RuntimeError("GraphedTrainStep: the kernel launch timers (uenc_prof_enable) are on; disable them before capturing")
    name = type(getattr(model, "backbone", None)).__name__
    if "Swin" not in name:
        raise ValueError(f"GraphedTrainStep: the Swin backbone is required (got {name}); other backbones run eagerly")


class GraphedTrainStep:
    """Capture `loss_fn(model.forward_features(batch)[0])` + backward once, replay it per step.

    model: a OneFormer built by uenc.d2.build_model (Swin backbone); its train() / eval() mode at construction is the captured one.
    loss_fn(outputs) -> scalar tensor; must be capturable (device ops only, no host copies / syncs).
    example_batch: the list of {"left_image", "task", "type": "segmentation"} dicts that fixes the image shape and batch size.
    warmup: eager steps on a side stream before the capture (they also register every randomness slot).
    seed: base seed of the device RNG (train mode).
    optimizer: a uenc.optim.FusedAdamW over the model's parameters, or None.  With one, every warm-up step and every replay ends with
    its step; the update leaves the gradients as they are, so after a replay `.grad` holds that step's raw gradients.

    step(images, tasks=None) -> (loss, outputs): copies the (B, 3, H, W) images (and, if given, the task prompts) into the static
    buffers, replays, and returns the static loss / output tensors (overwritten by the next replay).  The gradients land in the
    parameters' `.grad` tensors, overwritten at every replay."""

    def __init__(self, model, loss_fn: Callable, example_batch: Sequence[dict], warmup: int = 3, seed: int = 0, optimizer=None):
        _refuse_unsupported(model)
        if optimizer is not None:
            from .optim import FusedAdamW
            if not isinstance(optimizer, FusedAdamW):
                raise TypeError(f"GraphedTrainStep: optimizer must be a uenc.optim.FusedAdamW (got {type(optimizer).__name__}); a host-driven "
                                "optimizer reads learning rates and step counts on the host and cannot be captured")
        self.optimizer = optimizer
        if not example_batch:
            raise ValueError("GraphedTrainStep: empty example batch")
        for x in example_batch:
            if x.get("type", "segmentation") != "segmentation":
                raise ValueError("GraphedTrainStep: sequence-branch inputs (type != 'segmentation') cannot be captured")
        shapes = {tuple(x["left_image"].shape) for x in example_batch}
        if len(shapes) != 1:
            raise ValueError(f"GraphedTrainStep: all images of a captured batch must have one shape, got {sorted(shapes)}")
        self.model, self.loss_fn = model, loss_fn
        self.device = model.device
        self.training = model.training
        self.params = [p for p in model.parameters() if p.requires_grad]
        B = len(example_batch)
        self.images = torch.stack([x["left_image"].to(self.device, torch.float32) for x in example_batch])
        self.tasks = [x["task"] for x in example_batch]
        self.task_tokens = torch.cat([model._task_tokens(t) for t in self.tasks], 0).clone()
        self._batch = [{"left_image": self.images[i], "task": self.tasks[i], "type": "segmentation"} for i in range(B)]
        self.rng = ops.DeviceRNG(seed, self.device)
        self._arena = torch.empty(_ARENA_BYTES, dtype=torch.uint8, pin_memory=True)
        for p in self.params:                   # gradient buffers exist before the capture: replays write into them
            ops.grad_buf(p)

        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            for _ in range(max(int(warmup), 1)):
                self._run()
        torch.cuda.current_stream(self.device).wait_stream(side)
        torch.cuda.synchronize(self.device)

        self.graph = torch.cuda.CUDAGraph()
        K.CAPTURE_ARENA = [self._arena, 0]
        try:
            with torch.cuda.graph(self.graph):
                self.loss, self.outputs = self._run()
        finally:
            K.CAPTURE_ARENA = None
        # the graph reads (and, at its start, rewrites) the bf16 operand copies that existed at capture time: they stay allocated even
        # when the cache replaces an entry (a forward between replays after the weights moved)
        self._operands = [e.operand for e in ops.CACHE._store.values()]
        # likewise the arena chunks its parked partial sums are written to, which CACHE.invalidate() (a checkpoint load) gives back
        self._partials = list(ops.SMALLQ._chunks)
        torch.cuda.synchronize(self.device)

    def _run(self):
        m = self.model
        m.static_task_tokens = self.task_tokens
        try:
            with ops.device_rng(self.rng):
                grads = [p.grad for p in self.params if p.grad is not None]
                if grads:
                    torch._foreach_zero_(grads)
                ops.begin_step(fresh_grads=True)
                out, _ = m.forward_features(self._batch)
                loss = self.loss_fn(out)
                loss.backward()
                ops.flush_wgrads()
                if self.optimizer is not None:
                    self.optimizer.step()
        finally:
            m.static_task_tokens = None
        return loss.detach(), out

    def set_tasks(self, tasks: Sequence[str]):
        """New task prompts for the following replays (an upload outside the graph)."""
        if len(tasks) != len(self.tasks):
            raise ValueError(f"GraphedTrainStep: {len(tasks)} tasks for a captured batch of {len(self.tasks)}")
        self.task_tokens.copy_(torch.cat([self.model._task_tokens(t) for t in tasks], 0))
        self.tasks = list(tasks)

    def step(self, images: torch.Tensor, tasks: Optional[List[str]] = None):
        if self.model.training != self.training:
            raise RuntimeError(f"GraphedTrainStep: captured in {'train' if self.training else 'eval'} mode, the model is now in "
                               f"{'train' if self.model.training else 'eval'} mode -- recapture")
        if K.EXACT:
            raise RuntimeError("GraphedTrainStep: the fp32 exact mode was switched on after the capture")
        if tuple(images.shape) != tuple(self.images.shape):
            raise ValueError(f"GraphedTrainStep: images of shape {tuple(images.shape)} differ from the captured {tuple(self.images.shape)} "
                             "(image size or batch size changed) -- build a new GraphedTrainStep")
        self.images.copy_(images, non_blocking=True)
        if tasks is not None and list(tasks) != self.tasks:
            self.set_tasks(tasks)
        if self.optimizer is not None:
            self.optimizer.sync_groups()        # a scheduler's new learning rates: uploaded outside the graph, like the images
        self.graph.replay()
        if self.optimizer is not None:
            self.optimizer.mark_updated()
        return self.loss, self.outputs
