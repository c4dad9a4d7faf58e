"""Training targets: from a dataset annotation (panoptic id map + segments_info + task) to what HungarianMatcher / SetCriterion take.

The rules are the reference's dataset mapper, model/data/dataset_mappers/oneformer_unified_dataset_mapper.py:138-283 (`_get_semantic_dict`,
`_get_instance_dict`, `_get_panoptic_dict`), which builds one boolean mask per segment with numpy on the host.  Here the id map goes to
the device and the targets are built there (csrc/targets.hip), in a launch count that does not depend on the number of segments.

Per image, over its segment table in order (a row = one entry of segments_info):

    dropped        crowd rows, and rows whose id has no pixel in the map (they count nowhere)
    semantic       one target per class in order of first appearance, the rows of a class merged into it; a class counts once
    instance       the rows of thing classes only, one target each; the label map holds things only
    panoptic       every kept row, one target each, in table order
    label map      the class of the pixel's kept row, `ignore_label` elsewhere (and in the padding)
    texts          "a photo with a {name}" per counted object in `class_names` order, cut at num_texts; the rest is the task's default
                   sentence ("a semantic photo", "an instance photo", "a panoptic photo")

GPU inputs: uenc_targets_area, ONE device-to-host copy of the (B, 256) pixel counts, the host decides the target planes, then
uenc_targets_write.  The counts have to reach the host because the criterion's interface is per-image tensors of T_b targets.
CPU inputs run the same rules as torch ops (`write_torch`, which also runs on GPU tensors: the benchmark's baseline).
"""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

__all__ = ["build_targets", "targets_from_instances", "plan_targets", "write_torch", "TASKS", "MAX_SEGMENTS"]

MAX_SEGMENTS = 256           # rows of one image's segment table: UENC_TARGETS_MAX_SEGMENTS, also the matcher's limit on T
TASKS = {"The task is semantic": ("semantic", "a semantic photo"), "The task is instance": ("instance", "an instance photo"),
         "The task is panoptic": ("panoptic", "a panoptic photo")}


def plan_targets(segments: Sequence[dict], area: Sequence[int], task: str, thing_ids, class_names: Sequence[str], num_texts: int):
    """The host's decisions for one image from the pixel count of every table row -> (slot, cls, labels, texts): per row the target
    plane (-1: none) and the class it writes into the label map (-1: none), the targets' classes, and the num_texts sentences."""
    kind, default = TASKS[task]
    things = set(int(t) for t in thing_ids)
    slot, cls, labels = [-1] * len(segments), [-1] * len(segments), []
    count: Dict[int, int] = {}
    for r, s in enumerate(segments):
        c = int(s["category_id"])
        if s.get("iscrowd", 0) or int(area[r]) == 0 or (kind == "instance" and c not in things):
            continue
        if kind == "semantic":
            if c not in labels:
                labels.append(c)
                count[c] = 1
            slot[r] = labels.index(c)
        else:
            slot[r] = len(labels)
            labels.append(c)
            count[c] = count.get(c, 0) + 1
        cls[r] = c
    texts = [default] * num_texts
    num = 0
    for c, name in enumerate(class_names):
        for _ in range(count.get(c, 0)):
            if num >= num_texts:
                break
            texts[num] = f"a photo with a {name}"
            num += 1
    return slot, cls, labels, texts


def _as_map(m) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(m)) if isinstance(m, np.ndarray) else m
    if not torch.is_tensor(t) or t.dim() != 2 or t.dtype.is_floating_point or t.dtype in (torch.bool, torch.complex64, torch.complex128):
        raise ValueError("build_targets: pan_seg must be (h, w) integer id maps")
    return t if t.dtype in (torch.int32, torch.int64) else t.to(torch.int64)


def _check(pan_seg, segments_info, tasks, size):
    B = len(pan_seg)
    if B == 0 or len(segments_info) != B or len(tasks) != B:
        raise ValueError(f"build_targets: {B} id maps, {len(segments_info)} segment tables and {len(tasks)} tasks")
    H, W = (max(m.shape[0] for m in pan_seg), max(m.shape[1] for m in pan_seg)) if size is None else (int(size[0]), int(size[1]))
    for b, (m, segs, task) in enumerate(zip(pan_seg, segments_info, tasks)):
        if task not in TASKS:
            raise ValueError(f"build_targets: unknown task {task!r} for image {b} (known: {sorted(TASKS)})")
        if len(segs) > MAX_SEGMENTS:
            raise ValueError(f"build_targets: image {b} has {len(segs)} segments, more than 256 segments per image are not supported")
        ids = [int(s["id"]) for s in segs]
        if any(i <= 0 or i > 0x7fffffff for i in ids):
            raise ValueError(f"build_targets: image {b} lists a segment id <= 0 (or beyond int32); 0 is the void id of a panoptic map")
        if len(set(ids)) != len(ids):
            raise ValueError(f"build_targets: image {b} lists a duplicate segment id")
        if m.shape[0] > H or m.shape[1] > W:
            raise ValueError(f"build_targets: the id map of image {b}, {tuple(m.shape)}, is larger than size {(H, W)}")
    return B, H, W


def write_torch(pan: torch.Tensor, ids: Sequence[int], slot: Sequence[int], cls: Sequence[int], T: int, ignore_label: int,
                masks: torch.Tensor, sem: torch.Tensor):
    """One image with torch ops: pan (h, w); masks (T, H, W) uint8 and sem (H, W) int64 are filled in place, padding included."""
    h, w = pan.shape
    masks.zero_()
    sem.fill_(ignore_label)
    rows = [r for r in range(len(ids)) if slot[r] >= 0 or cls[r] >= 0]
    if not rows:
        return
    dev = pan.device
    hit = pan[None] == torch.tensor([ids[r] for r in rows], dtype=pan.dtype, device=dev)[:, None, None]          # (rows, h, w), disjoint
    with_slot = [i for i, r in enumerate(rows) if slot[r] >= 0]
    if with_slot:
        planes = torch.tensor([slot[rows[i]] for i in with_slot], dtype=torch.int64, device=dev)
        masks[:, :h, :w].index_add_(0, planes, hit[with_slot].to(torch.uint8))
    c = torch.tensor([cls[r] if cls[r] >= 0 else ignore_label for r in rows], dtype=torch.int64, device=dev)
    sem[:h, :w] = torch.where(hit.any(0), c[hit.to(torch.uint8).argmax(0)], sem[:h, :w])


def _area_torch(pan: torch.Tensor, ids: Sequence[int]) -> List[int]:
    if not ids:
        return []
    return (pan[None] == torch.tensor(ids, dtype=pan.dtype, device=pan.device)[:, None, None]).flatten(1).sum(1).tolist()


def build_targets(pan_seg, segments_info, tasks, *, thing_ids, class_names, ignore_label: int = 255, num_texts: int,
                  size: Optional[Tuple[int, int]] = None, use_kernels: Optional[bool] = None):
    """pan_seg: per image an (h_i, w_i) integer id map (torch tensor or numpy array; `uenc.data.rgb2id` of the panoptic PNG);
    segments_info: per image a list of {"id", "category_id", "iscrowd"}; tasks: per image "The task is semantic|instance|panoptic";
    thing_ids: the contiguous ids of the thing classes; class_names: name of every class id; size: the padded (H, W), default the
    batch maximum.

    -> targets: per image {"labels": (T,) int64, "masks": (T, H, W) uint8}, as HungarianMatcher / SetCriterion take them, all masks views
       of one allocation; sem_seg (B, H, W) int64; texts: per image num_texts strings.

    Tensors live on the device of pan_seg[0].  On the GPU this call SYNCHRONISES once (the device-to-host copy of the pixel counts,
    from which the host decides how many targets each image has): it belongs in batch staging, before the step, never inside a
    captured region.  use_kernels=False runs the torch-op composition on GPU tensors as well (the benchmark's baseline).

    ValueError: more than 256 segments in one image, a segment id <= 0 or listed twice, an id map larger than `size`, an unknown task."""
    pan_seg = [_as_map(m) for m in pan_seg]
    B, H, W = _check(pan_seg, segments_info, tasks, size)
    dev = pan_seg[0].device
    ids = [[int(s["id"]) for s in segs] for segs in segments_info]
    if use_kernels is None:
        use_kernels = dev.type == "cuda"

    if use_kernels:
        from .. import kernels as K
        S = K.TARGETS_MAX_SEGMENTS
        pan = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
        for b, m in enumerate(pan_seg):
            pan[b, :m.shape[0], :m.shape[1]].copy_(m)
        table = np.zeros(B * (S + 3), dtype=np.int32)
        for b, m in enumerate(pan_seg):
            table[b * S:b * S + len(ids[b])] = ids[b]
            table[B * S + b] = len(ids[b])
            table[B * S + B + 2 * b:B * S + B + 2 * b + 2] = m.shape
        table = torch.from_numpy(table).to(dev)
        area = K.targets_area(pan, table).cpu().tolist()                   # the one synchronisation
    else:
        area = [_area_torch(m.to(dev), ids[b]) for b, m in enumerate(pan_seg)]

    plans = [plan_targets(segments_info[b], area[b], tasks[b], thing_ids, class_names, num_texts) for b in range(B)]
    Ts = [len(p[2]) for p in plans]
    plane0 = [sum(Ts[:b]) for b in range(B)]
    labels = torch.tensor([c for p in plans for c in p[2]], dtype=torch.int64).to(dev)

    if use_kernels:
        plan = np.full(B * (2 * S + 2), -1, dtype=np.int32)
        for b, (slot, cls, _, _) in enumerate(plans):
            plan[b * S:b * S + len(slot)] = slot
            plan[B * S + b * S:B * S + b * S + len(cls)] = cls
            plan[2 * B * S + b], plan[2 * B * S + B + b] = plane0[b], Ts[b]
        masks, sem_seg = K.targets_write(pan, table, torch.from_numpy(plan).to(dev), sum(Ts), ignore_label)
    else:
        masks = torch.empty((sum(Ts), H, W), dtype=torch.uint8, device=dev)
        sem_seg = torch.empty((B, H, W), dtype=torch.int64, device=dev)
        for b, m in enumerate(pan_seg):
            write_torch(m.to(dev), ids[b], plans[b][0], plans[b][1], Ts[b], ignore_label, masks[plane0[b]:plane0[b] + Ts[b]], sem_seg[b])

    targets = [{"labels": labels[plane0[b]:plane0[b] + Ts[b]], "masks": masks[plane0[b]:plane0[b] + Ts[b]]} for b in range(B)]
    return targets, sem_seg, [p[3] for p in plans]


def targets_from_instances(instances, size):
    """The reference mapper's own output (`instances.gt_classes` (T,), `instances.gt_masks` (T, h, w) boolean, a tensor or a BitMasks)
    zero-padded at the bottom and right to size = (H, W): Mask2Former's `prepare_targets`.  -> per image {"labels": (T,) int64,
    "masks": (T, H, W) uint8}, all masks views of one allocation on the device of the first image's masks."""
    H, W = int(size[0]), int(size[1])
    gts = [getattr(i.gt_masks, "tensor", i.gt_masks) for i in instances]
    dev = gts[0].device
    Ts = [int(g.shape[0]) for g in gts]
    for b, g in enumerate(gts):
        if g.dim() != 3 or g.shape[1] > H or g.shape[2] > W:
            raise ValueError(f"targets_from_instances: the masks of image {b}, {tuple(g.shape)}, do not fit into size {(H, W)}")
        if len(instances[b].gt_classes) != Ts[b]:
            raise ValueError(f"targets_from_instances: image {b} has {Ts[b]} masks and {len(instances[b].gt_classes)} classes")
    masks = torch.zeros((sum(Ts), H, W), dtype=torch.uint8, device=dev)
    out, p = [], 0
    for inst, g, T in zip(instances, gts, Ts):
        view = masks[p:p + T]
        view[:, :g.shape[1], :g.shape[2]].copy_(g.to(dev) != 0)
        out.append({"labels": torch.as_tensor(inst.gt_classes).to(device=dev, dtype=torch.int64), "masks": view})
        p += T
    return out
