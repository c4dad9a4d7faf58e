"""tests/golden/targets.npz: what the REFERENCE's dataset mapper (model/data/dataset_mappers/oneformer_unified_dataset_mapper.py:138-283,
`_get_semantic_dict`, `_get_instance_dict`, `_get_panoptic_dict`) makes of five small panoptic annotations, each under all three tasks.

Build container only (needs the reference checkout, oracle.ref_loader.REF_ROOT).  The reference's file is loaded by path and its three
methods are called as they are, unbound, on a plain object that carries the four attributes they read (num_queries, ignore_label,
class_names, things); nothing of its text is restated.  Its own model/utils/box_ops.py is loaded by path as well.  Stand-ins, written
here, only for what the file imports from third parties and this image lacks: detectron2 (`configurable` as the identity, `Instances` as
an attribute bag, `BitMasks` holding `.tensor`, name holders for the data utilities the three methods never touch), fvcore's
HFlipTransform, cv2, the tokenizer and the colour augmentation (name holders).

Cases (Cityscapes' 19 class names, things = classes 11..18):
  a  24 x 37    a crowd segment, a listed segment with no pixel, a map id that is not listed, two instances of one thing class, two
                segments of one stuff class, void (0) pixels
  b  24 x 37    stuff only: the instance task has no target
  c  32 x 40    num_queries 5 with nine objects: more objects than texts
  d  64 x 96    ids up to 2^24 - 1 (the rgb2id range)
  e  96 x 160   60 segments, ids cityscapes-style (class * 1000 + instance)

Per case c{i}: c{i}_pan (h, w) int32, c{i}_segs (n, 3) int32 = id, category_id, iscrowd per listed segment, c{i}_num_queries; per task t in
(semantic, instance, panoptic): c{i}_{t}_masks = np.packbits of gt_masks (T, h, w), c{i}_{t}_classes (T,) int64, c{i}_{t}_label (h, w) int16,
c{i}_{t}_texts (num_queries,) fixed-width strings.  Once: class_names, things, ignore_label, names (the cases' letters), command.

    python tools/make_targets_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "uni-encoder-code_amd"))
from oracle.ref_loader import REF_ROOT  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "targets.npz")
COMMAND = "python tools/make_targets_golden.py"
TASKS = ("semantic", "instance", "panoptic")
IGNORE_LABEL = 255
THINGS = list(range(11, 19))


class _Instances:
    """detectron2.structures.Instances: per-image fields set as attributes."""

    def __init__(self, image_size):
        self.image_size = image_size


class _BitMasks:
    """detectron2.structures.BitMasks: a (N, H, W) boolean tensor under `.tensor`."""

    def __init__(self, tensor):
        self.tensor = tensor.to(torch.bool)


def load_reference_mapper():
    holders = {
        "cv2": {}, "detectron2": {}, "detectron2.config": {"configurable": lambda f=None, **kw: f if f is not None else (lambda g: g)},
        "detectron2.data": {"MetadataCatalog": None, "detection_utils": None, "transforms": None},
        "detectron2.data.detection_utils": {}, "detectron2.data.transforms": {},
        "detectron2.structures": {"BitMasks": _BitMasks, "Instances": _Instances},
        "fvcore": {}, "fvcore.transforms": {}, "fvcore.transforms.transform": {"HFlipTransform": type("HFlipTransform", (), {})},
        "model": {}, "model.utils": {}, "model.data": {}, "model.data.dataset_mappers": {},
        "model.data.tokenizer": {"SimpleTokenizer": None, "Tokenize": None},
        "model.data.dataset_mappers.custom_augs": {"CustomColorAugSSDAugment": None},
    }
    try:
        import torchvision.ops.boxes  # noqa: F401  (box_ops.py imports box_area from it)
    except Exception:
        holders.update({"torchvision": {}, "torchvision.ops": {}, "torchvision.ops.boxes": {"box_area": None}})
    names = list(holders) + ["model.utils.box_ops"]
    saved = {n: sys.modules.get(n) for n in names}
    for n, attrs in holders.items():
        m = types.ModuleType(n)
        m.__dict__.update(attrs)
        sys.modules[n] = m
    sys.modules["detectron2.data"].detection_utils = sys.modules["detectron2.data.detection_utils"]
    sys.modules["detectron2.data"].transforms = sys.modules["detectron2.data.transforms"]

    def by_path(name, rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, "model", rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    try:
        by_path("model.utils.box_ops", "utils/box_ops.py")
        mod = by_path("_reference_unified_mapper", "data/dataset_mappers/oneformer_unified_dataset_mapper.py")
    finally:
        sys.modules.pop("_reference_unified_mapper", None)
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
    return mod


def regions(rs, h, w, k):
    """(h, w) region index in [0, k): every pixel belongs to the nearest of k random sites (each site's own pixel is its own)."""
    yy, xx = np.mgrid[0:h, 0:w]
    cells = rs.choice(h * w, size=k, replace=False)
    sy, sx = cells // w, cells % w
    d = (yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2
    return d.argmin(0)


def make_cases():
    rs = np.random.RandomState(20241020)
    cases = []

    def case(name, h, w, region_ids, segs, num_queries):
        reg = regions(rs, h, w, len(region_ids))
        pan = np.asarray(region_ids, dtype=np.int64)[reg].astype(np.int32)
        assert set(np.unique(pan).tolist()) == set(region_ids), "every region has a pixel"
        cases.append({"name": name, "pan": pan, "segs": np.asarray(segs, dtype=np.int32).reshape(-1, 3), "num_queries": num_queries})

    # a: regions road, road (second segment of the stuff class), car, car, person (crowd), an id the table does not list, sky, void
    case("a", 24, 37, [5, 6, 26001, 26002, 24000, 99, 8, 0],
         [(5, 0, 0), (26001, 13, 0), (33000, 14, 0), (24000, 11, 1), (6, 0, 0), (8, 10, 0), (26002, 13, 0)], 12)
    case("b", 24, 37, [7, 8, 11, 21, 23], [(7, 0, 0), (8, 1, 0), (11, 2, 0), (21, 8, 0), (23, 10, 0)], 12)
    case("c", 32, 40, [1, 2, 3, 4, 5, 6, 7, 8, 9],
         [(1, 13, 0), (2, 0, 0), (3, 13, 0), (4, 11, 0), (5, 8, 0), (6, 11, 0), (7, 18, 0), (8, 0, 0), (9, 2, 0)], 5)
    big = [(1 << 24) - 1, (1 << 24) - 2, 65536, 65537, 256, 257, 1 << 23, (1 << 23) + 1024, 1024, 2048, 3072, 16711680]
    case("d", 64, 96, big + [0], [(i, c, 0) for i, c in zip(big, [11, 11, 0, 1, 13, 13, 10, 8, 17, 18, 2, 5])], 150)
    ids_e, segs_e = [], []
    for k in range(60):
        c = int(rs.randint(0, 19))
        i = c * 1000 + k if c >= 11 else 100 + k           # stuff classes may come in several segments as well
        ids_e.append(i)
        segs_e.append((i, c, int(k % 17 == 5)))
    case("e", 96, 160, ids_e + [0], segs_e, 40)
    return cases


def main():
    from uenc.datasets import CITYSCAPES_CATEGORIES        # the public label table (detectron2 builtin_meta): not reference content
    class_names = [k["name"] for k in CITYSCAPES_CATEGORIES]
    assert len(class_names) == 19
    ref = load_reference_mapper()
    Mapper = ref.OneFormerUnifiedDatasetMapper
    methods = {"semantic": Mapper._get_semantic_dict, "instance": Mapper._get_instance_dict, "panoptic": Mapper._get_panoptic_dict}
    out = {"class_names": np.array(class_names), "things": np.array(THINGS, dtype=np.int64), "ignore_label": np.int64(IGNORE_LABEL),
           "command": np.array(COMMAND)}
    cases = make_cases()
    out["names"] = np.array([c["name"] for c in cases])
    for i, c in enumerate(cases):
        pan, segs = c["pan"], c["segs"]
        h, w = pan.shape
        out[f"c{i}_pan"], out[f"c{i}_segs"], out[f"c{i}_num_queries"] = pan, segs, np.int64(c["num_queries"])
        infos = [{"id": int(a), "category_id": int(b), "iscrowd": int(cr)} for a, b, cr in segs]
        for task in TASKS:
            me = types.SimpleNamespace(num_queries=c["num_queries"], ignore_label=IGNORE_LABEL, class_names=class_names, things=THINGS)
            count = {name: 0 for name in class_names}
            inst, texts, label = methods[task](me, torch.as_tensor(pan.astype(np.int64)), (h, w), infos, count)
            masks = np.asarray(inst.gt_masks.numpy() if torch.is_tensor(inst.gt_masks) else inst.gt_masks).astype(bool).reshape(-1, h, w)
            classes = inst.gt_classes.numpy().astype(np.int64).reshape(-1)
            assert masks.shape[0] == classes.shape[0] and len(texts) == c["num_queries"]
            out[f"c{i}_{task}_masks"] = np.packbits(masks)
            out[f"c{i}_{task}_classes"] = classes
            out[f"c{i}_{task}_label"] = np.asarray(label).astype(np.int16)
            out[f"c{i}_{task}_texts"] = np.array(texts)
            print(f"case {c['name']} {h} x {w} {task}: {len(infos)} listed, T {masks.shape[0]}, "
                  f"labelled {(np.asarray(label) != IGNORE_LABEL).mean():.2f}, object texts {sum(t.startswith('a photo with') for t in texts)}")
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes")
    assert size < (1 << 18)
    np.load(OUT, allow_pickle=False)


if __name__ == "__main__":
    main()
