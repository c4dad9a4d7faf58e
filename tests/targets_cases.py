"""Shared by test_targets_cpu.py and test_targets_gpu.py: the fixture tests/golden/targets.npz (what the reference's dataset mapper makes
of five annotations under the three tasks, tools/make_targets_golden.py), a plain numpy statement of the target rules, and generators
of further annotations."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targets.npz")
TASK_NAMES = ("semantic", "instance", "panoptic")
DEFAULT_TEXT = {"semantic": "a semantic photo", "instance": "an instance photo", "panoptic": "a panoptic photo"}


def prompt(task):
    return f"The task is {task}"


def infos(segs):
    return [{"id": int(i), "category_id": int(c), "iscrowd": int(cr)} for i, c, cr in segs]


_CACHE = {}


def load_fixture():
    """-> (meta, cases): meta = class_names, things, ignore_label; a case = name, pan (h, w) int32, segs (n, 3), num_queries and per task
    {masks (T, h, w) bool, classes (T,), label (h, w) int64, texts [str]}.  Loaded once, never modified by a test."""
    if "fx" not in _CACHE:
        z = np.load(GOLDEN, allow_pickle=False)
        meta = {"class_names": [str(s) for s in z["class_names"]], "things": [int(t) for t in z["things"]], "ignore_label": int(z["ignore_label"])}
        cases = []
        for i, name in enumerate(z["names"]):
            pan = z[f"c{i}_pan"]
            h, w = pan.shape
            c = {"name": str(name), "pan": pan, "segs": z[f"c{i}_segs"], "num_queries": int(z[f"c{i}_num_queries"])}
            for t in TASK_NAMES:
                classes = z[f"c{i}_{t}_classes"]
                T = classes.shape[0]
                masks = np.unpackbits(z[f"c{i}_{t}_masks"])[:T * h * w].reshape(T, h, w).astype(bool)
                c[t] = {"masks": masks, "classes": classes, "label": z[f"c{i}_{t}_label"].astype(np.int64), "texts": [str(s) for s in z[f"c{i}_{t}_texts"]]}
            cases.append(c)
        _CACHE["fx"] = (meta, cases)
    return _CACHE["fx"]


def numpy_targets(pan, segs, task, things, class_names, ignore_label, num_texts):
    """The rules, stated once more with numpy alone: pan (h, w), segs rows of (id, category_id, iscrowd), task one of TASK_NAMES
    -> masks (T, h, w) bool, classes (T,) int64, label (h, w) int64, texts."""
    pan = np.asarray(pan)
    # a segment is kept when it is no crowd, has at least one pixel and, for the instance task, is a thing
    kept = [(int(i), int(c)) for i, c, crowd in segs if not crowd and (pan == i).any() and (task != "instance" or int(c) in things)]
    label = np.full(pan.shape, ignore_label, dtype=np.int64)
    for i, c in kept:
        label[pan == i] = c
    if task == "semantic":
        classes = list(dict.fromkeys(c for _, c in kept))                                  # distinct, in order of first appearance
        masks = [np.isin(pan, [i for i, c2 in kept if c2 == c]) for c in classes]
        objects = classes                                                                  # a class counts once
    else:
        classes = [c for _, c in kept]
        masks = [pan == i for i, _ in kept]
        objects = classes
    named = [f"a photo with a {class_names[c]}" for c in sorted(objects)]                  # class order; equal classes are adjacent
    texts = (named + [DEFAULT_TEXT[task]] * num_texts)[:num_texts]
    masks = np.stack(masks) if masks else np.zeros((0,) + pan.shape, dtype=bool)
    return masks, np.asarray(classes, dtype=np.int64), label, texts


def pad_masks(masks, H, W):
    out = np.zeros((masks.shape[0], H, W), dtype=np.uint8)
    out[:, :masks.shape[1], :masks.shape[2]] = masks
    return out


def pad_label(label, H, W, ignore_label):
    out = np.full((H, W), ignore_label, dtype=np.int64)
    out[:label.shape[0], :label.shape[1]] = label
    return out


def random_annotation(rs, h, w, ids, crowd_every=0, unlisted=0, empty_listed=0, blocks=4):
    """An (h, w) int32 map of rectangular blocks (blocks x blocks pixels each) drawn from `ids`, 0 (void) and `unlisted` further ids,
    and the table: the ids in the given order with classes cycling through 0..18, every crowd_every-th a crowd, plus `empty_listed`
    listed ids that have no pixel."""
    ids = [int(i) for i in ids]
    top = max(ids + [0])
    pool = np.array(ids + [0] + [top + 1 + k for k in range(unlisted)], dtype=np.int64)
    gh, gw = (h + blocks - 1) // blocks, (w + blocks - 1) // blocks
    cells = pool[rs.randint(0, len(pool), size=(gh, gw))]
    pan = np.repeat(np.repeat(cells, blocks, 0), blocks, 1)[:h, :w].astype(np.int32)
    segs = [(i, k % 19, int(bool(crowd_every) and k % crowd_every == crowd_every - 1)) for k, i in enumerate(ids)]
    segs += [(top + 1000 + k, (3 * k) % 19, 0) for k in range(empty_listed)]
    return pan, np.asarray(segs, dtype=np.int64).reshape(-1, 3)


def colliding_ids(n):
    """n distinct positive ids: consecutive integers mixed with multiples of 1024 plus a constant (equal low bits)."""
    half = n // 2
    return [1 + k for k in range(n - half)] + [1024 * (k + 1) + 7 for k in range(half)]
