"""The device path of the training mappers: `apply_plans` equals the augment="host" dict on every key, bit for bit, for both mappers
and a handful of seeds; and a two-image batch of the multi-pass mapper trains the small OneFormer of tests/test_targets_gpu.py."""
import itertools
import random

import numpy as np
import pytest
import torch
from PIL import Image

from uenc import train_data as T
from uenc.data import MetadataCatalog

pytestmark = pytest.mark.gpu

H, W = 64, 96
SEGMENTS = [{"id": 1000 * (11 + k) + k, "category_id": 11 + k, "iscrowd": 0} for k in range(3)] + [{"id": 7, "category_id": 7, "iscrowd": 0},
                                                                                                 {"id": 2, "category_id": 2, "iscrowd": 1}]


def _meta():
    return MetadataCatalog.get("augment_gpu_test_train").set(
        thing_dataset_id_to_contiguous_id={24 + k: 11 + k for k in range(8)}, stuff_classes=[f"class{c}" for c in range(19)], ignore_label=255)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_mappers_gpu")
    rng = np.random.RandomState(5)
    names = {}
    for key in ("file_name", "right_file_name", "left_prev_image_file", "left_nxt_image_file"):
        names[key] = str(root / f"{key}.png")
        Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(names[key])
    seg = np.kron(rng.randint(0, 5, (H // 8, W // 8)), np.ones((8, 8), dtype=np.int64))
    ids = np.array([s["id"] for s in SEGMENTS])[seg]
    names["pan"] = str(root / "pan.png")
    Image.fromarray(np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], -1).astype(np.uint8)).save(names["pan"])
    names["label"] = str(root / "label.png")
    Image.fromarray(np.array([s["category_id"] for s in SEGMENTS])[seg].astype(np.uint8)).save(names["label"])
    return names


def _aug(flip, size_divisibility=-1, sizes=(32, 64, 80, 128)):
    return T.TrainAugmentation(sizes, 4096, "choice", crop_enabled=True, crop_size=(64, 96), single_category_max_area=0.9,
                               ignored_category=255, colour_ssd=True, image_format="RGB", flip=flip, size_divisibility=size_divisibility)


def _seg_dict(files):
    return {"type": "segmentation", "file_name": files["file_name"], "pan_seg_file_name": files["pan"], "sem_seg_file_name": files["label"],
            "segments_info": SEGMENTS, "height": H, "width": W}


def _unified_dict(files):
    return {"file_name": files["file_name"], "right_file_name": files["right_file_name"], "left_prev_image_file": files["left_prev_image_file"],
            "left_nxt_image_file": files["left_nxt_image_file"], "left_pan_seg_file_name": files["pan"], "left_sem_seg_file_name": files["label"],
            "left_segments_info": SEGMENTS, "cam_info_file": None, "height": H, "width": W}


def _assert_same_dict(dev: dict, host: dict):
    assert set(dev) == set(host), set(dev) ^ set(host)
    for k, v in host.items():
        if torch.is_tensor(v):
            assert torch.is_tensor(dev[k]) and dev[k].dtype == v.dtype and torch.equal(dev[k].cpu(), v), k
        else:
            assert dev[k] == v, k


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("which", ["unified", "multi_pass"])
def test_apply_plans_equals_the_host_dict(files, which, seed):
    outs = []
    for mode in ("host", "device"):
        gens = dict(np_rng=np.random.RandomState(seed), py_rng=random.Random(seed))
        if which == "unified":
            mapper = T.OneFormerUnifiedDatasetMapper(name="x", num_queries=8, meta=_meta(), augmentations=_aug(False, 32 if seed == 3 else -1),
                                                     size_divisibility=32 if seed == 3 else -1, augment=mode, **gens)
            outs.append(mapper(_unified_dict(files)))
        else:
            mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True, 128 if seed == 3 else -1),
                                                          size_divisibility=128 if seed == 3 else -1, augment=mode, **gens)
            outs.append(mapper(_seg_dict(files)))
    host, dev = outs
    assert "_augment" in dev and "left_image" not in dev
    (dev,) = T.apply_plans([dev], "cuda")
    torch.cuda.synchronize()
    assert dev["left_image"].is_cuda and dev["pan_seg"].is_cuda
    _assert_same_dict(dev, host)


def test_with_instances_on_the_device_path(files):
    outs = []
    for mode in ("host", "device"):
        mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=6, meta=_meta(), seg_augmentations=_aug(True), with_instances=True,
                                                      augment=mode, np_rng=np.random.RandomState(4), py_rng=random.Random(4))
        outs.append(mapper(_seg_dict(files)))
    host, (dev,) = outs[0], T.apply_plans([outs[1]], "cuda")
    assert dev["text"] == host["text"] and torch.equal(dev["sem_seg"].cpu(), host["sem_seg"])
    assert torch.equal(dev["instances"].gt_classes.cpu(), host["instances"].gt_classes)
    assert torch.equal(dev["instances"].gt_masks.cpu(), host["instances"].gt_masks)


def test_a_mapped_batch_trains_the_small_model(files):
    import model  # noqa: F401
    from test_targets_gpu import _criterion, _small_train_model
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True, sizes=(64, 80, 128)), augment="device",
                                                  np_rng=np.random.RandomState(9), py_rng=random.Random(9))
    loader = T.build_detection_train_loader([_seg_dict(files)] * 4, mapper=mapper, total_batch_size=2, seed=0, world_size=1, device="cuda")
    (batch,) = list(itertools.islice(iter(loader), 1))
    assert len(batch) == 2 and all(d["left_image"].is_cuda and d["left_image"].shape == (3, 64, 96) and "_augment" not in d for d in batch)
    m = _small_train_model()
    m.set_criterion(_criterion().cuda())
    torch.manual_seed(0)
    losses = m(batch)
    assert isinstance(losses, dict) and {"loss_ce", "loss_mask", "loss_dice"} <= set(losses)
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    sum(losses.values()).backward()
    from uenc import ops
    ops.flush_wgrads()
    torch.cuda.synchronize()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().sum()) > 0 for g in grads)
