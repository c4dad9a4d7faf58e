"""The two training mappers and the training loader of uenc/train_data.py on PNG files written to tmp_path, with seeded generators.
The augment="host" output is held against a straight-line composition written here in the reference's order (PIL resize, crop, colour,
flip, pad, with the plan's numbers); every comparison is equality.  No GPU."""
import itertools
import json
import random

import numpy as np
import pytest
import torch
from PIL import Image

from uenc import train_data as T
from uenc.data import MetadataCatalog, read_sequence_image

H, W = 24, 48
SEGMENTS = [{"id": 1000 * (11 + k) + k, "category_id": 11 + k, "iscrowd": 0} for k in range(3)] + [{"id": 7, "category_id": 7, "iscrowd": 0}]


def _meta():
    return MetadataCatalog.get("augment_test_train").set(
        thing_dataset_id_to_contiguous_id={24 + k: 11 + k for k in range(8)}, stuff_classes=[f"class{c}" for c in range(19)], ignore_label=255)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("train_mappers")
    rng = np.random.RandomState(3)
    names = {}
    for key in ("file_name", "right_file_name", "left_prev_image_file", "left_nxt_image_file"):
        names[key] = str(root / f"{key}.png")
        Image.fromarray(rng.randint(0, 256, (H, W, 3)).astype(np.uint8)).save(names[key])
    seg = np.kron(rng.randint(0, 4, (H // 6, W // 8)), np.ones((6, 8), dtype=np.int64))
    ids = np.array([s["id"] for s in SEGMENTS])[seg]
    pan = np.stack([ids & 255, (ids >> 8) & 255, (ids >> 16) & 255], -1).astype(np.uint8)
    names["pan"] = str(root / "pan.png")
    Image.fromarray(pan).save(names["pan"])
    label = np.array([s["category_id"] for s in SEGMENTS])[seg].astype(np.uint8)
    label[rng.rand(H, W) < 0.1] = 255
    names["label"] = str(root / "label.png")
    Image.fromarray(label).save(names["label"])
    names["cam"] = str(root / "camera.json")
    with open(names["cam"], "w") as f:
        json.dump({"extrinsic": {"baseline": 0.209313}, "intrinsic": {"fx": 2262.52, "fy": 2265.30, "u0": 1096.98, "v0": 513.137}}, f)
    return names


def _unified_dict(files):
    return {"file_name": files["file_name"], "right_file_name": files["right_file_name"], "left_prev_image_file": files["left_prev_image_file"],
            "left_nxt_image_file": files["left_nxt_image_file"], "left_pan_seg_file_name": files["pan"], "left_sem_seg_file_name": files["label"],
            "left_segments_info": SEGMENTS, "cam_info_file": files["cam"], "height": H, "width": W, "image_id": "a"}


def _seg_dict(files, **kw):
    d = {"type": "segmentation", "file_name": files["file_name"], "pan_seg_file_name": files["pan"], "sem_seg_file_name": files["label"],
         "segments_info": SEGMENTS, "height": H, "width": W, "image_id": "a"}
    d.update(kw)
    return d


def _seq_dict(files):
    return {"type": "sequence", "file_name": files["file_name"], "left_prev_image_file": files["left_prev_image_file"],
            "left_nxt_image_file": files["left_nxt_image_file"], "cam_info_file": files["cam"]}


def _aug(flip, size_divisibility=-1, max_area=0.9, colour=True):
    return T.TrainAugmentation((12, 24, 36, 48), 4096, "choice", crop_enabled=True, crop_size=(16, 24), single_category_max_area=max_area,
                               ignored_category=255, colour_ssd=colour, image_format="RGB", flip=flip, size_divisibility=size_divisibility)


def _straight_line(plan, path, kind):
    """One file through the reference's sequence of transforms, with the plan's numbers."""
    (nh, nw), (x0, y0, cw, ch), (OH, OW) = plan.resized_hw, plan.crop, plan.out_hw
    amounts = [0, OW - cw, 0, OH - ch]
    if kind == "image":
        img = np.asarray(Image.open(path).convert("RGB"))
        img = np.asarray(Image.fromarray(img).resize((nw, nh), Image.BILINEAR))[y0:y0 + ch, x0:x0 + cw]
        img = T.ssd_colour(img, plan.colour)
        img = np.flip(img, axis=1) if plan.flip else img
        return torch.nn.functional.pad(torch.as_tensor(np.ascontiguousarray(img.transpose(2, 0, 1))), amounts, value=128)
    if kind == "pan":
        seg = np.asarray(Image.open(path).convert("RGB"))
        seg = np.asarray(Image.fromarray(seg).resize((nw, nh), Image.NEAREST))[y0:y0 + ch, x0:x0 + cw]
        seg = (np.flip(seg, axis=1) if plan.flip else seg).astype(np.int64)
        ids = seg[:, :, 0] + 256 * seg[:, :, 1] + 65536 * seg[:, :, 2]
        return torch.nn.functional.pad(torch.as_tensor(ids), amounts, value=0)
    lab = np.asarray(Image.open(path)).astype("double")
    t = torch.from_numpy(lab).view(lab.shape[0], lab.shape[1], 1, 1).permute(2, 3, 0, 1)
    lab = torch.nn.functional.interpolate(t, (nh, nw), mode="nearest")[0, 0].numpy()[y0:y0 + ch, x0:x0 + cw]
    lab = np.flip(lab, axis=1) if plan.flip else lab
    return torch.nn.functional.pad(torch.as_tensor(lab.astype("long")), amounts, value=255)


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


def _task(rng, sem=0.33, ins=0.66):
    p = rng.uniform(0, 1.)
    return "The task is semantic" if p < sem else ("The task is instance" if p < ins else "The task is panoptic")


@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("size_divisibility", [-1, 32, 8])
def test_unified_mapper_equals_the_straight_line_composition(files, seed, size_divisibility):
    aug = _aug(False, size_divisibility)
    a, pa = np.random.RandomState(seed), random.Random(seed)
    mapper = T.OneFormerUnifiedDatasetMapper(name="augment_test_train", num_queries=8, meta=_meta(), augmentations=aug, image_format="RGB",
                                             size_divisibility=size_divisibility, np_rng=a, py_rng=pa)
    src = _unified_dict(files)
    out = mapper(src)
    assert "left_pan_seg_file_name" in src and "left_image" not in src                    # the input dict is not modified
    b, pb = np.random.RandomState(seed), random.Random(seed)
    label = np.asarray(Image.open(files["label"]))
    plan = aug.plan(H, W, label, b, pb)
    assert not plan.flip and plan.colour is not None
    task = _task(b)
    for key, name in T.OneFormerUnifiedDatasetMapper.FRAMES:
        ref = _straight_line(plan, files[name], "image")
        assert out[key].dtype == torch.uint8 and torch.equal(out[key], ref), key
    assert out["pan_seg"].dtype == torch.int32 and torch.equal(out["pan_seg"].long(), _straight_line(plan, files["pan"], "pan"))
    assert torch.equal(out["sem_seg_gt"].long(), _straight_line(plan, files["label"], "label"))
    assert out["task"] == task and out["segments_info"] == SEGMENTS and out["thing_ids"] == list(range(11, 19))
    assert tuple(out["orig_shape"]) == tuple(out["left_image"].shape[-2:]) == plan.out_hw
    assert out["baseline"] == 0.209313
    K = np.array([[2262.52 / 2048 * 512, 0, 256, 0], [0, 2265.30 / 1024 * 256, 128, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
    assert torch.equal(out["K"], torch.from_numpy(K)) and torch.equal(out["inv_K"], torch.from_numpy(np.linalg.pinv(K)).float())
    assert out["stereo_T"][0, 3] == np.float32(-0.1) and torch.equal(out["stereo_T"][:3, :3], torch.eye(3))
    assert _same_state(a, b) and pa.getstate() == pb.getstate()


@pytest.mark.parametrize("seed", range(6))
def test_multi_pass_segmentation_equals_the_straight_line_composition(files, seed):
    aug = _aug(True, 32 if seed % 2 else -1, max_area=0.8)
    a, pa = np.random.RandomState(seed), random.Random(seed)
    mapper = T.OneFormerUnifiedMultiPassCityscapesMapper(name="augment_test_train", num_queries=8, meta=_meta(), seg_augmentations=aug,
                                                         size_divisibility=aug.size_divisibility, np_rng=a, py_rng=pa)
    out = mapper(_seg_dict(files))
    b, pb = np.random.RandomState(seed), random.Random(seed)
    plan = aug.plan(H, W, np.asarray(Image.open(files["label"])), b, pb)
    task = _task(b)
    assert torch.equal(out["left_image"], _straight_line(plan, files["file_name"], "image"))
    assert torch.equal(out["pan_seg"].long(), _straight_line(plan, files["pan"], "pan"))
    assert torch.equal(out["sem_seg_gt"].long(), _straight_line(plan, files["label"], "label"))
    assert out["task"] == task and out["type"] == "segmentation" and "pan_seg_file_name" not in out
    assert _same_state(a, b) and pa.getstate() == pb.getstate()


def test_flips_occur_and_both_paths_leave_the_generators_in_the_same_state(files):
    aug = _aug(True)
    flips = set()
    for seed in range(8):
        gens = [(np.random.RandomState(seed), random.Random(seed)) for _ in range(2)]
        outs = [T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=aug, augment=mode, np_rng=g[0],
                                                     py_rng=g[1])(_seg_dict(files)) for mode, g in zip(("host", "device"), gens)]
        rec = outs[1]["_augment"]
        flips.add(rec["plan"].flip)
        assert "left_image" not in outs[1] and rec["keys"] == ["left_image"] and rec["meta"]["F"] == 1
        at = rec["off"]["frame0"]                                            # the untouched source frame travels in the packed buffer
        assert np.array_equal(rec["buf"].numpy()[at:at + H * W * 3].reshape(H, W, 3), np.asarray(Image.open(files["file_name"]).convert("RGB")))
        assert outs[0]["task"] == outs[1]["task"] and tuple(outs[0]["orig_shape"]) == rec["plan"].out_hw
        assert _same_state(gens[0][0], gens[1][0]) and gens[0][1].getstate() == gens[1][1].getstate()
    assert flips == {True, False}


@pytest.mark.parametrize("probs,expect", [((0.33, 0.66), (0.33, 0.33, 0.34)), ((0.2, 0.7), (0.2, 0.5, 0.3))])
def test_task_frequencies_follow_task_prob(files, probs, expect):
    aug = T.TrainAugmentation((24,), 4096, "choice")
    rng = np.random.RandomState(17)
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=aug, semantic_prob=probs[0],
                                                  instance_prob=probs[1], np_rng=rng, py_rng=random.Random(0))
    n = 600
    tasks = [mapper(_seg_dict(files))["task"] for _ in range(n)]
    # the literal replay of the draws: one `choice` for the resize, then the task's uniform
    replay = np.random.RandomState(17)
    want = []
    for _ in range(n):
        replay.choice((24,))
        want.append(_task(replay, *probs))
    assert tasks == want
    for name, p in zip(("semantic", "instance", "panoptic"), expect):
        share = tasks.count(f"The task is {name}") / n
        assert abs(share - p) < 4.5 * (p * (1 - p) / n) ** 0.5, (name, share)       # 4.5 standard deviations of the binomial share


def test_sequence_dicts_flip_the_frames_and_the_principal_point(files):
    seen = set()
    for seed in range(8):
        rng = np.random.RandomState(seed)
        mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True), np_rng=rng,
                                                      py_rng=random.Random(seed))
        out = mapper(_seq_dict(files))
        flip = bool(np.random.RandomState(seed).uniform(0, 1.0) < 0.5)
        seen.add(flip)
        u0 = 1096.98 / 2048.0 * 512.0
        K = np.array([[2262.52 / 2048.0 * 512.0, 0, 512. - u0 if flip else u0, 0], [0, 2265.30 / 768.0 * 192.0, 513.137 / 768.0 * 192.0, 0],
                      [0, 0, 1, 0], [0, 0, 0, 1]], dtype=np.float32)
        assert torch.equal(out["K"], torch.from_numpy(K)) and torch.equal(out["inv_K"], torch.from_numpy(np.linalg.pinv(K)).float())
        for key, name in (("left_image", "file_name"), ("left_prev_image", "left_prev_image_file"), ("left_next_image", "left_nxt_image_file")):
            img = read_sequence_image(files[name], format="RGB", dataset="cs")
            img = np.flip(img, axis=1) if flip else img
            ref = torch.as_tensor(np.ascontiguousarray(img.transpose(2, 0, 1)))
            assert out[key].shape == (3, 192, 512) and torch.equal(out[key], ref) and torch.equal(out["orig_" + key], ref)
    assert seen == {True, False}


def test_sequence_dicts_are_padded(files):
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True), size_divisibility=256,
                                                  np_rng=np.random.RandomState(0), py_rng=random.Random(0))
    out = mapper(_seq_dict(files))
    assert out["left_image"].shape == (3, 256, 256) and bool((out["left_image"][:, 192:] == 128).all())      # grows below, crops at the right
    assert torch.equal(out["orig_left_next_image"], out["left_next_image"])


def _cfg():
    import model  # noqa: F401
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    _meta()
    cfg.merge_from_list(["DATASETS.TRAIN", ("augment_test_train",), "INPUT.FORMAT", "RGB", "INPUT.CROP.ENABLED", True, "INPUT.CROP.TYPE", "absolute",
                         "INPUT.CROP.SIZE", (16, 24), "INPUT.SEG_CROP.ENABLED", True, "INPUT.SEG_CROP.SIZE", (16, 24),
                         "INPUT.SEG_MIN_SIZE_TRAIN", (12, 24, 48), "INPUT.SEG_MAX_SIZE_TRAIN", 4096, "INPUT.COLOR_AUG_SSD", True,
                         "INPUT.SEG_COLOR_AUG_SSD", True])
    return cfg


def test_from_config_and_the_mapper_name_binding(files):
    cfg = _cfg()
    m = T.build_train_mapper(cfg, np_rng=np.random.RandomState(0), py_rng=random.Random(0))
    assert isinstance(m, T.OneFormerUnifiedDatasetMapper) and m.tfm_gens.crop_size == (16, 24) and not m.tfm_gens.flip and m.tfm_gens.colour_ssd
    assert m.num_queries == cfg.MODEL.ONE_FORMER.NUM_OBJECT_QUERIES - cfg.MODEL.TEXT_ENCODER.N_CTX and m.things == list(range(11, 19))
    assert m(_unified_dict(files))["left_image"].shape[0] == 3
    cfg.merge_from_list(["INPUT.DATASET_MAPPER_NAME", "oneformer_unified_multi_pass"])
    m = T.build_train_mapper(cfg, np_rng=np.random.RandomState(0), py_rng=random.Random(0))
    assert isinstance(m, T.OneFormerUnifiedMultiPassCityscapesMapper) and m.seg_tfm_gens.flip
    assert m(_seg_dict(files))["pan_seg"].dtype == torch.int32
    cfg.merge_from_list(["INPUT.DATASET_MAPPER_NAME", "coco_unified_lsj"])
    with pytest.raises(NotImplementedError, match="DATASET_MAPPER_NAME"):
        T.build_train_mapper(cfg)


def test_refusals(files):
    cfg = _cfg()
    cfg.merge_from_list(["INPUT.CROP.TYPE", "relative_range"])
    with pytest.raises(NotImplementedError, match="INPUT.CROP.TYPE"):
        T.OneFormerUnifiedDatasetMapper(cfg, True)
    cfg = _cfg()
    cfg.merge_from_list(["INPUT.SEG_CROP.TYPE", "relative"])
    with pytest.raises(NotImplementedError, match="INPUT.SEG_CROP.TYPE"):
        T.OneFormerUnifiedMultiPassCityscapesMapper(cfg, True)
    cfg = _cfg()
    cfg.merge_from_list(["INPUT.DEPTH_COLOR_JITTER", True])
    with pytest.raises(NotImplementedError, match="INPUT.DEPTH_COLOR_JITTER"):
        T.OneFormerUnifiedMultiPassCityscapesMapper(cfg, True)
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True, max_area=0.5),
                                                  np_rng=np.random.RandomState(0), py_rng=random.Random(0))
    d = _seg_dict(files)
    del d["sem_seg_file_name"]
    with pytest.raises(ValueError, match="label map"):
        mapper(d)
    with pytest.raises(ValueError, match="annotations"):
        mapper(_seg_dict(files, annotations=[]))
    with pytest.raises(ValueError, match="Unknown dataset type"):
        mapper({"type": "depth"})
    with pytest.raises(AssertionError):
        T.OneFormerUnifiedDatasetMapper(is_train=False, name="x", num_queries=8, meta=_meta(), augmentations=_aug(False))
    with pytest.raises(ValueError, match="augment"):
        T.OneFormerUnifiedDatasetMapper(name="x", num_queries=8, meta=_meta(), augmentations=_aug(False), augment="gpu")


def test_reference_module_names_import():
    import model  # noqa: F401
    from model.data.build import build_detection_train_loader
    from model.data.dataset_mappers.oneformer_multi_pass_cityscapes_mapper import OneFormerUnifiedMultiPassCityscapesMapper
    from model.data.dataset_mappers.oneformer_unified_dataset_mapper import OneFormerUnifiedDatasetMapper
    assert OneFormerUnifiedDatasetMapper is T.OneFormerUnifiedDatasetMapper
    assert OneFormerUnifiedMultiPassCityscapesMapper is T.OneFormerUnifiedMultiPassCityscapesMapper is T.OneFormerMultiPassCityscapesMapper
    assert build_detection_train_loader is T.build_detection_train_loader


def test_with_instances_adds_the_reference_keys(files):
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=6, meta=_meta(), seg_augmentations=_aug(True), with_instances=True,
                                                  np_rng=np.random.RandomState(2), py_rng=random.Random(2))
    out = mapper(_seg_dict(files))
    inst = out["instances"]
    assert inst.gt_masks.dtype == torch.bool and inst.gt_masks.shape[1:] == out["pan_seg"].shape and len(inst.gt_classes) == inst.gt_masks.shape[0]
    assert len(out["text"]) == 6 and out["sem_seg"].shape == out["pan_seg"].shape and out["sem_seg"].dtype == torch.int64
    kept = {s["category_id"] for s in SEGMENTS if bool((out["pan_seg"] == s["id"]).any())}
    if out["task"] != "The task is instance":
        assert set(inst.gt_classes.tolist()) == kept


class _Probe:
    """A mapper wrapper for a worker process: records whether the GPU runtime was initialised by the mapping."""

    def __init__(self, mapper):
        self.mapper = mapper

    def __call__(self, d):
        out = self.mapper(d)
        out["cuda_initialized"] = torch.cuda.is_initialized()
        return out


def test_device_mapping_in_a_worker_touches_no_gpu_api(files):
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True), augment="device")
    loader = torch.utils.data.DataLoader(T._MapDataset([_seg_dict(files)] * 3, _Probe(mapper)), batch_size=1, num_workers=1,
                                         collate_fn=T.trivial_batch_collator, worker_init_fn=T._worker_init_reset_seed)
    n = 0
    for (d,) in loader:
        assert d["cuda_initialized"] is False and isinstance(d["_augment"]["plan"], T.AugPlan)
        buf = d["_augment"]["buf"]
        assert torch.is_tensor(buf) and buf.dtype == torch.uint8 and not buf.is_cuda and not any(torch.is_tensor(v) and v.is_cuda for v in d.values())
        n += 1
    assert n == 3


def test_training_sampler_and_loader(files):
    one = list(itertools.islice(T.TrainingSampler(5, seed=3, rank=0, world_size=1), 20))
    assert all(sorted(one[i:i + 5]) == list(range(5)) for i in (0, 5, 10, 15)) and len({tuple(one[i:i + 5]) for i in (0, 5, 10, 15)}) > 1
    assert one == list(itertools.islice(T.TrainingSampler(5, seed=3, rank=0, world_size=1), 20))          # seeded
    r0 = list(itertools.islice(T.TrainingSampler(5, seed=3, rank=0, world_size=2), 10))
    r1 = list(itertools.islice(T.TrainingSampler(5, seed=3, rank=1, world_size=2), 10))
    assert [x for pair in zip(r0, r1) for x in pair] == one                                                # rank-sharded: one stream, dealt out
    assert list(itertools.islice(T.TrainingSampler(3, shuffle=False), 7)) == [0, 1, 2, 0, 1, 2, 0]
    dicts = [_seg_dict(files, image_id=str(i)) for i in range(3)] + [_seq_dict(files)]
    mapper = T.OneFormerMultiPassCityscapesMapper(name="x", num_queries=8, meta=_meta(), seg_augmentations=_aug(True),
                                                  np_rng=np.random.RandomState(0), py_rng=random.Random(0))
    loader = T.build_detection_train_loader(dicts, mapper=mapper, total_batch_size=2, augment="host", seed=1, world_size=1)
    batches = list(itertools.islice(iter(loader), 4))                                                      # more than one pass: the stream is infinite
    assert all(isinstance(b, list) and len(b) == 2 for b in batches)
    for d in (d for b in batches for d in b):
        assert d["left_image"].dtype == torch.uint8 and ("pan_seg" in d) == (d["type"] == "segmentation")
    with pytest.raises(ValueError, match="divisible"):
        T.build_detection_train_loader(dicts, mapper=mapper, total_batch_size=3, world_size=2)
    with pytest.raises(ValueError, match="mapper"):
        T.build_detection_train_loader(dicts, total_batch_size=2)
