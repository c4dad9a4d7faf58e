"""Input pipeline + evaluation loop on the CPU: test-time DatasetMapper, ResizeShortestEdge, InferenceSampler,
build_detection_test_loader, inference_on_dataset, SemSegEvaluator, and the `model.*` import surface train_net.py uses."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    import model  # noqa: F401
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    return cfg


def _write_images(tmp_path, sizes):
    from PIL import Image
    g = np.random.default_rng(0)
    dicts = []
    for i, (h, w) in enumerate(sizes):
        arr = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        fn = str(tmp_path / f"img{i}.png")
        Image.fromarray(arr).save(fn)
        dicts.append({"file_name": fn, "height": h, "width": w, "image_id": i, "type": "segmentation",
                      "annotations": [{"bbox": [0, 0, 1, 1]}], "sem_seg_gt": (arr[:, :, 0] % 19).astype(np.int64)})
    return dicts


def test_resize_shortest_edge_sizes():
    from uenc.data import ResizeShortestEdge
    f = ResizeShortestEdge.get_output_shape
    assert f(512, 1024, 384, 1024) == (384, 768)           # the shipped Cityscapes test size (unified_encoder_cityscapes.yaml: 384 / 1024)
    assert f(1024, 2048, 384, 1024) == (384, 768)
    assert f(100, 1000, 384, 1024) == (102, 1024)          # capped by the long edge, rounded half up
    assert f(1000, 100, 384, 1024) == (1024, 102)
    assert f(333, 500, 384, 10000) == (384, 577)
    img = np.zeros((50, 100, 3), dtype=np.uint8); img[:, 50:] = 200
    out = ResizeShortestEdge(25, 1000)(img)
    assert out.shape == (25, 50, 3) and out[:, :20].max() == 0 and out[:, 30:].min() == 200


def test_dataset_mapper_test_time(tmp_path):
    from uenc.data import DatasetMapper
    cfg = _cfg()
    cfg.merge_from_list(["INPUT.SEG_MIN_SIZE_TEST", 32, "INPUT.SEG_MAX_SIZE_TEST", 80, "INPUT.FORMAT", "RGB", "MODEL.TEST.TASK", "semantic"])
    d = _write_images(tmp_path, [(48, 96)])[0]
    out = DatasetMapper(cfg, False)(d)
    assert out["task"] == "The task is semantic" and out["type"] == "segmentation"
    assert out["left_image"].dtype == torch.uint8 and tuple(out["left_image"].shape) == (3, 32, 64)
    assert out["height"] == 48 and out["width"] == 96 and "annotations" not in out            # outputs are asked for at the original size
    assert "annotations" in d                                                              # the input dict was not modified
    # RGB order: channel 0 of the tensor is the file's red channel (checked on an un-resized read)
    from PIL import Image
    raw = np.asarray(Image.open(d["file_name"]))
    same = DatasetMapper(is_train=False, seg_augmentations=[], image_format="RGB", task="panoptic")(d)
    assert np.array_equal(same["left_image"].numpy(), raw.transpose(2, 0, 1))
    bgr = DatasetMapper(is_train=False, seg_augmentations=[], image_format="BGR", task="panoptic")(d)
    assert np.array_equal(bgr["left_image"].numpy()[0], raw[:, :, 2])
    with pytest.raises(ValueError):
        DatasetMapper(cfg, False)({"file_name": d["file_name"], "type": "detection"})
    with pytest.raises(ValueError):                                                        # size check of detection_utils.check_image_size
        DatasetMapper(cfg, False)({**d, "width": 97})
    with pytest.raises(NotImplementedError):
        DatasetMapper(cfg, True)


def test_test_loader_and_sampler(tmp_path):
    from uenc.data import DatasetCatalog, InferenceSampler, build_detection_test_loader
    cfg = _cfg()
    cfg.merge_from_list(["INPUT.SEG_MIN_SIZE_TEST", 32, "INPUT.SEG_MAX_SIZE_TEST", 64, "DATALOADER.NUM_WORKERS", 0])
    dicts = _write_images(tmp_path, [(40, 56)] * 5)
    name = "uenc_test_synthetic_%d" % os.getpid()
    DatasetCatalog.register(name, lambda: dicts)
    loader = build_detection_test_loader(cfg, name)
    batches = list(loader)
    assert len(batches) == 5 and all(isinstance(b, list) and len(b) == 1 for b in batches)
    assert [b[0]["image_id"] for b in batches] == [0, 1, 2, 3, 4]
    # shards over ranks cover every index exactly once
    parts = [list(InferenceSampler(11, rank=r, world_size=4)) for r in range(4)]
    assert sorted(sum(parts, [])) == list(range(11)) and [len(p) for p in parts] == [3, 3, 3, 2]
    with pytest.raises(KeyError):
        DatasetCatalog.get("not_registered")


def test_inference_on_dataset_and_semseg_evaluator(tmp_path, caplog):
    from uenc.data import DatasetMapper, build_detection_test_loader
    from uenc.evaluation import DatasetEvaluators, SemSegEvaluator, inference_on_dataset
    dicts = _write_images(tmp_path, [(24, 32)] * 8)
    mapper = DatasetMapper(is_train=False, seg_augmentations=[], image_format="RGB", task="semantic")
    loader = build_detection_test_loader(dicts, mapper=mapper)

    class Oracle(torch.nn.Module):          # predicts the ground truth for even images, class 0 everywhere for odd ones
        def forward(self, inputs):
            assert not self.training and not torch.is_grad_enabled()
            outs = []
            for x in inputs:
                gt = torch.as_tensor(x["sem_seg_gt"])
                sem = torch.zeros(19, *gt.shape)
                if x["image_id"] % 2 == 0:
                    sem.scatter_(0, gt[None], 1.0)
                else:
                    sem[0] = 1.0
                outs.append({"sem_seg": sem})
            return outs
    m = Oracle().train()
    stats = {}
    with caplog.at_level(logging.INFO, logger="uenc.evaluation"):
        res = inference_on_dataset(m, loader, [SemSegEvaluator(19)], stats=stats)
    assert m.training                                              # mode restored
    assert any("Total inference time:" in r.message and "s / iter per device, on 1 devices" in r.message for r in caplog.records)
    assert stats["iterations"] == 3 and stats["warmup"] == 5       # min(5, total - 1) warm-up iterations are not timed
    r = res["sem_seg"]
    gt = np.stack([d["sem_seg_gt"] for d in dicts])
    want_pacc = 100.0 * (np.sum(gt[0::2] == gt[0::2]) + np.sum(gt[1::2] == 0)) / gt.size
    assert abs(r["pACC"] - want_pacc) < 1e-9 and 0 < r["mIoU"] < 100
    assert inference_on_dataset(m, loader, None) == {}
    with pytest.raises(AssertionError):
        DatasetEvaluators([SemSegEvaluator(19), SemSegEvaluator(19)]).reset() or inference_on_dataset(m, loader, [SemSegEvaluator(19), SemSegEvaluator(19)])


def test_model_package_import_surface():
    """The `model.*` names train_net.py:43-65 and demo/demo.py:26-31 import resolve against the facade."""
    import model
    from model import InstanceSegEvaluator, add_common_config, add_swin_config, add_uni_encoder_config  # noqa: F401
    from model.data.build import build_detection_test_loader  # noqa: F401
    from model.data.dataset_mappers.dataset_mapper import DatasetMapper  # noqa: F401
    from model.evaluation import COCOEvaluator, CityscapesDepthEvaluator, CityscapesInstanceEvaluator, KITTIDepthEvaluator  # noqa: F401
    from model.data.datasets import register_cityscapes_panoptic, register_kitti  # noqa: F401  (registers the splits on import)
    from uenc.datasets import _catalog_names
    assert "cityscapes_fine_panoptic_val" in _catalog_names() and "KITTI_standard_eigen_test_split" in _catalog_names()
    assert KITTIDepthEvaluator("KITTI_standard_eigen_test_split") is not None and CityscapesDepthEvaluator("x") is not None
    from model.utils.events import MLflowWriter, set_environment_variables, setup_mlflow  # noqa: F401
    assert hasattr(model, "add_dinat_config")
    for cls in (InstanceSegEvaluator, COCOEvaluator, CityscapesInstanceEvaluator, MLflowWriter):
        with pytest.raises(NotImplementedError):
            cls()


# ---------------------------------------------------------------------------------------------------------------------
# fixture-backed: tests/golden/data_eval.npz was produced by the REFERENCE's own functions (oracle/make_data_eval_golden.py) on the
# seeded inputs of oracle/data_eval_inputs.py, which are rebuilt here and fed to the product
# ---------------------------------------------------------------------------------------------------------------------
def _fixture():
    import json
    z = np.load(os.path.join(ROOT, "tests", "golden", "data_eval.npz"), allow_pickle=False)
    return z, json.loads(bytes(z["meta_json"]).decode())


def test_compute_errors_matches_the_reference():
    from oracle.data_eval_inputs import random_depths
    from uenc.evaluation import compute_errors
    z, _ = _fixture()
    np.testing.assert_allclose(np.asarray(compute_errors(*random_depths()), dtype=np.float64), z["compute_errors"], rtol=1e-12, atol=0)


def test_kitti_depth_map_and_evaluation_match_the_reference(tmp_path):
    """generate_depth_map (velodyne -> camera-2 depth map, incl. the closest-point rule for pixels hit twice) and the per-image
    Eigen-crop / median-scaling / clamping / averaging of KITTIDepthEvaluator.evaluate, against the reference's outputs."""
    from oracle.data_eval_inputs import depth_pairs, kitti_calibration, velodyne_scan
    from uenc.evaluation import KITTIDepthEvaluator
    z, _ = _fixture()
    calib = kitti_calibration(str(tmp_path))
    velo = str(tmp_path / "scan.bin")
    velodyne_scan().tofile(velo)
    depth = KITTIDepthEvaluator.generate_depth_map(calib, velo, 2, True)
    assert depth.shape == z["depth_map"].shape and int((depth > 0).sum()) == int(z["depth_map_nonzero"][0]) > 1000
    np.testing.assert_array_equal(depth.astype(np.float32), z["depth_map"])               # bit-exact: same float64 arithmetic
    ev = KITTIDepthEvaluator("KITTI_standard_eigen_test_split")
    ev.reset()
    ev._pairs = list(depth_pairs())
    got = ev.evaluate()["depth_error"]
    np.testing.assert_allclose([got[k] for k in ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")], z["kitti_depth_error"], rtol=1e-12)


def test_kitti_depth_evaluator_process_end_to_end(tmp_path):
    """process(): disparity -> depth at the ground-truth resolution (bilinear, half-pixel centres: cv2.resize's default, which
    is not in the reference tree -- this step is checked against its definition, not a fixture): a prediction that IS the
    ground truth (up to the median scale) scores abs_rel ~ 0 and a1 = 1."""
    from oracle.data_eval_inputs import kitti_calibration, velodyne_scan
    from uenc.evaluation import KITTIDepthEvaluator, disp_to_depth
    calib = kitti_calibration(str(tmp_path))
    velo = str(tmp_path / "scan.bin")
    velodyne_scan(n=200000, seed=5).tofile(velo)                    # dense enough that the Eigen crop holds valid pixels
    gt = KITTIDepthEvaluator.generate_depth_map(calib, velo, 2, True)
    depth = np.where(gt > 0, gt, 10.0) * 0.5                           # predicted depth = half the truth: median scaling must undo it
    scaled = 1.0 / depth
    disp = (scaled - 0.01) / (10.0 - 0.01)                             # inverse of disp_to_depth's affine map
    s, d = disp_to_depth(torch.as_tensor(disp))
    assert torch.allclose(d, torch.as_tensor(depth), rtol=1e-6)
    ev = KITTIDepthEvaluator("x")
    ev.reset()
    ev.process([{"calib_path": calib, "velo_file": velo, "file_name": "a/b/c/d.jpg"}], [{"disp_results": torch.as_tensor(disp, dtype=torch.float32)[None, None]}])
    r = ev.evaluate()["depth_error"]
    assert r["abs_rel"] < 1e-5 and r["a1"] == 1.0 and r["rmse"] < 1e-3


def test_inference_on_dataset_matches_the_reference(caplog):
    """Same toy model / recording evaluator / 8 batches as the fixture run of the reference's inference_on_dataset: identical results,
    evaluator call sequence, train/eval mode handling and log lines (up to the measured times)."""
    import re
    from oracle.data_eval_inputs import toy_batches
    from uenc.evaluation import DatasetEvaluator, inference_on_dataset
    _, meta = _fixture()
    want = meta["inference"]
    calls = []

    class Rec(DatasetEvaluator):
        def reset(self):
            calls.append("reset")

        def process(self, inputs, outputs):
            calls.append(["process", [i["id"] for i in inputs], [float(o["y"]) for o in outputs]])

        def evaluate(self):
            calls.append("evaluate")
            return {"toy": {"sum": float(sum(c[2][0] for c in calls if isinstance(c, list)))}}

    class Toy(torch.nn.Module):
        seen = []

        def forward(self, inputs):
            Toy.seen.append(self.training)
            assert not torch.is_grad_enabled()
            return [{"y": torch.tensor(float(i["id"]) * 2.0 + 1.0)} for i in inputs]
    toy = Toy().train()
    with caplog.at_level(logging.INFO, logger="uenc.evaluation"):
        res = inference_on_dataset(toy, toy_batches(), [Rec()])
    assert res == want["results"] and calls == want["calls"] and Toy.seen == want["mode_inside"] and toy.training == want["mode_after"]
    assert inference_on_dataset(Toy(), toy_batches(), None) == want["none_evaluator_returns"] == {}
    blank = lambda s: re.sub(r"[0-9]+:[0-9]{2}:[0-9]{2}(\.[0-9]+)?|[0-9]+\.[0-9]+", "#", s)      # durations and seconds
    assert [blank(r.message) for r in caplog.records] == [blank(s) for s in want["log_lines"]]


def test_dataset_registration_matches_the_reference(tmp_path, monkeypatch):
    """Cityscapes panoptic and KITTI sequence dataset dicts from synthetic trees, and the registered names / metadata, against what the
    reference's register_cityscapes_panoptic.py / register_kitti.py produced on the same trees."""
    from oracle.data_eval_inputs import make_cityscapes_tree, make_kitti_tree
    from uenc import datasets as DS
    from uenc.data import DatasetCatalog, MetadataCatalog
    _, meta = _fixture()
    # the trees live under a relative, dot-free root: the loader derives sem_seg_file_name with `path.split(".")[0]`, as the reference
    # does (register_cityscapes_panoptic.py:93), which a dot anywhere in the temporary directory's absolute path would cut short
    monkeypatch.chdir(tmp_path)
    croot = "cs"
    image_dir, gt_dir, gt_json = make_cityscapes_tree(croot)
    dicts = DS.load_cityscapes_panoptic(image_dir, gt_dir, gt_json, DS.cityscapes_panoptic_meta())
    rel = lambda d, root: {k: (os.path.relpath(v, root) if isinstance(v, str) and v.startswith(root) else v) for k, v in d.items()}
    assert [rel(d, croot) for d in dicts] == meta["cityscapes_dicts"]
    assert {d["type"] for d in dicts} == {"segmentation"} and dicts[0]["segments_info"][1]["category_id"] == 13        # car: label id 26 -> train id 13
    kroot = "kitti"
    data_root, files_list = make_kitti_tree(kroot)
    kd = DS.load_kitti_sequence(data_root, files_list, ".jpg")
    assert [rel(d, kroot) for d in kd] == meta["kitti_dicts"]
    assert kd[0]["left_prev_image_file"] is not None and kd[1]["left_prev_image_file"] is None and len(kd) == 2        # the missing frame is skipped
    # registration under a root: names, lazy loading, metadata
    os.makedirs(os.path.join(croot, "kitti_data"), exist_ok=True)
    DS.register_all(croot)
    names = DS._catalog_names()
    assert sorted(n for n in names if n.startswith("cityscapes")) == meta["registered_cityscapes"]
    assert sorted(n for n in names if n.startswith("KITTI")) == meta["registered_kitti"]
    got = DatasetCatalog.get("cityscapes_fine_panoptic_val")
    assert [rel(d, croot) for d in got] == meta["cityscapes_dicts"]
    md = MetadataCatalog.get("cityscapes_fine_panoptic_val")
    want = meta["cityscapes_metadata"]
    for k, v in want.items():
        g = getattr(md, k)
        if isinstance(g, dict):
            g = {str(a): b for a, b in g.items()}
        elif isinstance(g, str) and g.startswith(croot):
            continue                                                   # paths: rooted differently in the fixture run
        assert (json_norm(g) == json_norm(v)) or isinstance(v, str), k
    assert MetadataCatalog.get("KITTI_standard_eigen_test_split").evaluator_type == meta["kitti_metadata"]["evaluator_type"] == "kitti_depth"
    DS.register_all(croot)                                             # re-registration replaces, as the reference's `remove` + `register`


def json_norm(x):
    import json
    return json.loads(json.dumps(x))


def test_sequence_mapper_feeds_the_sequence_branch(tmp_path):
    """A KITTI "sequence" dataset dict through DatasetMapper.process_sequence_data (reference dataset_mapper.py:290-332): every frame is
    read at 192 x 640 (PIL LANCZOS, the mapper's own reader), goes through the depth test transform, and comes out under the keys
    OneFormer._forward_sequence reads."""
    from PIL import Image
    from oracle.data_eval_inputs import make_kitti_tree
    from uenc import datasets as DS
    from uenc.data import DatasetMapper
    cfg = _cfg()
    cfg.merge_from_list(["INPUT.DEPTH_MIN_SIZE_TEST", 96, "INPUT.DEPTH_MAX_SIZE_TEST", 512, "INPUT.FORMAT", "RGB"])
    data_root, files_list = make_kitti_tree(str(tmp_path))
    full, alone = DS.load_kitti_sequence(data_root, files_list, ".jpg")
    m = DatasetMapper(cfg, False)
    out = m(full)
    assert out["type"] == "sequence" and (out["height"], out["width"]) == (192, 640)
    for k in ("left_image", "left_prev_image", "left_next_image"):
        assert out[k].dtype == torch.uint8 and tuple(out[k].shape) == (3, 96, 320), k       # 192 x 640 -> shortest edge 96
    # the reader: LANCZOS resize of the file to 640 x 192, then the transform (PIL bilinear)
    want = np.asarray(Image.open(full["left_prev_image_file"]).resize((640, 192), Image.LANCZOS).convert("RGB").resize((320, 96), Image.BILINEAR))
    assert np.array_equal(out["left_prev_image"].numpy(), want.transpose(2, 0, 1))
    assert "left_prev_image_file" in full and "left_image" not in full                       # the input dict is untouched
    solo = m(alone)
    assert "left_prev_image" not in solo and "left_next_image" not in solo and tuple(solo["left_image"].shape) == (3, 96, 320)
    with pytest.raises(ValueError):
        m({**full, "width": 641, "height": 192})
