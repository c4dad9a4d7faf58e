"""The segmentation evaluators on the host (no GPU): PanopticEvaluator against hand-worked literals and the mask-based numpy oracle of
pq_cases.py, the PNG ground truth through rgb2id, COCOPanopticEvaluator / build_evaluator from registered metadata, and SemSegEvaluator's
default path pinned to the bytes it gave before it learnt accumulate="device"."""
import numpy as np
import pytest
import torch

from pq_cases import KEYS, LITERALS, infos, numpy_pq, random_case


def _feed(ev, images, tensors=False):
    ev.reset()
    for pred, pred_segs, gt, gt_segs in images:
        p = torch.from_numpy(pred) if tensors else pred
        ev.process([{"pan_seg": gt, "segments_info": infos(gt_segs)}], [{"panoptic_seg": (p, infos(pred_segs))}])
    return ev.evaluate()["panoptic_seg"]


@pytest.mark.parametrize("case", LITERALS, ids=[c[0] for c in LITERALS])
def test_host_panoptic_equals_the_literals(case):
    from uenc.evaluation import PanopticEvaluator
    _, images, things, K, expect, counts = case
    ev = PanopticEvaluator(things, K)
    res = _feed(ev, images)
    assert tuple(res) == KEYS
    assert res == expect
    assert {k: ev._stats[k].tolist() for k in ("tp", "fp", "fn")} == counts
    oracle, oracle_counts = numpy_pq(images, things, K)                 # the oracle itself reproduces the hand-worked figures
    assert oracle == expect and oracle_counts == counts


def test_host_panoptic_equals_the_oracle_on_random_maps():
    from uenc.evaluation import PanopticEvaluator
    rs = np.random.RandomState(11)
    K, things = 7, [3, 4, 5, 6]
    images = [random_case(rs, 33, 47, range(1, 13), range(101, 112), K),
              random_case(rs, 40, 64, [1000 * k + 3 for k in range(1, 30)], range(1, 25), K, crowd_every=3),
              random_case(rs, 20, 20, [], range(1, 4), K, unlisted_gt=0),                   # no ground-truth segment
              random_case(rs, 20, 20, range(1, 6), [], K)]                                  # no prediction
    res = _feed(PanopticEvaluator(things, K), images, tensors=True)
    oracle, _ = numpy_pq(images, things, K)
    assert res == oracle
    assert 0 < res["PQ"] < 100 and res["RQ_th"] > 0                      # the maps do produce matches, misses and false positives


def test_host_panoptic_has_no_segment_cap_and_reports_unknown_predictions():
    from uenc.evaluation import PanopticEvaluator
    n = 300
    gt = np.arange(1, n + 1, dtype=np.int32).reshape(15, 20)
    segs = [(i, i % 5, 0) for i in range(1, n + 1)]
    res = _feed(PanopticEvaluator([0, 1], 5), [(gt, [(i, c) for i, c, _ in segs], gt, segs)])
    assert res["PQ"] == 100.0 and res["RQ_st"] == 100.0
    ev = PanopticEvaluator([0, 1], 5)
    ev.process([{"pan_seg": gt, "segments_info": infos(segs)}], [{"panoptic_seg": (gt, infos([(1, 1)]))}])
    with pytest.raises(ValueError, match="does not list"):
        ev.evaluate()
    with pytest.raises(ValueError, match="category"):
        ev.process([{"pan_seg": gt, "segments_info": infos([(1, 5, 0)])}], [{"panoptic_seg": (gt, [])}])


def test_png_ground_truth_goes_through_rgb2id(tmp_path):
    from PIL import Image
    from uenc.evaluation import PanopticEvaluator, rgb2id
    ids = np.array([[0, 26001, 26001], [300, 300, 70000], [70000, 70000, 16777215]], dtype=np.int64)
    rgb = np.stack([ids % 256, ids // 256 % 256, ids // 65536], axis=-1).astype(np.uint8)
    path = tmp_path / "pan.png"
    Image.fromarray(rgb).save(path)
    assert np.array_equal(rgb2id(np.asarray(Image.open(path))), ids)
    assert rgb2id((1, 2, 3)) == 1 + 256 * 2 + 65536 * 3
    segs = [(26001, 1, 0), (300, 0, 0), (70000, 1, 0), (16777215, 0, 0)]
    ev = PanopticEvaluator([1], 2)
    ev.process([{"pan_seg_file_name": str(path), "segments_info": infos(segs)}], [{"panoptic_seg": (ids.astype(np.int32), infos([s[:2] for s in segs]))}])
    assert ev.evaluate()["panoptic_seg"]["PQ"] == 100.0
    with pytest.raises(KeyError):
        ev.process([{"segments_info": []}], [{"panoptic_seg": (ids, [])}])


def test_coco_panoptic_evaluator_and_build_evaluator_from_metadata():
    import model.evaluation as ME
    from uenc import evaluation as E
    from uenc.config import add_common_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    from uenc.data import MetadataCatalog
    from uenc.datasets import register_all_cityscapes_panoptic
    register_all_cityscapes_panoptic("datasets")
    name = "cityscapes_fine_panoptic_val"
    ev = E.COCOPanopticEvaluator(name, None)
    assert isinstance(ev, E.PanopticEvaluator) and ME.COCOPanopticEvaluator is E.COCOPanopticEvaluator and ME.PanopticEvaluator is E.PanopticEvaluator
    assert ev._things == list(range(11, 19)) and ev._K == 19 and ev._accumulate == "host"
    with pytest.raises(ValueError):
        E.COCOPanopticEvaluator("a_dataset_nobody_registered")
    with pytest.raises(ValueError):
        E.PanopticEvaluator([1], 2, accumulate="gpu")

    cfg = get_cfg()
    add_common_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list(["MODEL.TEST.PANOPTIC_ON", True, "MODEL.TEST.SEMANTIC_ON", False])
    built = E.build_evaluator(cfg, name)
    assert type(built) is E.COCOPanopticEvaluator and built._accumulate == "device"
    cfg.merge_from_list(["MODEL.TEST.SEMANTIC_ON", True])               # its scorer is cityscapesscripts: the name keeps raising
    with pytest.raises(NotImplementedError, match="cityscapesscripts"):
        E.build_evaluator(cfg, name)
    MetadataCatalog.get("evaluators_cpu_sem_seg").set(evaluator_type="sem_seg", stuff_classes=[str(k) for k in range(6)], ignore_label=254)
    sem = ME.build_evaluator(cfg, "evaluators_cpu_sem_seg", accumulate="host")
    assert type(sem) is E.SemSegEvaluator and (sem._num_classes, sem._ignore_label, sem._accumulate) == (6, 254, "host")
    MetadataCatalog.get("evaluators_cpu_other").set(evaluator_type="something_else")
    with pytest.raises(NotImplementedError, match="no Evaluator"):
        E.build_evaluator(cfg, "evaluators_cpu_other")


def test_semseg_default_path_is_what_it_was():
    """The (N + 1) x (N + 1) matrix and the four figures of a fixed input, as the evaluator produced them before `accumulate` existed."""
    from uenc.evaluation import SemSegEvaluator
    g = torch.Generator().manual_seed(3)
    ev = SemSegEvaluator(4, ignore_label=9)
    assert ev._accumulate == "host"
    for _ in range(2):
        scores = torch.randint(0, 3, (4, 6, 10), generator=g).float()                     # small integers: many ties
        gt = torch.randint(0, 5, (6, 10), generator=g).numpy()
        gt[gt == 4] = 9
        ev.process([{"sem_seg_gt": gt}], [{"sem_seg": scores}])
    assert ev._conf.dtype == np.int64 and ev._conf.tolist() == _SEMSEG_CONF
    res = ev.evaluate()["sem_seg"]
    assert {k: v.hex() for k, v in res.items()} == _SEMSEG_HEX


def test_device_accumulation_refuses_host_tensors():
    from uenc.evaluation import PanopticEvaluator, SemSegEvaluator
    gt = np.zeros((4, 4), dtype=np.int32)
    with pytest.raises(ValueError, match="GPU tensor"):
        SemSegEvaluator(3, accumulate="device").process([{"sem_seg_gt": gt}], [{"sem_seg": torch.zeros(3, 4, 4)}])
    with pytest.raises(ValueError, match="GPU tensor"):
        PanopticEvaluator([1], 2, accumulate="device").process([{"pan_seg": gt, "segments_info": []}], [{"panoptic_seg": (torch.zeros(4, 4, dtype=torch.int32), [])}])
    with pytest.raises(ValueError):
        SemSegEvaluator(3, accumulate="both")


# recorded from the evaluator of the commit before `accumulate` was added
_SEMSEG_CONF = [[11, 15, 9, 12, 7], [8, 11, 5, 5, 7], [7, 4, 4, 3, 2], [2, 2, 1, 3, 2], [0, 0, 0, 0, 0]]
_SEMSEG_HEX = {"mIoU": "0x1.f02f197d3abc5p+3", "fwIoU": "0x1.04b3f7919cb1dp+4", "mACC": "0x1.af06fce74febep+4", "pACC": "0x1.c6e6e6e6e6e6ep+4"}
