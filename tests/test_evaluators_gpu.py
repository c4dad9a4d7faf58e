"""SemSegEvaluator and PanopticEvaluator with accumulate="device" return the dicts of their host paths (==, floats included) over a stream
of small synthetic batches, directly and through build_evaluator + inference_on_dataset with a stub model that leaves its outputs on
the GPU."""
import numpy as np
import pytest
import torch

from pq_cases import infos, numpy_pq, random_case

pytestmark = pytest.mark.gpu

H, W, NCLS = 64, 96, 19
THINGS = list(range(11, 19))


def _stream():
    """Four batches of two 64 x 96 images: dataset dicts (host ground truth) and model outputs (GPU tensors).  One image has no
    prediction, one no ground-truth segment."""
    rs = np.random.RandomState(31)
    g = torch.Generator().manual_seed(31)
    gt_ids = [1000 * (11 + k % 8) + k for k in range(12)] + [3, 4, 5, 6]
    batches, images = [], []
    for i in range(8):
        case = random_case(rs, H, W, [] if i == 5 else gt_ids, [] if i == 2 else range(1, 15), NCLS, crowd_every=4, unlisted_gt=0)
        pred, psegs, pan, gsegs = case
        images.append(case)
        sem_gt = rs.randint(0, NCLS, (H, W))
        sem_gt[rs.rand(H, W) < 0.1] = 255
        inp = {"image_id": i, "pan_seg": pan, "segments_info": infos(gsegs), "sem_seg_gt": sem_gt}
        out = {"sem_seg": torch.randint(0, 5, (NCLS, H, W), generator=g).float().cuda(),
               "panoptic_seg": (torch.from_numpy(pred).cuda(), infos(psegs))}
        if i % 2 == 0:
            batches.append(([], []))
        batches[-1][0].append(inp)
        batches[-1][1].append(out)
    return batches, images


@pytest.fixture(scope="module")
def stream():
    return _stream()


def _run(ev, batches, gt_on_device=False):
    ev.reset()
    for inputs, outputs in batches:
        if gt_on_device:
            inputs = [dict(d, pan_seg=torch.from_numpy(d["pan_seg"]).cuda(), sem_seg_gt=torch.from_numpy(d["sem_seg_gt"]).cuda()) for d in inputs]
        ev.process(inputs, outputs)
    return ev.evaluate()


def test_device_semseg_equals_host(stream):
    from uenc.evaluation import SemSegEvaluator
    batches, _ = stream
    host = _run(SemSegEvaluator(NCLS), batches)
    dev = SemSegEvaluator(NCLS, accumulate="device")
    res = _run(dev, batches)
    assert res == host and dev._conf.sum() == 8 * H * W and 0 < res["sem_seg"]["mIoU"] < 100
    assert _run(dev, batches, gt_on_device=True) == host                 # reset() starts over; ground truth already on the GPU


def test_device_panoptic_equals_host(stream):
    from uenc.evaluation import PanopticEvaluator
    batches, images = stream
    host = _run(PanopticEvaluator(THINGS, NCLS), batches)
    assert host["panoptic_seg"] == numpy_pq(images, THINGS, NCLS)[0]
    dev = PanopticEvaluator(THINGS, NCLS, accumulate="device")
    assert _run(dev, batches) == host and _run(dev, batches, gt_on_device=True) == host
    assert 0 < host["panoptic_seg"]["PQ"] < 100 and host["panoptic_seg"]["PQ_th"] > 0 and host["panoptic_seg"]["PQ_st"] > 0


def test_inference_on_dataset_with_built_evaluators(stream):
    from uenc import evaluation as E
    from uenc.config import add_common_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    from uenc.data import MetadataCatalog
    batches, _ = stream
    MetadataCatalog.get("evaluators_gpu_panoptic").set(
        evaluator_type="ade20k_panoptic_seg", stuff_classes=[str(k) for k in range(NCLS)], ignore_label=255,
        thing_dataset_id_to_contiguous_id={100 + k: k for k in THINGS}, stuff_dataset_id_to_contiguous_id={100 + k: k for k in range(11)})
    cfg = get_cfg()
    add_common_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list(["MODEL.TEST.PANOPTIC_ON", True])
    outputs = {d["image_id"]: o for inputs, outs in batches for d, o in zip(inputs, outs)}
    model = lambda inputs: [outputs[d["image_id"]] for d in inputs]
    loader = [inputs for inputs, _ in batches]
    results = {}
    for accumulate in ("device", "host"):
        ev = E.build_evaluator(cfg, "evaluators_gpu_panoptic", accumulate=accumulate)
        assert [type(e) for e in ev._evaluators] == [E.SemSegEvaluator, E.COCOPanopticEvaluator]
        assert all(e._accumulate == accumulate for e in ev._evaluators)
        results[accumulate] = E.inference_on_dataset(model, loader, ev)
    assert list(results["device"]) == ["sem_seg", "panoptic_seg"] and results["device"] == results["host"]


def test_device_panoptic_refuses_more_than_256_segments():
    from uenc.evaluation import PanopticEvaluator
    n = 257
    pan = (np.arange(20 * 20, dtype=np.int32) % n + 1).reshape(20, 20)
    segs = [(i, i % 5, 0) for i in range(1, n + 1)]
    dev = PanopticEvaluator([0, 1], 5, accumulate="device")
    few = (torch.from_numpy(pan).cuda(), infos([(1, 0)]))
    with pytest.raises(ValueError, match="at most 256 segments"):
        dev.process([{"pan_seg": pan, "segments_info": infos(segs)}], [{"panoptic_seg": few}])
    with pytest.raises(ValueError, match="at most 256 segments"):
        dev.process([{"pan_seg": pan, "segments_info": infos(segs[:3])}], [{"panoptic_seg": (few[0], infos([s[:2] for s in segs]))}])
    dev.process([{"pan_seg": pan, "segments_info": infos(segs[:256])}], [{"panoptic_seg": (few[0], infos([s[:2] for s in segs[:256]]))}])
    with pytest.raises(ValueError, match="does not list"):                # id 257 is in the predicted map and in no table row
        dev.evaluate()
