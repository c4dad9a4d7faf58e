"""The evaluation loop around the hot path: reference model/evaluation/evaluator.py:16-99 (DatasetEvaluator,
DatasetEvaluators), :107-213 (`inference_on_dataset`: the timed `outputs = model(inputs)` loop of §3.1) and :216-229
(inference_context).  Same protocol and log lines (the "Total inference time ... s / iter per device" line is parsed by grep
upstream).  Evaluators: `SemSegEvaluator` (confusion-matrix mIoU / pixel accuracy as detectron2.evaluation.SemSegEvaluator reports
them [not in reference]) and the two depth evaluators of the "sequence" branch, whose arithmetic is plain numpy in the reference:
`KITTIDepthEvaluator` (kitti_evaluation.py:71-279: velodyne ground truth, Eigen crop, median scaling, the seven depth metrics of
`compute_errors` :282-299) and `CityscapesDepthEvaluator` (cityscapes_evaluation.py:231-362).  The reference's Cityscapes instance /
semantic and COCO instance evaluators wrap third-party scorers (cityscapesscripts, pycocotools) that are not installable here: their
names resolve and raise when constructed.  `inference_on_dataset`, `compute_errors`, the KITTI depth-map projection and the KITTI
evaluation are pinned by fixtures generated from the reference's own functions (oracle/make_data_eval_golden.py ->
tests/golden/data_eval.npz, tests/test_data_eval_cpu.py).

The two segmentation evaluators of the reference's driver (train_net.py:94-108) score here without a third-party package and, with
accumulate="device", without leaving the GPU until `evaluate()` (csrc/evalstats.hip): `SemSegEvaluator` and `PanopticEvaluator` /
`COCOPanopticEvaluator`; `build_evaluator` picks them as the reference's Trainer does.  Everything they count is an integer, so the
host and the device paths agree exactly.  The two depth evaluators take accumulate="device" as well (csrc/ext/depth_eval.hip): they score
every image where the model left its disparity and keep one row of doubles per image on the device; their two paths agree to about 1e-5
relative (the prediction is rounded to fp32 on either path, differently), not bit for bit.

Panoptic quality: the rules of panopticapi's `pq_compute_single_core` and `PQStat.pq_average`, which `pq_match_host`,
uenc_eval_pq_match and `PanopticEvaluator.evaluate` implement literally.  Per image, inter[g, p] = the pixels that have ground-truth id g
and predicted id p; id 0 is VOID on both sides; an id that its side's segments_info does not list is "unknown", kept apart from VOID.
  * Areas are row and column sums of inter: a predicted segment's area includes its pixels over VOID and over unknown ground truth.
  * Candidate pairs have inter > 0 with a listed segment on both sides.  A pair is skipped if the ground truth is a crowd, and if the
    categories differ.  union = area_pred + area_gt - inter - inter[VOID, pred]; if inter / union > 0.5 (decided as 2 inter > union)
    the pair is a TP of its category, both segments are matched and the IoU is added.  Such a match is unique.
  * FN: every unmatched, non-crowd listed ground-truth segment with area > 0 adds to fn[category].
  * FP: for every unmatched predicted segment, v = inter[VOID, pred] + the sum of inter[g, pred] over crowds g of its category; it is
    skipped if v / area_pred > 0.5 (strictly), else it adds to fp[category].
  * Per category with tp + fp + fn > 0: PQ = iou / (tp + fp / 2 + fn / 2), SQ = iou / tp (0 when tp == 0), RQ = tp / (tp + fp / 2 +
    fn / 2); All / Things / Stuff are the means over the categories counted; with none counted the result is 0.
  * Pixels of an unknown predicted id are an error (panopticapi raises as well): `evaluate()` raises.
"""
import datetime
import logging
import os
import time
from collections import OrderedDict
from contextlib import ExitStack, contextmanager
from typing import List, Optional, Union

import numpy as np
import torch
from torch import nn


class DatasetEvaluator:
    """evaluator.py:16-63: reset / process(inputs, outputs) / evaluate() -> dict."""

    def reset(self):
        pass

    def process(self, inputs, outputs):
        pass

    def evaluate(self):
        pass


class DatasetEvaluators(DatasetEvaluator):
    """evaluator.py:66-99: dispatches to several evaluators; result keys must not collide."""

    def __init__(self, evaluators):
        super().__init__()
        self._evaluators = evaluators

    def reset(self):
        for e in self._evaluators:
            e.reset()

    def process(self, inputs, outputs):
        for e in self._evaluators:
            e.process(inputs, outputs)

    def evaluate(self):
        results = OrderedDict()
        for e in self._evaluators:
            r = e.evaluate()
            if _is_main_process() and r is not None:
                for k, v in r.items():
                    assert k not in results, "Different evaluators produce results with the same key {}".format(k)
                    results[k] = v
        return results


def _world_size() -> int:
    import torch.distributed as dist
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _is_main_process() -> bool:
    import torch.distributed as dist
    return (not (dist.is_available() and dist.is_initialized())) or dist.get_rank() == 0


@contextmanager
def inference_context(model):
    """evaluator.py:216-229: eval mode inside, previous mode restored."""
    training_mode = model.training
    model.eval()
    yield
    model.train(training_mode)


def inference_on_dataset(model, data_loader, evaluator: Union[DatasetEvaluator, List[DatasetEvaluator], None], stats: Optional[dict] = None):
    """evaluator.py:107-213.  Runs `model` over `data_loader` under no_grad / eval mode, feeds the evaluator, times data loading,
    compute (synchronised) and evaluation per iteration after min(5, total - 1) warm-up iterations, logs the reference's lines and
    returns `evaluator.evaluate()` ({} when that is None).  `stats`, if given, receives the per-iteration seconds."""
    logger = logging.getLogger(__name__)
    num_devices = _world_size()
    total = len(data_loader)
    logger.info("Start inference on {} batches".format(total))
    if evaluator is None:
        evaluator = DatasetEvaluators([])
    if isinstance(evaluator, (list, tuple)):
        evaluator = DatasetEvaluators(list(evaluator))
    evaluator.reset()
    num_warmup = min(5, total - 1)
    start_time = time.perf_counter()
    total_data_time = total_compute_time = total_eval_time = 0.0
    last_log = 0.0
    with ExitStack() as stack:
        if isinstance(model, nn.Module):
            stack.enter_context(inference_context(model))
        stack.enter_context(torch.no_grad())
        start_data_time = time.perf_counter()
        for idx, inputs in enumerate(data_loader):
            total_data_time += time.perf_counter() - start_data_time
            if idx == num_warmup:
                start_time = time.perf_counter()
                total_data_time = total_compute_time = total_eval_time = 0.0
            start_compute_time = time.perf_counter()
            outputs = model(inputs)
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            total_compute_time += time.perf_counter() - start_compute_time
            start_eval_time = time.perf_counter()
            evaluator.process(inputs, outputs)
            total_eval_time += time.perf_counter() - start_eval_time
            iters_after_start = idx + 1 - num_warmup * int(idx >= num_warmup)
            total_seconds_per_iter = (time.perf_counter() - start_time) / iters_after_start
            if (idx >= num_warmup * 2 or total_compute_time / iters_after_start > 5) and time.perf_counter() - last_log > 5:
                last_log = time.perf_counter()
                eta = datetime.timedelta(seconds=int(total_seconds_per_iter * (total - idx - 1)))
                logger.info(f"Inference done {idx + 1}/{total}. Dataloading: {total_data_time / iters_after_start:.4f} s/iter. "
                            f"Inference: {total_compute_time / iters_after_start:.4f} s/iter. Eval: {total_eval_time / iters_after_start:.4f} s/iter. "
                            f"Total: {total_seconds_per_iter:.4f} s/iter. ETA={eta}")
            start_data_time = time.perf_counter()
    total_time = time.perf_counter() - start_time
    n = max(total - num_warmup, 1)
    # NOTE this format is parsed by grep
    logger.info("Total inference time: {} ({:.6f} s / iter per device, on {} devices)".format(
        str(datetime.timedelta(seconds=total_time)), total_time / n, num_devices))
    logger.info("Total inference pure compute time: {} ({:.6f} s / iter per device, on {} devices)".format(
        str(datetime.timedelta(seconds=int(total_compute_time))), total_compute_time / n, num_devices))
    if stats is not None:
        stats.update(total_s_per_iter=total_time / n, compute_s_per_iter=total_compute_time / n, data_s_per_iter=total_data_time / n,
                     eval_s_per_iter=total_eval_time / n, iterations=n, warmup=num_warmup)
    results = evaluator.evaluate()
    return {} if results is None else results


def _check_accumulate(accumulate: str) -> str:
    if accumulate not in ("host", "device"):
        raise ValueError(f'accumulate must be "host" or "device", got {accumulate!r}')
    return accumulate


def _device_map(a, device, what: str) -> torch.Tensor:
    """An (H, W) integer map as a contiguous int32 tensor on `device`: an upload for host data, no copy for a device int32 tensor."""
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a), dtype=np.int32))
    if t.dim() != 2:
        raise ValueError(f"{what} must be an (H, W) map, got {tuple(t.shape)}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def _need_device(t, what: str):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f'accumulate="device" counts on the GPU where the model left {what}: it must be a GPU tensor '
                         f'(got {"a " + str(t.device) + " tensor" if torch.is_tensor(t) else type(t).__name__}); use accumulate="host" for host data')


class _SizeCache(dict):
    """(H, W, device) -> the (1, 2) int32 size row the kernels take, uploaded once per size."""

    def __missing__(self, key):
        h, w, device = key
        self[key] = torch.tensor([[h, w]], dtype=torch.int32).to(device)
        return self[key]


class SemSegEvaluator(DatasetEvaluator):
    """mIoU / fwIoU / mACC / pACC of the "sem_seg" outputs against "sem_seg" ground-truth maps held by the dataset dicts (key
    `gt_key`, an (H, W) integer array or tensor), accumulated as an (N+1) x (N+1) confusion matrix like
    detectron2.evaluation.SemSegEvaluator; single process (the sharded multi-rank gather is Detectron2 plumbing).
    accumulate="host": argmax on the device, the label map copied to the host and counted with numpy.  accumulate="device": the class
    argmax and the counting happen in uenc_eval_confusion on the (C, H, W) scores where they are; `process` uploads the ground truth
    (or takes a device tensor), copies nothing back and does not synchronise; the matrix is read once, in `evaluate`."""

    def __init__(self, num_classes: int, ignore_label: int = 255, gt_key: str = "sem_seg_gt", accumulate: str = "host"):
        self._num_classes, self._ignore_label, self._gt_key = num_classes, ignore_label, gt_key
        self._accumulate = _check_accumulate(accumulate)
        self._sizes = _SizeCache()
        self.reset()

    def reset(self):
        self._conf = np.zeros((self._num_classes + 1, self._num_classes + 1), dtype=np.int64)
        self._dev_conf = None                         # allocated on the device of the first prediction

    def _process_device(self, inputs, outputs):
        from . import kernels as K
        for inp, out in zip(inputs, outputs):
            scores = out["sem_seg"]
            _need_device(scores, 'out["sem_seg"]')
            if scores.dim() != 3:
                raise ValueError(f'out["sem_seg"] must be (C, H, W), got {tuple(scores.shape)}')
            gt = _device_map(inp[self._gt_key], scores.device, self._gt_key)
            if tuple(gt.shape) != tuple(scores.shape[1:]):
                raise ValueError(f"prediction {tuple(scores.shape[1:])} and ground truth {tuple(gt.shape)} differ in size")
            if self._dev_conf is None:
                self._dev_conf = torch.zeros(self._conf.shape, dtype=torch.int64, device=scores.device)
            H, W = gt.shape
            K.eval_confusion(scores.float().contiguous()[None], gt[None], self._sizes[(H, W, scores.device)], self._dev_conf, self._ignore_label)

    def process(self, inputs, outputs):
        if self._accumulate == "device":
            return self._process_device(inputs, outputs)
        for inp, out in zip(inputs, outputs):
            pred = out["sem_seg"].argmax(dim=0).to("cpu").numpy().astype(np.int64)
            gt = np.asarray(inp[self._gt_key]).astype(np.int64)
            gt[gt == self._ignore_label] = self._num_classes
            self._conf += np.bincount((self._num_classes + 1) * pred.reshape(-1) + gt.reshape(-1),
                                      minlength=self._conf.size).reshape(self._conf.shape)

    def evaluate(self):
        N = self._num_classes
        if self._dev_conf is not None:                # the one read-back
            self._conf = self._conf + self._dev_conf.cpu().numpy()
            self._dev_conf = None
        tp = self._conf.diagonal()[:-1].astype(np.float64)
        pos_gt = np.sum(self._conf[:-1, :-1], axis=0).astype(np.float64)
        pos_pred = np.sum(self._conf[:-1, :-1], axis=1).astype(np.float64)
        class_weights = pos_gt / max(np.sum(pos_gt), 1.0)
        acc_valid = pos_gt > 0
        acc = np.where(acc_valid, tp / np.maximum(pos_gt, 1.0), np.nan)
        union = pos_gt + pos_pred - tp
        iou_valid = acc_valid & (union > 0)
        iou = np.where(iou_valid, tp / np.maximum(union, 1.0), np.nan)
        res = {"mIoU": 100 * float(np.nansum(iou) / max(np.sum(iou_valid), 1)), "fwIoU": 100 * float(np.nansum(iou * class_weights)),
               "mACC": 100 * float(np.nansum(acc) / max(np.sum(acc_valid), 1)), "pACC": 100 * float(np.sum(tp) / max(np.sum(pos_gt), 1.0))}
        return OrderedDict({"sem_seg": res})


# ---------------------------------------------------------------------------------------------------------------------
# panoptic quality (the rules are stated in the module docstring)
# ---------------------------------------------------------------------------------------------------------------------
PQ_MAX_SEGMENTS = 256          # per image and side on the device path: the rows of the kernels' id table


def rgb2id(color):
    """panopticapi.utils.rgb2id: an (H, W, 3) uint8 panoptic PNG -> the (H, W) id map R + 256 G + 65536 B (or one colour -> one id)."""
    color = np.asarray(color)
    if color.ndim == 3:
        color = color.astype(np.int32)
        return color[:, :, 0] + 256 * color[:, :, 1] + 256 * 256 * color[:, :, 2]
    return int(color[0]) + 256 * int(color[1]) + 256 * 256 * int(color[2])


def pq_intersect_host(pred: np.ndarray, gt: np.ndarray, gt_ids, pred_ids) -> np.ndarray:
    """inter (n_gt + 2, n_pred + 2) int64 of two (H, W) id maps: row / column 0 = id 0 (VOID), 1 + k = the k-th listed id (of two equal
    ids the first; an id <= 0 lists nothing), n + 1 = an id that is not listed.  What uenc_eval_pq_intersect counts, with numpy."""
    def rows(m, ids):
        first = {}
        for k, i in enumerate(ids):
            if i > 0:
                first.setdefault(int(i), k + 1)
        values, inverse = np.unique(m, return_inverse=True)
        row = np.array([0 if v == 0 else first.get(int(v), len(ids) + 1) for v in values], dtype=np.int64)
        return row[inverse.reshape(-1)]
    if pred.shape != gt.shape:
        raise ValueError(f"prediction {pred.shape} and ground truth {gt.shape} differ in size")
    R, C = len(gt_ids) + 2, len(pred_ids) + 2
    return np.bincount(rows(gt, gt_ids) * C + rows(pred, pred_ids), minlength=R * C).reshape(R, C)


def pq_match_host(inter: np.ndarray, gt_cat, gt_crowd, pred_cat, num_categories: int):
    """The matching rules on one image's intersection matrix -> rec (n_gt, 4) int64 = matched predicted row or -1, inter, union, category
    per ground-truth row; fp (K), fn (K) int64; the pixel count of unlisted predicted ids.  What uenc_eval_pq_match computes."""
    ng, npd = len(gt_cat), len(pred_cat)
    area_g, area_p = inter.sum(axis=1), inter.sum(axis=0)
    rec = np.zeros((ng, 4), dtype=np.int64)
    rec[:, 0], rec[:, 3] = -1, gt_cat
    fp, fn = np.zeros(num_categories, dtype=np.int64), np.zeros(num_categories, dtype=np.int64)
    hit, crowd = np.zeros(npd, dtype=bool), np.zeros(npd, dtype=np.int64)
    for g, p in zip(*np.nonzero(inter[1:ng + 1, 1:npd + 1])):
        v = int(inter[g + 1, p + 1])
        if gt_cat[g] != pred_cat[p]:
            continue
        if gt_crowd[g]:
            crowd[p] += v
            continue
        union = int(area_p[p + 1]) + int(area_g[g + 1]) - v - int(inter[0, p + 1])
        if 2 * v > union:                                               # IoU > 0.5, exactly
            rec[g, :3] = (p, v, union)
            hit[p] = True
    for g in range(ng):
        if rec[g, 0] < 0 and not gt_crowd[g] and area_g[g + 1] > 0:
            fn[gt_cat[g]] += 1
    for p in range(npd):
        if not hit[p] and not 2 * (int(inter[0, p + 1]) + int(crowd[p])) > int(area_p[p + 1]):
            fp[pred_cat[p]] += 1
    return rec, fp, fn, int(area_p[npd + 1])


class PanopticEvaluator(DatasetEvaluator):
    """PQ / SQ / RQ (all, things, stuff) of the "panoptic_seg" outputs = (id map, segments_info), as `panoptic_inference_fused` returns
    them, against the dataset dicts' panoptic annotation: `dict[gt_key]`, an (H, W) id map, with `dict["segments_info"]` (id, category_id,
    iscrowd: the keys the training forward reads), else `pan_seg_file_name`, a panoptic PNG.  Category ids on both sides are the
    contiguous ones, 0 <= id < num_categories; `thing_ids` splits them into things and stuff.
    accumulate="host": numpy, any number of segments.  accumulate="device": uenc_eval_pq_intersect + uenc_eval_pq_match on the maps where
    they are (the ground truth is uploaded, or taken as a device tensor), at most 256 segments per image and side; `process` copies
    nothing back, the per-image records stay on the device until `evaluate` gathers them in one copy.  Both paths sum the IoUs of the
    matched pairs with the same host code, in float64, in image order then row order: they return equal floats."""

    def __init__(self, thing_ids, num_categories: int, accumulate: str = "host", gt_key: str = "pan_seg"):
        self._things = sorted({int(t) for t in thing_ids})
        self._K, self._gt_key = int(num_categories), gt_key
        self._accumulate = _check_accumulate(accumulate)
        if not self._K >= 1 or any(not 0 <= t < self._K for t in self._things):
            raise ValueError(f"thing_ids {self._things} must lie in [0, num_categories = {num_categories})")
        self._logger = logging.getLogger(__name__)
        self.reset()

    def reset(self):
        self._records = []            # host: (rec, fp, fn, unknown) per image; device: (the match kernel's buffer, n_gt)

    def _ground_truth(self, inp):
        if self._gt_key in inp:
            pan = inp[self._gt_key]
        elif "pan_seg_file_name" in inp:
            from PIL import Image
            with Image.open(inp["pan_seg_file_name"]) as im:
                pan = rgb2id(np.asarray(im.convert("RGB")))
        else:
            raise KeyError(f'a dataset dict needs "{self._gt_key}" (an id map) or "pan_seg_file_name" for the panoptic evaluation')
        return pan, [(int(s["id"]), self._category(s), int(s.get("iscrowd", 0))) for s in inp["segments_info"]]

    def _category(self, seg) -> int:
        c = int(seg["category_id"])
        if not 0 <= c < self._K:
            raise ValueError(f"segment {seg.get('id')} has category {c}, outside [0, {self._K})")
        return c

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            pred, info = out["panoptic_seg"]
            pan, gt_segs = self._ground_truth(inp)
            pred_segs = [(int(s["id"]), self._category(s)) for s in info]
            if self._accumulate == "device":
                self._records.append(self._process_device(pred, pred_segs, pan, gt_segs))
                continue
            pred = pred.cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
            pan = pan.cpu().numpy() if torch.is_tensor(pan) else np.asarray(pan)
            inter = pq_intersect_host(pred, pan, [i for i, _, _ in gt_segs], [i for i, _ in pred_segs])
            self._records.append(pq_match_host(inter, [c for _, c, _ in gt_segs], [k for _, _, k in gt_segs], [c for _, c in pred_segs], self._K))

    def _process_device(self, pred, pred_segs, pan, gt_segs):
        from . import kernels as K
        _need_device(pred, 'the id map of out["panoptic_seg"]')
        S, ng, npd = PQ_MAX_SEGMENTS, len(gt_segs), len(pred_segs)
        if ng > S or npd > S:
            raise ValueError(f'accumulate="device" takes at most {S} segments per image on either side (the kernels\' id table); this image has '
                             f'{ng} ground-truth and {npd} predicted segments: use accumulate="host"')
        pred = _device_map(pred, pred.device, "the predicted id map")
        gt = _device_map(pan, pred.device, "the ground-truth id map")
        if gt.shape != pred.shape:
            raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} differ in size")
        table = np.zeros(5 * S + 4, dtype=np.int32)                       # K._eval_pq_table with B = 1: one upload
        if ng:
            table[0:ng], table[2 * S:2 * S + ng], table[3 * S:3 * S + ng] = np.asarray(gt_segs, dtype=np.int64).T
        if npd:
            table[S:S + npd], table[4 * S:4 * S + npd] = np.asarray(pred_segs, dtype=np.int64).T
        table[5 * S:] = (ng, npd) + tuple(gt.shape)
        table = torch.from_numpy(table).to(pred.device)
        inter = K.eval_pq_intersect(pred[None], gt[None], table)
        return K.eval_pq_match(inter, table, self._K), ng

    def _gathered(self):
        """Every image's (rec (n_gt, 4), fp, fn, unknown) as int64 numpy, in image order: for the device path its one device-to-host copy."""
        records = self._records
        if self._accumulate == "device" and records:
            from . import kernels as K
            host = torch.stack([r for r, _ in records]).cpu().numpy().astype(np.int64)
            records = []
            for row, (_, ng) in zip(host, self._records):
                rec, fp, fn, unknown = K.eval_pq_unpack(row, 1, self._K)
                records.append((rec[0, :ng], fp[0], fn[0], int(unknown[0])))
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            box = [None] * dist.get_world_size()
            dist.all_gather_object(box, records)
            records = [r for part in box for r in part]
        return records

    def evaluate(self):
        records = self._gathered()
        if not _is_main_process():
            return None
        K = self._K
        unknown = [(i, r[3]) for i, r in enumerate(records) if r[3]]
        if unknown:
            raise ValueError(f"{len(unknown)} image(s) have pixels of a predicted id that their segments_info does not list "
                             f"(first: image {unknown[0][0]}, {unknown[0][1]} pixels)")
        iou, tp = np.zeros(K, dtype=np.float64), np.zeros(K, dtype=np.int64)
        fp, fn = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        for rec, img_fp, img_fn, _ in records:
            for col, inter, union, cat in rec.tolist():
                if col >= 0:
                    tp[cat] += 1
                    iou[cat] += inter / union
            fp += img_fp
            fn += img_fn
        res = {}
        for name, cats in (("", range(K)), ("_th", self._things), ("_st", [c for c in range(K) if c not in set(self._things)])):
            pq = sq = rq = 0.0
            n = 0
            for c in cats:
                t, p, f = int(tp[c]), int(fp[c]), int(fn[c])
                if t + p + f == 0:
                    continue                                              # a category never seen is not part of the mean
                n += 1
                pq += float(iou[c]) / (t + 0.5 * p + 0.5 * f)
                sq += float(iou[c]) / t if t else 0.0
                rq += t / (t + 0.5 * p + 0.5 * f)
            for key, v in (("PQ", pq), ("SQ", sq), ("RQ", rq)):
                res[key + name] = 100 * v / n if n else 0.0
        self._stats = {"tp": tp, "fp": fp, "fn": fn, "iou": iou}
        return OrderedDict({"panoptic_seg": res})


class COCOPanopticEvaluator(PanopticEvaluator):
    """detectron2.evaluation.COCOPanopticEvaluator's place in the reference's train_net.py:100-108, scored by `PanopticEvaluator` instead
    of panopticapi: thing ids and the number of categories come from the dataset's metadata (the contiguous train ids that
    `thing_dataset_id_to_contiguous_id` / `stuff_dataset_id_to_contiguous_id` map to, as uenc.datasets registers them and as
    the dataset dicts and the predictions carry them).  Nothing is written to `output_dir`."""

    def __init__(self, dataset_name: str, output_dir: Optional[str] = None, accumulate: str = "host", gt_key: str = "pan_seg"):
        from .data import MetadataCatalog
        meta = MetadataCatalog.get(dataset_name)
        things = getattr(meta, "thing_dataset_id_to_contiguous_id", None)
        stuff = getattr(meta, "stuff_dataset_id_to_contiguous_id", None)
        if things is None or stuff is None:
            raise ValueError(f"dataset {dataset_name!r} has no thing / stuff_dataset_id_to_contiguous_id metadata: is it a registered panoptic dataset?")
        cats = set(things.values()) | set(stuff.values())
        self._dataset_name, self._output_dir = dataset_name, output_dir
        super().__init__(sorted(set(things.values())), max(cats) + 1, accumulate=accumulate, gt_key=gt_key)


# ---------------------------------------------------------------------------------------------------------------------
# depth metrics of the "sequence" branch
# ---------------------------------------------------------------------------------------------------------------------
def compute_errors(gt: np.ndarray, pred: np.ndarray):
    """cityscapes_evaluation.py:365-383 = kitti_evaluation.py:282-299: (abs_rel, sq_rel, rmse, rmse_log, a1, a2, a3) of predicted
    against ground-truth depths (1-D arrays of valid pixels, same dtype arithmetic as numpy gives the inputs)."""
    ratio = np.maximum(gt / pred, pred / gt)
    a1, a2, a3 = ((ratio < 1.25 ** k).mean() for k in (1, 2, 3))
    diff = gt - pred
    rmse = np.sqrt((diff ** 2).mean())
    rmse_log = np.sqrt(((np.log(gt) - np.log(pred)) ** 2).mean())
    return np.mean(np.abs(diff) / gt), np.mean(diff ** 2 / gt), rmse, rmse_log, a1, a2, a3


def disp_to_depth(disp, min_depth=0.1, max_depth=100.0):
    """monodepth_loss.py:103-112: sigmoid disparity -> (scaled disparity, depth)."""
    min_disp, max_disp = 1 / max_depth, 1 / min_depth
    scaled = min_disp + (max_disp - min_disp) * disp
    return scaled, 1 / scaled


def _resize_bilinear(a: np.ndarray, width: int, height: int) -> np.ndarray:
    """cv2.resize(a, (width, height)) with its default INTER_LINEAR [cv2 is not in the reference tree]: bilinear taps at half-pixel
    centres, clamped at the borders, no antialiasing = F.interpolate(..., mode="bilinear", align_corners=False)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))[None, None]
    return torch.nn.functional.interpolate(t, size=(height, width), mode="bilinear", align_corners=False)[0, 0].numpy()


_DEPTH_KEYS = ("abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3")


class _DepthEvaluator(DatasetEvaluator):
    """Shared protocol of the two depth evaluators: process() collects (ground-truth depth map, prediction) pairs, evaluate() scores
    every image after median scaling and averages the seven metrics over images -> {"depth_error": {...}} on the main process.
    (The reference parks the pairs as .npy files in a temporary directory shared by the ranks of one machine; here they stay in
    memory and are gathered.)
    accumulate="device": process() scores every image where the model left its disparity (csrc/ext/depth_eval.hip: resize + invert,
    valid mask, exact medians, the seven sums), uploads only the ground truth, keeps one row of doubles per image on the device, copies
    nothing back and does not synchronise; evaluate() reads the rows once.  The device path rounds the prediction to fp32 once (the host
    path resizes in fp32 as well, with fp32 weights) and sums in fp64: the two agree to about 1e-5 relative, not bit for bit."""
    MIN_DEPTH = 1e-3
    MAX_DEPTH = 80

    ROW_CHUNK = 256                # rows the device buffer grows by

    def __init__(self, dataset_name=None, accumulate: str = "host"):
        self._dataset_name = dataset_name
        self._accumulate = _check_accumulate(accumulate)
        self._logger = logging.getLogger(__name__)
        self.reset()

    def reset(self):
        self._pairs = []
        self._dev_rows, self._dev_count, self._dev_ws = None, 0, {}       # (capacity, DEPTH_EVAL_ROW) fp64 on the device, rows in use

    def _score_device(self, depth_gt: np.ndarray, disp: torch.Tensor, window):
        """One image on the device: depth_gt (H, W) host fp32 / fp64 (uploaded as it is), disp (h, w) the scaled disparity where the model
        left it, window = (r0, r1, c0, c1) computed by the caller exactly as the host path slices.  Appends one row; copies nothing
        back and does not synchronise (growing the buffer allocates)."""
        from . import kernels as K
        if depth_gt.dtype not in (np.float32, np.float64):
            depth_gt = depth_gt.astype(np.float64)
        gt = torch.from_numpy(np.ascontiguousarray(depth_gt)).to(disp.device)
        H, W = gt.shape
        i = self._dev_count
        if self._dev_rows is None or i >= self._dev_rows.shape[0]:
            grown = torch.zeros((i + self.ROW_CHUNK, K.DEPTH_EVAL_ROW), dtype=torch.float64, device=disp.device)
            if self._dev_rows is not None:
                grown[:i] = self._dev_rows
            self._dev_rows = grown
        r0, r1, c0, c1 = (int(v) for v in window)
        r0, r1, c0, c1 = min(max(r0, 0), H), min(max(r1, 0), H), min(max(c0, 0), W), min(max(c1, 0), W)      # as a slice clamps
        if r0 >= r1 or c0 >= c1:                                            # an empty window scores like an empty valid set
            self._dev_rows[i] = float("nan")
            self._dev_rows[i, 7] = 0.0
        else:
            key = (H, W, disp.device)
            if key not in self._dev_ws:
                self._dev_ws[key] = K.depth_eval_ws(H, W, disp.device)
            pred = K.depth_eval_pred(disp.detach().float().contiguous(), (H, W))
            K.depth_eval_score(gt, pred, (r0, r1, c0, c1), self.MIN_DEPTH, self.MAX_DEPTH, self._dev_rows, i, self._dev_ws[key])
        self._dev_count = i + 1

    def _score(self, depth_gt: np.ndarray, pred: np.ndarray):
        raise NotImplementedError

    def evaluate(self):
        import torch.distributed as dist
        if self._accumulate == "device":
            return self._evaluate_device()
        pairs = self._pairs
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            box = [None] * dist.get_world_size()
            dist.all_gather_object(box, pairs)
            pairs = [p for part in box for p in part]
        if not _is_main_process():
            return None
        rows = [self._score(gt, pred) for gt, pred in pairs]
        means = np.mean(np.asarray(rows, dtype=np.float64), axis=0) if rows else np.full(7, np.nan)
        return OrderedDict(depth_error={k: v for k, v in zip(_DEPTH_KEYS, means)})

    def _evaluate_device(self):
        """The one read-back: the seven metrics of every image; several ranks gather these rows, not maps."""
        import torch.distributed as dist
        rows = np.zeros((0, 7), dtype=np.float64)
        if self._dev_rows is not None and self._dev_count:
            rows = self._dev_rows[:self._dev_count, :7].cpu().numpy()
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            box = [None] * dist.get_world_size()
            dist.all_gather_object(box, rows)
            rows = np.concatenate(box, axis=0)
        if not _is_main_process():
            return None
        means = np.mean(rows, axis=0) if len(rows) else np.full(7, np.nan)
        return OrderedDict(depth_error={k: v for k, v in zip(_DEPTH_KEYS, means)})

    def _scaled_errors(self, depth_gt: np.ndarray, depth_pred: np.ndarray):
        """per-image median scaling, clamp to [MIN_DEPTH, MAX_DEPTH], the seven metrics (both arrays: valid pixels only)."""
        depth_pred = depth_pred * (np.median(depth_gt) / np.median(depth_pred))
        return compute_errors(depth_gt, np.clip(depth_pred, self.MIN_DEPTH, self.MAX_DEPTH))


class KITTIDepthEvaluator(_DepthEvaluator):
    """kitti_evaluation.py:71-279.  Ground truth = the frame's velodyne scan projected into camera 2 (`generate_depth_map`, depth =
    the points' forward distance); prediction = 1 / (bilinear resize of the scaled disparity to the ground-truth size); scored on
    0.001 < gt < 80 inside the Eigen crop."""

    @staticmethod
    def load_velodyne_points(filename):
        pts = np.fromfile(filename, dtype=np.float32).reshape(-1, 4)
        pts[:, 3] = 1.0                                   # homogeneous (the fourth column is reflectance in the file)
        return pts

    @staticmethod
    def read_calib_file(path):
        """KITTI calibration text: `key: v v v ...` -> float arrays where every token is numeric, strings otherwise."""
        numeric = set("0123456789.e+- ")
        data = {}
        with open(path, "r") as f:
            for line in f:
                key, value = line.split(":", 1)
                value = value.strip()
                data[key] = value
                if numeric.issuperset(value):
                    try:
                        data[key] = np.array([float(v) for v in value.split(" ")])
                    except ValueError:
                        pass
        return data

    @classmethod
    def generate_depth_map(cls, calib_dir, velo_filename, cam=2, vel_depth=False):
        """kitti_evaluation.py:109-166: project the scan with P_rect_0<cam> R_rect_00 [R|T]_velo->cam, round to pixels (minus 1, as
        the KITTI matlab code), keep points inside the S_rect_02 image; where several points hit one pixel the closest wins
        (duplicates are found through the reference's own linear index `row * (W - 1) + col - 1`)."""
        cam2cam = cls.read_calib_file(os.path.join(calib_dir, "calib_cam_to_cam.txt"))
        v2c = cls.read_calib_file(os.path.join(calib_dir, "calib_velo_to_cam.txt"))
        velo2cam = np.vstack((np.hstack((v2c["R"].reshape(3, 3), v2c["T"][..., np.newaxis])), np.array([0, 0, 0, 1.0])))
        im_shape = cam2cam["S_rect_02"][::-1].astype(np.int32)
        R_cam2rect = np.eye(4)
        R_cam2rect[:3, :3] = cam2cam["R_rect_00"].reshape(3, 3)
        P_velo2im = np.dot(np.dot(cam2cam["P_rect_0" + str(cam)].reshape(3, 4), R_cam2rect), velo2cam)
        velo = cls.load_velodyne_points(velo_filename)
        velo = velo[velo[:, 0] >= 0, :]                   # in front of the image plane (approximation)
        pts = np.dot(P_velo2im, velo.T).T
        pts[:, :2] = pts[:, :2] / pts[:, 2][..., np.newaxis]
        if vel_depth:
            pts[:, 2] = velo[:, 0]
        pts[:, 0] = np.round(pts[:, 0]) - 1
        pts[:, 1] = np.round(pts[:, 1]) - 1
        inside = (pts[:, 0] >= 0) & (pts[:, 1] >= 0) & (pts[:, 0] < im_shape[1]) & (pts[:, 1] < im_shape[0])
        pts = pts[inside, :]
        depth = np.zeros((im_shape[:2]))
        rows, cols = pts[:, 1].astype(int), pts[:, 0].astype(int)
        depth[rows, cols] = pts[:, 2]
        lin = pts[:, 1] * (depth.shape[1] - 1) + pts[:, 0] - 1
        uniq, inv, counts = np.unique(lin, return_inverse=True, return_counts=True)
        for u in np.nonzero(counts > 1)[0]:
            hit = np.nonzero(inv == u)[0]
            depth[rows[hit[0]], cols[hit[0]]] = pts[hit, 2].min()
        depth[depth < 0] = 0
        return depth

    @staticmethod
    def _eigen_crop(h: int, w: int):
        return np.array([0.40810811 * h, 0.99189189 * h, 0.03594771 * w, 0.96405229 * w]).astype(np.int32)

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            if self._accumulate == "device":
                _need_device(out["disp_results"], 'out["disp_results"]')
            depth_gt = self.generate_depth_map(inp["calib_path"], inp["velo_file"], 2, True)
            disp, _ = disp_to_depth(out["disp_results"])
            if self._accumulate == "device":
                disp = disp.squeeze()
                if disp.dim() != 2:
                    raise ValueError(f'out["disp_results"] must hold one (h, w) map, got {tuple(out["disp_results"].shape)}')
                self._score_device(depth_gt, disp, self._eigen_crop(*depth_gt.shape[:2]))
                continue
            disp = np.asarray(disp.squeeze().detach().float().cpu().numpy())
            self._pairs.append((depth_gt, 1 / _resize_bilinear(disp, depth_gt.shape[1], depth_gt.shape[0])))

    def _score(self, depth_gt, depth_pred):
        h, w = depth_gt.shape[:2]
        mask = np.logical_and(depth_gt > self.MIN_DEPTH, depth_gt < self.MAX_DEPTH)
        crop = self._eigen_crop(h, w)
        inside = np.zeros(mask.shape, dtype=bool)
        inside[crop[0]:crop[1], crop[2]:crop[3]] = True
        mask &= inside
        return self._scaled_errors(depth_gt[mask], depth_pred[mask])


class CityscapesDepthEvaluator(_DepthEvaluator):
    """cityscapes_evaluation.py:231-362.  Ground truth = the .npy depth map stored beside the image (`/leftImg8bit/test/` ->
    `/gt_depths/`); its lower quarter (ego vehicle) is cut, the scaled disparity is resized to the rest and inverted, and the
    window [256:, 192:1856] is scored on 0.001 < gt < 80."""

    def process(self, inputs, outputs):
        for inp, out in zip(inputs, outputs):
            gt_path = inp["file_name"].replace("/leftImg8bit/test/", "/gt_depths/").replace(".png", ".npy")
            if self._accumulate == "device":
                _need_device(out["disp_results"], 'out["disp_results"]')
                disp, _ = disp_to_depth(out["disp_results"])
                depth_gt = np.load(gt_path)                                 # once per call, not per batch element
                h, w = depth_gt.shape[:2]
                h = int(round(h * 0.75))
                for d in disp[:, 0]:
                    self._score_device(depth_gt[:h], d, (256, h, 192, 1856))
                continue
            disp, _ = disp_to_depth(out["disp_results"])
            for d in disp.detach().float().cpu()[:, 0].numpy():
                self._pairs.append((np.load(gt_path), d))

    def _score(self, depth_gt, disp_pred):
        h, w = depth_gt.shape[:2]
        h = int(round(h * 0.75))
        depth_gt = depth_gt[:h]
        depth_pred = 1 / _resize_bilinear(np.squeeze(disp_pred), w, h)
        depth_gt, depth_pred = depth_gt[256:, 192:1856], depth_pred[256:, 192:1856]
        mask = np.logical_and(depth_gt > self.MIN_DEPTH, depth_gt < self.MAX_DEPTH)
        return self._scaled_errors(depth_gt[mask], depth_pred[mask])


def print_csv_format(results):
    """detectron2.evaluation.print_csv_format: copy-pastable metric lines."""
    logger = logging.getLogger(__name__)
    for task, res in results.items():
        if isinstance(res, dict):
            important = [(k, v) for k, v in res.items() if "-" not in k]
            logger.info("copypaste: Task: {}".format(task))
            logger.info("copypaste: " + ",".join([k[0] for k in important]))
            logger.info("copypaste: " + ",".join(["{0:.4f}".format(k[1]) for k in important]))
        else:
            logger.info(f"copypaste: {task}={res}")


def _needs(name: str, dep: str):
    class _Unavailable(DatasetEvaluator):
        __doc__ = f"{name} of the reference wraps `{dep}`, which is not installable in this environment (SURVEY.md §8c)."

        def __init__(self, *a, **k):
            raise NotImplementedError(f"{name} needs the third-party package `{dep}` (out of the hot-path scope, SURVEY.md §8f)")
    _Unavailable.__name__ = _Unavailable.__qualname__ = name
    return _Unavailable


COCOEvaluator = _needs("COCOEvaluator", "pycocotools")
InstanceSegEvaluator = _needs("InstanceSegEvaluator", "pycocotools")
CityscapesInstanceEvaluator = _needs("CityscapesInstanceEvaluator", "cityscapesscripts")
CityscapesSemSegEvaluator = _needs("CityscapesSemSegEvaluator", "cityscapesscripts")


def build_evaluator(cfg, dataset_name: str, accumulate: str = "device", output_folder: Optional[str] = None):
    """The reference's Trainer.build_evaluator (train_net.py:75-149): the evaluator(s) for a dataset by its metadata's `evaluator_type`
    and cfg.MODEL.TEST.  `accumulate` goes to the segmentation evaluators and to both depth evaluators: they count / score on the device
    by default.  The branches whose scorers are third-party packages
    (Cityscapes instance / semantic scripts, COCO instance AP) construct the names that raise."""
    from .data import MetadataCatalog
    meta = MetadataCatalog.get(dataset_name)
    evaluator_type = getattr(meta, "evaluator_type", None)
    if output_folder is None:
        output_folder = os.path.join(cfg.OUTPUT_DIR, "inference")
    test = cfg.MODEL.TEST
    evaluators = []
    if evaluator_type == "kitti_depth" and test.DEPTH_ON:
        evaluators.append(KITTIDepthEvaluator(dataset_name, accumulate=accumulate))
    if evaluator_type in ("sem_seg", "ade20k_panoptic_seg"):
        evaluators.append(SemSegEvaluator(len(meta.stuff_classes), ignore_label=getattr(meta, "ignore_label", 255), accumulate=accumulate))
    if evaluator_type in ("coco_panoptic_seg", "ade20k_panoptic_seg", "cityscapes_panoptic_seg", "mapillary_vistas_panoptic_seg") and test.PANOPTIC_ON:
        evaluators.append(COCOPanopticEvaluator(dataset_name, output_folder, accumulate=accumulate))
    if evaluator_type == "cityscapes_instance":
        return CityscapesInstanceEvaluator(dataset_name)
    if evaluator_type == "cityscapes_sem_seg":
        return CityscapesSemSegEvaluator(dataset_name)
    if evaluator_type == "cityscapes_panoptic_seg":
        if test.SEMANTIC_ON:
            evaluators.append(CityscapesSemSegEvaluator(dataset_name))
        if test.INSTANCE_ON:
            evaluators.append(CityscapesInstanceEvaluator(dataset_name))
    if evaluator_type == "cityscapes_depth" and test.DEPTH_ON:
        evaluators.append(CityscapesDepthEvaluator(dataset_name, accumulate=accumulate))
    if evaluator_type == "ade20k_panoptic_seg" and test.INSTANCE_ON:
        evaluators.append(InstanceSegEvaluator(dataset_name, output_dir=output_folder))
    if not evaluators:
        raise NotImplementedError("no Evaluator for the dataset {} with the type {}".format(dataset_name, evaluator_type))
    return evaluators[0] if len(evaluators) == 1 else DatasetEvaluators(evaluators)
