"""KITTIDepthEvaluator and CityscapesDepthEvaluator with accumulate="device" against their own host paths on the same tensors, and
uenc_depth_eval_score against the reference's recorded KITTI result.

Bounds.  Continuous metrics: rtol = 1e-4.  The two paths differ by the fp32 rounding of the prediction (the host resizes with fp32
weights, the device rounds a float64 lerp once): a few times 2^-24 per pixel and in the median ratio, i.e. below 1e-6 relative on each
term; divided by abs_rel, asserted >= 0.05 on the host result, that is about 1e-5: a tenfold margin.  a1..a3: per image
|count_device - count_host| <= the number of valid pixels whose host ratio lies within relative 1e-5 of a threshold (counted here from the
host arrays; test_depth_eval_cases_cpu.py caps it at 0.1 % of the valid pixels for these very cases)."""
import os

import numpy as np
import pytest
import torch

import depth_eval_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _to_cuda(outputs):
    return [{k: v.cuda() for k, v in o.items()} for o in outputs]


def _device_rows(ev):
    return ev._dev_rows[:ev._dev_count].cpu().numpy()


def _compare(cls, inputs, outputs, images):
    host = cls("x", accumulate="host")
    host.process(inputs, outputs)
    dev = cls("x", accumulate="device")
    dev.process(inputs, _to_cuda(outputs))
    assert dev._pairs == [] and dev._dev_count == images == len(host._pairs)
    rows = _device_rows(dev)
    per_image = C.host_rows(host)
    for i, (row, g, p) in enumerate(per_image):
        n = len(g)
        assert row[0] >= 0.05 and rows[i, 7] == n > 0
        print(f"image {i}: n {n}  host {row[:4]}  device {rows[i, :4]}  rel {np.abs(rows[i, :4] - row[:4]) / row[:4]}")
        np.testing.assert_allclose(rows[i, :4], row[:4], rtol=1e-4, atol=0)
        border = C.borderline_count(g, p)
        host_counts = np.round(row[4:7] * n)
        assert np.all(np.abs(rows[i, 10:13] - host_counts) <= border), (i, rows[i, 10:13], host_counts, border)
    want, got = host.evaluate()["depth_error"], dev.evaluate()["depth_error"]
    assert list(got) == list(want) == ["abs_rel", "sq_rel", "rmse", "rmse_log", "a1", "a2", "a3"]
    np.testing.assert_array_equal([got[k] for k in got], np.mean(rows[:, :7], axis=0))
    np.testing.assert_allclose([got[k] for k in got][:4], [want[k] for k in want][:4], rtol=1e-4, atol=0)
    return dev


def test_kitti_device_against_host(tmp_path):
    """On the parent this fails at once: KITTIDepthEvaluator() takes no `accumulate`."""
    from uenc.evaluation import KITTIDepthEvaluator
    inputs, outputs = C.kitti_case(tmp_path)
    _compare(KITTIDepthEvaluator, inputs, outputs, 3)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_cityscapes_device_against_host(tmp_path, dtype):
    from uenc.evaluation import CityscapesDepthEvaluator
    inputs, outputs = C.cityscapes_case(tmp_path, dtype)
    dev = _compare(CityscapesDepthEvaluator, inputs, outputs, 2)
    assert np.all(_device_rows(dev)[:, 7] <= 8 * 1664)


def test_score_against_the_references_number():
    """depth_pairs() through uenc_depth_eval_score with the KITTI window, predictions rounded to fp32 (the kernel's input format),
    against kitti_depth_error of tests/golden/data_eval.npz, which the reference computed from the float64 predictions.  The shift
    the rounding alone causes is computed on the CPU with the restatement and asserted to be inside the bound."""
    from oracle.data_eval_inputs import depth_pairs
    from uenc import kernels as K
    from uenc.evaluation import KITTIDepthEvaluator
    golden = np.load(os.path.join(ROOT, "tests", "golden", "data_eval.npz"))["kitti_depth_error"]
    pairs = depth_pairs()
    rows = torch.zeros((len(pairs), K.DEPTH_EVAL_ROW), dtype=torch.float64, device="cuda")
    cpu32 = []
    for i, (gt, pred) in enumerate(pairs):
        win = C.kitti_window(*gt.shape)
        p32 = pred.astype(np.float32)
        K.depth_eval_score(torch.from_numpy(gt).cuda(), torch.from_numpy(p32).cuda(), win, C.MIN_DEPTH, C.MAX_DEPTH, rows, i)
        cpu32.append(C.score_f64(gt, p32, win)["row"])
    rows = rows.cpu().numpy()
    shift = np.abs(np.mean(cpu32, axis=0)[:4] - golden[:4]) / golden[:4]
    print("rounding shift", shift, " device", np.mean(rows[:, :7], axis=0), " reference", golden)
    assert np.all(shift < 1e-4)
    np.testing.assert_allclose(np.mean(rows[:, :4], axis=0), golden[:4], rtol=1e-4, atol=0)
    host = KITTIDepthEvaluator("x")
    host._pairs = list(pairs)
    for i, (row, g, p) in enumerate(C.host_rows(host)):
        assert rows[i, 7] == len(g)
        assert np.all(np.abs(rows[i, 10:13] - np.round(row[4:7] * len(g))) <= C.borderline_count(g, p)), i


def test_process_keeps_nothing_and_does_not_synchronise(tmp_path, monkeypatch):
    from uenc.evaluation import KITTIDepthEvaluator
    inputs, outputs = C.kitti_case(tmp_path)
    outputs = _to_cuda(outputs)
    ev = KITTIDepthEvaluator("x", accumulate="device")
    ev.process(inputs[:1], outputs[:1])                                   # first call: allocates the row buffer and the workspace
    torch.cuda.synchronize()
    calls = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: calls.append("synchronize"))
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: calls.append("cpu") or self)
    monkeypatch.setattr(torch.Tensor, "item", lambda self: calls.append("item") or 0)
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: calls.append("tolist") or [])
    monkeypatch.setattr(torch.Tensor, "numpy", lambda self, *a, **k: calls.append("numpy") or np.zeros(1))
    ev.process(inputs[1:], outputs[1:])
    monkeypatch.undo()
    assert calls == [] and ev._pairs == [] and ev._dev_count == 3 and ev._dev_rows.is_cuda
    assert ev._dev_rows.shape[0] >= 3 and ev._dev_rows.shape[0] % ev.ROW_CHUNK == 0
    small = KITTIDepthEvaluator("x", accumulate="device")                 # growing keeps the rows already written
    small.ROW_CHUNK = 2
    small.process(inputs, outputs)
    assert small._dev_rows.shape[0] == 4 and np.array_equal(_device_rows(small), _device_rows(ev))


def test_reset_and_empty_evaluate(tmp_path):
    from uenc.evaluation import KITTIDepthEvaluator
    inputs, outputs = C.kitti_case(tmp_path)
    ev = KITTIDepthEvaluator("x", accumulate="device")
    ev.process(inputs[:1], _to_cuda(outputs[:1]))
    ev.reset()
    assert ev._dev_rows is None and ev._dev_count == 0
    got, want = ev.evaluate()["depth_error"], KITTIDepthEvaluator("x").evaluate()["depth_error"]
    assert list(got) == list(want) and all(np.isnan(got[k]) and np.isnan(want[k]) for k in got)


def test_image_order_does_not_matter(tmp_path):
    from uenc.evaluation import KITTIDepthEvaluator
    inputs, outputs = C.kitti_case(tmp_path)
    outputs = _to_cuda(outputs)
    a, b = KITTIDepthEvaluator("x", accumulate="device"), KITTIDepthEvaluator("x", accumulate="device")
    a.process(inputs, outputs)
    b.process(inputs[::-1], outputs[::-1])
    ra, rb = _device_rows(a), _device_rows(b)
    assert np.array_equal(ra[np.lexsort(ra.T[::-1])], rb[np.lexsort(rb.T[::-1])]) and np.array_equal(ra, rb[::-1])
    ea, eb = a.evaluate()["depth_error"], b.evaluate()["depth_error"]
    np.testing.assert_allclose([ea[k] for k in ea], [eb[k] for k in eb], rtol=4 * np.finfo(np.float64).eps, atol=0)     # np.mean's own ordering


def test_build_evaluator_passes_accumulate():
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    from uenc.data import MetadataCatalog
    from uenc.evaluation import KITTIDepthEvaluator, build_evaluator
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list(["MODEL.TEST.DEPTH_ON", True])
    name = "depth_eval_test_kitti"
    MetadataCatalog.get(name).set(evaluator_type="kitti_depth")
    for acc in ("device", "host"):
        ev = build_evaluator(cfg, name, accumulate=acc)
        assert type(ev) is KITTIDepthEvaluator and ev._accumulate == acc
    assert build_evaluator(cfg, name)._accumulate == "device"
