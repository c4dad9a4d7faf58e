"""uenc.modeling.targets on the CPU: the rules against the reference mapper's own output (tests/golden/targets.npz), and the refusals."""
import numpy as np
import pytest
import torch

import uenc.modeling.targets as targets_module
from targets_cases import TASK_NAMES, infos, load_fixture, numpy_targets, pad_label, pad_masks, prompt, random_annotation


@pytest.fixture(scope="module")
def TG():
    return targets_module


def _build(TG, meta, pans, segs, tasks, num_texts, size=None, **kw):
    return TG.build_targets(pans, [infos(s) for s in segs], [prompt(t) for t in tasks], thing_ids=meta["things"],
                            class_names=meta["class_names"], ignore_label=meta["ignore_label"], num_texts=num_texts, size=size, **kw)


def test_fixture_holds_the_cases_it_promises():
    meta, cases = load_fixture()
    by = {c["name"]: c for c in cases}
    assert [c["name"] for c in cases] == list("abcde") and len(meta["class_names"]) == 19 and meta["things"] == list(range(11, 19))
    a = by["a"]
    ids, cat, crowd = a["segs"][:, 0], a["segs"][:, 1], a["segs"][:, 2]
    present = set(np.unique(a["pan"]).tolist())
    assert a["pan"].shape == (24, 37) and crowd.any() and any(int(i) not in present for i in ids)
    assert (present - {0}) - set(ids.tolist())                                       # a map id the table does not list
    assert a["panoptic"]["classes"].tolist().count(13) == 2                          # two instances of one thing class
    assert a["panoptic"]["classes"].tolist().count(0) == 2 and a["semantic"]["classes"].tolist().count(0) == 1
    assert by["b"]["instance"]["masks"].shape[0] == 0 and not (by["b"]["instance"]["label"] != meta["ignore_label"]).any()
    c = by["c"]
    assert c["num_queries"] == 5 and c["panoptic"]["masks"].shape[0] > 5 and all(t.startswith("a photo with a ") for t in c["panoptic"]["texts"])
    assert by["d"]["pan"].shape == (64, 96) and by["d"]["pan"].max() == 2 ** 24 - 1
    assert by["e"]["pan"].shape == (96, 160) and len(by["e"]["segs"]) == 60


def test_numpy_rules_equal_the_reference():
    meta, cases = load_fixture()
    for c in cases:
        for t in TASK_NAMES:
            masks, classes, label, texts = numpy_targets(c["pan"], c["segs"], t, meta["things"], meta["class_names"], meta["ignore_label"], c["num_queries"])
            ref = c[t]
            assert masks.shape == ref["masks"].shape and np.array_equal(masks, ref["masks"]), (c["name"], t)
            assert np.array_equal(classes, ref["classes"]) and np.array_equal(label, ref["label"]), (c["name"], t)
            assert texts == ref["texts"], (c["name"], t)


def test_cpu_path_equals_the_reference(TG):
    meta, cases = load_fixture()
    for c in cases:
        h, w = c["pan"].shape
        targets, sem, texts = _build(TG, meta, [torch.from_numpy(c["pan"])] * 3, [c["segs"]] * 3, TASK_NAMES, c["num_queries"])
        assert sem.dtype == torch.int64 and tuple(sem.shape) == (3, h, w)
        for b, t in enumerate(TASK_NAMES):
            ref = c[t]
            assert targets[b]["masks"].dtype == torch.uint8 and targets[b]["labels"].dtype == torch.int64
            assert np.array_equal(targets[b]["masks"].numpy(), ref["masks"].astype(np.uint8)), (c["name"], t)
            assert np.array_equal(targets[b]["labels"].numpy(), ref["classes"]), (c["name"], t)
            assert np.array_equal(sem[b].numpy(), ref["label"]), (c["name"], t)
            assert texts[b] == ref["texts"], (c["name"], t)
        # all images are views of one allocation, in order
        store = targets[0]["masks"].untyped_storage().data_ptr()
        assert all(t["masks"].untyped_storage().data_ptr() == store for t in targets)


def test_cpu_path_pads_a_mixed_batch(TG):
    meta, cases = load_fixture()
    picks = [(cases[0], "panoptic"), (cases[1], "instance"), (cases[3], "semantic"), (cases[2], "instance")]
    H, W = 64, 128
    targets, sem, texts = _build(TG, meta, [c["pan"] for c, _ in picks], [c["segs"] for c, _ in picks], [t for _, t in picks], 7, size=(H, W))
    for b, (c, t) in enumerate(picks):
        ref = c[t]
        assert np.array_equal(targets[b]["masks"].numpy(), pad_masks(ref["masks"], H, W)), b
        assert np.array_equal(sem[b].numpy(), pad_label(ref["label"], H, W, meta["ignore_label"])), b
        assert np.array_equal(targets[b]["labels"].numpy(), ref["classes"])
        assert texts[b] == numpy_targets(c["pan"], c["segs"], t, meta["things"], meta["class_names"], meta["ignore_label"], 7)[3]
    assert targets[1]["masks"].shape == (0, H, W) and targets[1]["labels"].shape == (0,)


def test_targets_from_instances(TG):
    from uenc.d2 import Instances
    meta, cases = load_fixture()
    picks = [(cases[0], "panoptic"), (cases[1], "instance"), (cases[4], "semantic")]
    inst = []
    for c, t in picks:
        i = Instances(c["pan"].shape)
        i.gt_classes = torch.from_numpy(c[t]["classes"])
        i.gt_masks = torch.from_numpy(c[t]["masks"])
        inst.append(i)
    H, W = 96, 160
    got = TG.targets_from_instances(inst, (H, W))
    want, _, _ = _build(TG, meta, [c["pan"] for c, _ in picks], [c["segs"] for c, _ in picks], [t for _, t in picks], 3, size=(H, W))
    for g, w_ in zip(got, want):
        assert g["masks"].dtype == torch.uint8 and torch.equal(g["masks"], w_["masks"]) and torch.equal(g["labels"], w_["labels"])
    with pytest.raises(ValueError, match="do not fit"):
        TG.targets_from_instances(inst, (95, 160))


def test_rgb2id():
    from uenc.data import rgb2id
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (5, 7, 3)).astype(np.uint8)
    img[0, 0] = (255, 255, 255)
    ids = rgb2id(img)
    assert ids.shape == (5, 7) and ids.dtype == np.int32 and ids[0, 0] == 2 ** 24 - 1
    want = img[..., 0].astype(np.int64) + 256 * img[..., 1].astype(np.int64) + 65536 * img[..., 2].astype(np.int64)
    assert np.array_equal(ids, want)
    assert rgb2id([1, 2, 3]) == 1 + 512 + 3 * 65536 and isinstance(rgb2id(img[1, 1]), int)


def test_refusals(TG):
    meta, _ = load_fixture()
    rs = np.random.RandomState(1)
    pan, segs = random_annotation(rs, 8, 12, [3, 4, 5])
    ok = dict(thing_ids=meta["things"], class_names=meta["class_names"], num_texts=4)
    TG.build_targets([pan], [infos(segs)], [prompt("panoptic")], **ok)
    with pytest.raises(ValueError, match="more than 256 segments"):
        TG.build_targets([pan], [infos([(k + 1, 0, 0) for k in range(257)])], [prompt("panoptic")], **ok)
    with pytest.raises(ValueError, match="id <= 0"):
        TG.build_targets([pan], [infos([(3, 0, 0), (0, 1, 0)])], [prompt("panoptic")], **ok)
    with pytest.raises(ValueError, match="id <= 0"):
        TG.build_targets([pan], [infos([(-7, 0, 0)])], [prompt("panoptic")], **ok)
    with pytest.raises(ValueError, match="duplicate segment id"):
        TG.build_targets([pan], [infos([(3, 0, 0), (4, 1, 0), (3, 2, 0)])], [prompt("panoptic")], **ok)
    with pytest.raises(ValueError, match="larger than size"):
        TG.build_targets([pan], [infos(segs)], [prompt("panoptic")], size=(8, 11), **ok)
    with pytest.raises(ValueError, match="unknown task"):
        TG.build_targets([pan], [infos(segs)], ["The task is depth"], **ok)
    with pytest.raises(ValueError):
        TG.build_targets([pan, pan], [infos(segs)], [prompt("panoptic")], **ok)
    with pytest.raises(ValueError, match="integer id maps"):
        TG.build_targets([pan.astype(np.float32)], [infos(segs)], [prompt("panoptic")], **ok)


def test_reachable_through_the_reference_package_name(TG):
    import model  # noqa: F401
    from model.modeling.targets import build_targets, targets_from_instances
    assert build_targets is TG.build_targets and targets_from_instances is TG.targets_from_instances


def test_training_forward_dispatch_without_a_gpu():
    """forward() takes the training path only in train mode, with a criterion and with targets in the dicts; sequence dicts raise there."""
    import model  # noqa: F401
    from uenc.oneformer_model import OneFormer
    m = OneFormer.__new__(OneFormer)
    torch.nn.Module.__init__(m)
    m.criterion = None
    calls = []
    m.training_losses = lambda batch, point_draws=None: calls.append("losses") or {"loss_ce": 0}
    m._forward_segmentation = lambda batch: calls.append("results") or [{}]
    plain = [{"type": "segmentation"}]
    tgt = [{"type": "segmentation", "pan_seg": None, "segments_info": []}]
    m.train()
    assert m(tgt) == [{}]                                       # no criterion: results, as before
    m.set_criterion(torch.nn.Identity())
    assert m(plain) == [{}]                                     # no targets in the dicts
    assert m(tgt) == {"loss_ce": 0} and m([{"type": "segmentation", "instances": None}]) == {"loss_ce": 0}
    m.eval()
    assert m(tgt) == [{}]
    assert calls == ["results", "results", "losses", "losses", "results"]
    del m.training_losses
    m.train()
    with pytest.raises(ValueError, match="sequence"):
        m(tgt + [{"type": "sequence"}])
    m.set_criterion(None)
    with pytest.raises(RuntimeError, match="no criterion"):
        m.training_losses(tgt)
