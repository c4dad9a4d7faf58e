"""uenc_targets_area / uenc_targets_write (csrc/targets.hip) and the training forward on the GPU: the kernel path bit for bit against the
reference mapper's output (tests/golden/targets.npz) and against the numpy statement of the rules at the shapes that reach each branch
of the kernels, then `model(batch)` in train mode against the criterion composed by hand, losses and gradients."""
import numpy as np
import pytest
import torch

import uenc.modeling.targets as targets_module
from conftest import record_parity
from targets_cases import TASK_NAMES, colliding_ids, infos, load_fixture, numpy_targets, pad_label, pad_masks, prompt, random_annotation

pytestmark = pytest.mark.gpu

LOSS_REL = 1e-6                 # same kernels, same inputs, same order: the expected difference is 0; a few fp32 ulps of headroom
GRAD_REL_L2 = 1e-5              # or twice the hand composition's own run-to-run spread, whichever is larger
HAND_RUNS = 5                   # the spread is the largest difference between any two of this many runs of the hand composition: the
#                                 forward is the same bits every run (the losses differ by 0), the backward is not (float atomics, then
#                                 bf16 roundings that flip), and the difference of one pair of runs has been seen between 5e-6 and 1.5e-3
#                                 on query_embed: one pair alone underestimates it


@pytest.fixture(scope="module")
def TG():
    import model  # noqa: F401  registers the architecture
    return targets_module


def _build(TG, meta, pans, segs, tasks, num_texts=6, size=None):
    return TG.build_targets([torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in pans], [infos(s) for s in segs], [prompt(t) for t in tasks],
                            thing_ids=meta["things"], class_names=meta["class_names"], ignore_label=meta["ignore_label"], num_texts=num_texts,
                            size=size)


def _check_batch(TG, meta, pans, segs, tasks, size=None, num_texts=6):
    """The kernel path on one batch against the numpy rules, image by image, padding included -> the T of every image."""
    H, W = size if size is not None else (max(p.shape[0] for p in pans), max(p.shape[1] for p in pans))
    targets, sem, texts = _build(TG, meta, pans, segs, tasks, num_texts, size)
    torch.cuda.synchronize()
    assert sem.is_cuda and sem.dtype == torch.int64 and tuple(sem.shape) == (len(pans), H, W)
    store = targets[0]["masks"].untyped_storage().data_ptr()
    Ts = []
    for b, (p, s, t) in enumerate(zip(pans, segs, tasks)):
        masks, classes, label, want_texts = numpy_targets(p, s, t, meta["things"], meta["class_names"], meta["ignore_label"], num_texts)
        got = targets[b]["masks"]
        assert got.dtype == torch.uint8 and got.is_contiguous() and got.untyped_storage().data_ptr() == store
        assert tuple(got.shape) == (masks.shape[0], H, W), (b, tuple(got.shape), masks.shape)
        assert np.array_equal(got.cpu().numpy(), pad_masks(masks, H, W)), b
        assert np.array_equal(targets[b]["labels"].cpu().numpy(), classes), b
        assert np.array_equal(sem[b].cpu().numpy(), pad_label(label, H, W, meta["ignore_label"])), b
        assert texts[b] == want_texts, b
        Ts.append(masks.shape[0])
    return Ts


def test_kernel_path_equals_the_reference(TG):
    meta, cases = load_fixture()
    for c in cases:
        targets, sem, texts = _build(TG, meta, [c["pan"]] * 3, [c["segs"]] * 3, TASK_NAMES, c["num_queries"])
        torch.cuda.synchronize()
        for b, t in enumerate(TASK_NAMES):
            ref = c[t]
            assert np.array_equal(targets[b]["masks"].cpu().numpy(), ref["masks"].astype(np.uint8)), (c["name"], t)
            assert np.array_equal(targets[b]["labels"].cpu().numpy(), ref["classes"]), (c["name"], t)
            assert np.array_equal(sem[b].cpu().numpy(), ref["label"]), (c["name"], t)
            assert texts[b] == ref["texts"], (c["name"], t)


def test_padded_batches_on_both_store_paths(TG):
    meta, cases = load_fixture()
    rs = np.random.RandomState(3)
    a, d = cases[0], cases[3]
    mid, mid_segs = random_annotation(rs, 33, 64, [11001, 11002, 7, 9, 13001, 21], crowd_every=4, unlisted=2, empty_listed=1)
    # 64 x 96 = 16 * 384 pixels: 16-byte stores; h_i < H and w_i < W in the first two images
    _check_batch(TG, meta, [a["pan"], mid, d["pan"]], [a["segs"], mid_segs, d["segs"]], ["panoptic", "semantic", "instance"])
    # 24 x 37 = 888 pixels, no multiple of 16: the one-pixel-per-lane path, with a smaller image padded into it
    small, small_segs = random_annotation(rs, 20, 30, [5, 6, 12001, 12002], unlisted=1, blocks=3)
    _check_batch(TG, meta, [a["pan"], small, a["pan"]], [a["segs"], small_segs, a["segs"]], ["semantic", "panoptic", "instance"])
    # an explicit size beyond every image, odd in both directions (35 * 51 = 1785)
    _check_batch(TG, meta, [a["pan"], small], [a["segs"], small_segs], ["panoptic", "instance"], size=(35, 51))


def test_plane_offsets_with_an_empty_image(TG):
    meta, cases = load_fixture()
    a, b = cases[0], cases[1]
    Ts = _check_batch(TG, meta, [a["pan"], b["pan"], a["pan"], b["pan"]], [a["segs"], b["segs"], a["segs"], b["segs"]],
                      ["panoptic", "instance", "semantic", "instance"])
    assert Ts[1] == 0 and Ts[3] == 0 and Ts[0] > 0 and Ts[2] > 0
    Ts = _check_batch(TG, meta, [b["pan"], a["pan"]], [b["segs"], a["segs"]], ["instance", "instance"], size=(32, 48))
    assert Ts == [0, 2]


def test_table_sizes_and_colliding_ids(TG):
    meta, _ = load_fixture()
    rs = np.random.RandomState(4)
    ids = colliding_ids(256)
    h, w = 32, 48                                                   # 1536 = 16 * 96 pixels, every id has at least one
    fill = np.array(ids + [0, 1024 * 300 + 7, 300], dtype=np.int64)            # void and two ids of the map that the table does not list
    pan = np.concatenate([rs.permutation(np.array(ids)), fill[rs.randint(0, len(fill), h * w - 256)]]).reshape(h, w).astype(np.int32)
    full = np.array([(i, k % 19, 0) for k, i in enumerate(ids)], dtype=np.int64)
    one = full[200:201]
    none = np.zeros((0, 3), dtype=np.int64)
    Ts = _check_batch(TG, meta, [pan, pan, pan, pan], [full, none, one, full], ["panoptic", "panoptic", "semantic", "semantic"])
    assert Ts == [256, 0, 1, 19]
    # the same on the narrow path: 31 x 47 = 1457 pixels keeps 256 distinct ids only if they sit in the first rows, which they do
    cut = pan[:31, :47]
    T_cut = _check_batch(TG, meta, [cut, cut], [full, one], ["panoptic", "instance"])
    assert T_cut[0] > 200


def test_several_workgroups_per_image(TG):
    meta, cases = load_fixture()
    e = cases[4]
    rs = np.random.RandomState(5)
    other, other_segs = random_annotation(rs, 90, 150, [1000 * (11 + k % 8) + k for k in range(30)] + [3, 4, 5], crowd_every=7, unlisted=3,
                                          empty_listed=2, blocks=5)
    assert e["pan"].size > 3 * 4096                                  # four chunks of 4096 pixels: four workgroups per image
    _check_batch(TG, meta, [e["pan"], other, e["pan"]], [e["segs"], other_segs, e["segs"]], ["panoptic", "panoptic", "semantic"], num_texts=40)


def test_area_against_bincount(TG):
    from uenc import kernels as K
    meta, cases = load_fixture()
    rs = np.random.RandomState(6)
    ids = colliding_ids(256)
    big = np.array(ids + [0, 999999], dtype=np.int64)[rs.randint(0, 258, (96, 160))].astype(np.int32)
    maps = [(cases[0]["pan"], cases[0]["segs"][:, 0].tolist()), (big, ids), (cases[3]["pan"], cases[3]["segs"][:, 0].tolist()), (big[:50, :70], ids[:100])]
    for H, W in ((96, 160), (97, 161)):                              # 16-byte loads, and the narrow path
        B, S = len(maps), K.TARGETS_MAX_SEGMENTS
        pan = torch.full((B, H, W), 5, dtype=torch.int32)            # id 5 in the padding: it must not be counted
        table = np.zeros(B * (S + 3), dtype=np.int32)
        for b, (m, row_ids) in enumerate(maps):
            pan[b, :m.shape[0], :m.shape[1]] = torch.from_numpy(m)
            table[b * S:b * S + len(row_ids)] = row_ids
            table[B * S + b] = len(row_ids)
            table[B * S + B + 2 * b:B * S + B + 2 * b + 2] = m.shape
        area = K.targets_area(pan.cuda(), torch.from_numpy(table).cuda()).cpu().numpy()
        for b, (m, row_ids) in enumerate(maps):
            values, inverse = np.unique(m, return_inverse=True)      # ids reach 2^24: count their ranks
            counts = dict(zip(values.tolist(), np.bincount(inverse.reshape(-1)).tolist()))
            assert area[b, :len(row_ids)].tolist() == [counts.get(i, 0) for i in row_ids], (H, W, b)
            assert not area[b, len(row_ids):].any()


# ---- the training forward -------------------------------------------------------------------------------------------------------------
def _small_train_model():
    """The small OneFormer of test_matcher_gpu._small_model_outputs in train() mode, every stochastic layer switched off."""
    from oracle import fill
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM", 64,
        "MODEL.SWIN.DEPTHS", [2, 2, 2, 2], "MODEL.SWIN.NUM_HEADS", [2, 4, 8, 16], "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 6, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.SWIN.DROP_PATH_RATE", 0.0, "MODEL.ONE_FORMER.DROPOUT", 0.0,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    fill.fill_module(m)
    m.train()
    return m


def _criterion():
    from uenc.modeling.criterion import SetCriterion
    from uenc.modeling.matcher import HungarianMatcher
    base = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    weights = dict(base)
    for i in range(9):
        weights.update({f"{k}_{i}": v for k, v in base.items()})
    del weights["loss_dice_3"]                                      # a loss without a weight: dropped from the result
    return SetCriterion(19, matcher=HungarianMatcher(2.0, 5.0, 5.0, num_points=448), weight_dict=weights, eos_coef=0.1, losses=["labels", "masks"],
                        num_points=448, oversample_ratio=3.0, importance_sample_ratio=0.75)


def _rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))


@pytest.fixture(scope="module")
def trained():
    """One model, one batch with targets; the training forward through model(batch), and the hand composition twice."""
    import model  # noqa: F401
    m = _small_train_model()
    crit = _criterion().cuda()
    meta, cases = load_fixture()
    g = torch.Generator().manual_seed(11)
    imgs = torch.randint(0, 256, (2, 3, 64, 96), generator=g).float().cuda()
    rs = np.random.RandomState(12)
    pan1, segs1 = random_annotation(rs, 64, 96, [11001, 11002, 13001, 1, 2, 9, 10], crowd_every=5, unlisted=1, blocks=8)
    anns = [(cases[3]["pan"], cases[3]["segs"], "panoptic"), (pan1, segs1, "semantic")]
    plain = [{"left_image": imgs[i], "task": prompt(anns[i][2]), "type": "segmentation"} for i in range(2)]
    batch = [dict(x, pan_seg=torch.from_numpy(np.ascontiguousarray(a[0])), segments_info=infos(a[1])) for x, a in zip(plain, anns)]
    names = {}
    for n, p in m.named_parameters():
        for key in ("query_embed.weight", "class_embed.weight", "mask_embed.layers.0.weight", "qkv.weight"):
            if n.endswith(key) and key not in names:
                names[key] = n
    assert len(names) == 4, names
    params = dict(m.named_parameters())

    def grads():
        out = {k: params[n].grad.detach().clone() for k, n in names.items()}
        m.zero_grad(set_to_none=True)
        return out

    seed = 1234                                                     # fixes the matcher's points and the criterion's draws in every pass
    without = m(batch)                                              # train mode, no criterion: results
    m.set_criterion(crit)
    torch.manual_seed(seed)
    got = m(batch)
    sum(got.values()).backward()
    got_grads = grads()

    def by_hand():
        torch.manual_seed(seed)
        targets = m.training_targets(batch)
        raw = crit(m.forward_features(batch)[0], targets)
        weighted = {k: v * crit.weight_dict[k] for k, v in raw.items() if k in crit.weight_dict}
        sum(weighted.values()).backward()
        return raw, weighted, grads(), targets

    raw, hand, hand_grads, targets = by_hand()
    hand_more = [by_hand()[2] for _ in range(HAND_RUNS - 1)]
    # fixed point_draws handed to both: the matcher's own points still come from the seed
    M, n_unc, n_rnd = crit.point_counts()
    N = sum(min(150, int(t["labels"].shape[0])) for t in targets)
    draws = {"oversampled": torch.rand(10, N, M, 2, generator=g), "random": torch.rand(10, N, n_rnd, 2, generator=g)}
    torch.manual_seed(seed)
    fixed = m.training_losses(batch, point_draws=draws)
    torch.manual_seed(seed)
    fixed_raw = crit(m.forward_features(batch)[0], targets, point_draws=draws)
    no_targets = m(plain)                                           # a criterion, but dicts without targets: results
    m.set_criterion(None)
    again = m(batch)
    torch.cuda.synchronize()
    return dict(model=m, crit=crit, without=without, again=again, no_targets=no_targets, got=got, raw=raw, hand=hand, hand_more=hand_more, got_grads=got_grads,
                hand_grads=hand_grads, fixed=fixed, fixed_raw=fixed_raw, targets=targets, meta=meta, anns=anns)


def test_loss_dict_equals_the_hand_composition(trained):
    t = trained
    crit, got, hand, raw = t["crit"], t["got"], t["hand"], t["raw"]
    assert isinstance(got, dict) and set(got) == set(crit.weight_dict) == set(hand)
    assert "loss_dice_3" in raw and "loss_dice_3" not in got and len(got) == 29
    for b, (pan, segs, task) in enumerate(t["anns"]):               # the targets the model built are the rules' targets
        masks, classes, _, _ = numpy_targets(pan, segs, task, t["meta"]["things"], t["meta"]["class_names"], 255, 0)
        assert np.array_equal(t["targets"][b]["masks"].cpu().numpy(), masks.astype(np.uint8)) and np.array_equal(t["targets"][b]["labels"].cpu().numpy(), classes)
    worst = 0.0
    for k in sorted(got):
        a, b = float(got[k]), float(hand[k])
        rel = abs(a - b) / max(abs(b), 1e-30)
        worst = max(worst, rel)
        print(f"{k}: model(batch) {a:.9g}  by hand {b:.9g}  rel {rel:.3e}")
    fixed_worst = max(abs(float(t["fixed"][k]) - float(t["fixed_raw"][k]) * crit.weight_dict[k]) / max(abs(float(t["fixed"][k])), 1e-30) for k in t["fixed"])
    print(f"worst rel {worst:.3e}; with point_draws given {fixed_worst:.3e}")
    record_parity("targets_loss_dict_vs_hand", worst_rel=worst, worst_rel_fixed_draws=fixed_worst, keys=len(got), bound=LOSS_REL)
    assert all(np.isfinite(float(v)) for v in got.values()) and float(sum(got.values())) > 0
    assert set(t["fixed"]) == set(got)
    assert worst <= LOSS_REL and fixed_worst <= LOSS_REL


def test_gradients_equal_the_hand_composition(trained):
    """Gradients of the summed loss through model(batch) against the hand composition's, per parameter: rel L2 within the larger of 1e-5
    and twice the hand composition's own run-to-run spread (HAND_RUNS runs, largest pairwise difference).  Measured on one MI355X
    (profiles/targets_parity.json): qkv 1.1e-2 against a spread of 1.2e-2, query_embed 2e-5 .. 1.5e-3 against 5e-6 .. 1.1e-4 from
    single pairs, class_embed and mask_embed 3e-8 .. 6e-8."""
    t = trained
    figs, fails = {}, []
    for k, g in t["got_grads"].items():
        h = t["hand_grads"][k]
        runs = [h] + [more[k] for more in t["hand_more"]]
        assert torch.isfinite(g).all() and float(g.abs().max()) > 0, k
        spread = max(_rel_l2(runs[i], runs[j]) for i in range(len(runs)) for j in range(i))
        rel = _rel_l2(g, h)
        bound = max(GRAD_REL_L2, 2 * spread)
        figs[k] = {"rel_l2": rel, "hand_run_to_run": spread, "bound": bound}
        print(f"{k}: rel L2 to the hand composition {rel:.3e}  the hand composition's run-to-run spread {spread:.3e}  bound {bound:.3e}")
        if rel > bound:
            fails.append(k)
    record_parity("targets_gradients_vs_hand", **figs)
    assert not fails, fails


def test_train_mode_without_a_criterion_returns_results(trained):
    t = trained
    for res in (t["without"], t["again"], t["no_targets"]):
        assert isinstance(res, list) and len(res) == 2
        for r in res:
            assert isinstance(r, dict) and tuple(r["pred_logits"].shape) == (150, 20)
    m = t["model"]
    assert m.training and m.criterion is None
