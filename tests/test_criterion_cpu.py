"""SetCriterion on the CPU (uenc/modeling/criterion.py): its torch path against the float64 restatement of tests/criterion_cases.py, its pair
losses against the matcher's reference-pinned pairwise functions, its configuration, and the validity of the cases themselves."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from criterion_cases import CASES, EOS, MIN_GAP, SMALL, build, coef_dict, counts, final_points_sorted, pairs_of, ref64, rel_l2

REL_L2 = 1e-6                   # fp32 torch ops against float64


@pytest.fixture(scope="module")
def C():
    import model  # noqa: F401
    import uenc.modeling.criterion as c
    return c


def make_criterion(C, name, losses=("labels", "masks")):
    from uenc.modeling.matcher import HungarianMatcher
    P, over, imp = CASES[name][6:9]
    return C.SetCriterion(CASES[name][2] - 1, HungarianMatcher(2.0, 5.0, 5.0, num_points=P), coef_dict(build(name)), EOS, list(losses), P, over, imp)


def leaf_outputs(inp, device="cpu"):
    heads = [{k: v.clone().to(device).requires_grad_(True) for k, v in h.items()} for h in inp["heads"]]
    return dict(heads[0], aux_outputs=heads[1:]), heads


def test_facade_and_exports(C):
    import model.modeling.criterion as facade
    import uenc.modeling as um
    assert facade is C and um.SetCriterion is C.SetCriterion and um.build_criterion is C.build_criterion


@pytest.mark.parametrize("name", list(CASES))
def test_cpu_path_against_float64(C, name):
    inp, ref = build(name), ref64(name)
    crit = make_criterion(C, name)
    outputs, heads = leaf_outputs(inp)
    losses = crit(outputs, inp["targets"], indices=inp["indices"], point_draws=inp["draws"])
    assert set(losses) == set(coef_dict(inp))
    crit.weighted_sum(losses).backward()
    for i, (hd, r) in enumerate(zip(heads, ref)):
        sfx = "" if i == 0 else f"_{i - 1}"
        for k in ("loss_ce", "loss_mask", "loss_dice"):
            got = float(losses[k + sfx].detach())
            print(f"{name} head {i} {k}: {got:.9g} (float64 {r[k]:.9g})")
            assert abs(got - r[k]) <= REL_L2 * max(abs(r[k]), 1e-30) or (r[k] == 0.0 and got == 0.0), (name, i, k, got, r[k])
        e_m, e_l = rel_l2(hd["pred_masks"].grad, r["g_masks"]), rel_l2(hd["pred_logits"].grad, r["g_logits"])
        print(f"{name} head {i}: gradient rel L2 masks {e_m:.3e} logits {e_l:.3e}")
        if inp["N"]:
            assert e_m <= REL_L2, (name, i, e_m)
        else:                                            # no pair: exact zeros, and a zero gradient that still reaches pred_masks
            assert float(losses["loss_mask" + sfx]) == 0.0 and float(losses["loss_dice" + sfx]) == 0.0
            assert hd["pred_masks"].grad is not None and not hd["pred_masks"].grad.any()
        assert e_l <= REL_L2, (name, i, e_l)


@pytest.mark.parametrize("name", [c for c in SMALL if c != "H"])
def test_pair_losses_are_the_matcher_diagonal(C, name):
    """ce_n / dice_n on the sampled points equal the diagonal of the matcher's pairwise losses (pinned to the reference by the golden
    matcher tests), and the CPU path's losses are their sums over num_masks."""
    from uenc.modeling.matcher import batch_dice_loss, batch_sigmoid_ce_loss, point_sample
    inp, ref = build(name), ref64(name)
    crit = make_criterion(C, name)
    points = crit.select_points(inp["outputs"], inp["targets"], inp["indices"], point_draws=inp["draws"])
    losses = crit(inp["outputs"], inp["targets"], indices=inp["indices"], point_draws=inp["draws"])
    for i, (hd, r) in enumerate(zip(inp["heads"], ref)):
        prs = pairs_of(inp["indices"][i])
        n_unc = counts(name)[1]                          # the CPU path selects the float64 restatement's SET (top-k's order is its own)
        assert torch.equal(final_points_sorted(points[i], n_unc), final_points_sorted(r["points"], n_unc))
        assert torch.equal(points[i][:, n_unc:], r["points"][:, n_unc:])
        src = torch.stack([hd["pred_masks"][b, q] for b, q, _ in prs])[:, None]
        tgt = torch.stack([inp["targets"][b]["masks"][t] for b, _, t in prs]).float()[:, None]
        x = point_sample(src, points[i], align_corners=False).squeeze(1)
        t = point_sample(tgt, points[i], align_corners=False).squeeze(1)
        ce, dice = C.SetCriterion.pair_losses(x, t)
        assert rel_l2(ce, batch_sigmoid_ce_loss(x, t).diagonal()) <= REL_L2 and rel_l2(dice, batch_dice_loss(x, t).diagonal()) <= REL_L2
        assert rel_l2(ce, r["ce"]) <= REL_L2 and rel_l2(dice, r["dice"]) <= REL_L2
        sfx = "" if i == 0 else f"_{i - 1}"
        assert rel_l2(losses["loss_mask" + sfx], ce.sum() / inp["num_masks"]) <= REL_L2
        assert rel_l2(losses["loss_dice" + sfx], dice.sum() / inp["num_masks"]) <= REL_L2


@pytest.mark.parametrize("name", ["B", "C", "H"])
def test_loss_ce_is_weighted_cross_entropy(C, name):
    inp, ref = build(name), ref64(name)
    crit = make_criterion(C, name, losses=("labels",))
    losses = crit(inp["outputs"], inp["targets"], indices=inp["indices"])
    assert set(losses) == {k for k in coef_dict(inp) if k.startswith("loss_ce")}
    w = torch.ones(CASES[name][2])
    w[-1] = EOS
    for i, (hd, r) in enumerate(zip(inp["heads"], ref)):
        want = F.cross_entropy(hd["pred_logits"].transpose(1, 2), r["target_classes"], w)
        assert rel_l2(losses["loss_ce" + ("" if i == 0 else f"_{i - 1}")], want) <= REL_L2
    if name == "C":                                      # three pairs for five targets; the repeated label is hit
        y = ref[0]["target_classes"]
        assert (y != CASES[name][2] - 1).sum() == 3


def test_case_validity():
    """Every pair of every case that uses top-k has a float64 gap >= 1e-3 in |logit| between the last kept and the first dropped
    oversampled point, so an fp32 kernel must select the identical set."""
    checked = 0
    for name in CASES:
        M, n_unc, _ = counts(name)
        if not n_unc or not build(name)["N"]:
            continue
        for i, r in enumerate(ref64(name)):
            assert r["gap"].shape == (build(name)["N"],)
            assert float(r["gap"].min()) >= MIN_GAP, (name, i, float(r["gap"].min()))
            checked += r["gap"].numel()
    assert checked >= 260 + 20
    assert counts("F") == (37632, 9408, 3136) and counts("G") == (25, 3, 7) and counts("G0")[1] == 0 and counts("G1")[2] == 0
    kinds = {CASES[c][10] for c in CASES}
    assert kinds == {"bool", "uint8", "float"}


def test_case_e_reaches_dropped_taps():
    inp = build("E")
    pts = inp["draws"]["random"]
    assert (pts == 0.0).any() and (pts.max() < 1.0) and float(pts.max()) == float(torch.nextafter(torch.tensor(1.0), torch.tensor(0.0)))


def test_build_criterion_from_the_reference_config(C):
    from uenc.config import add_common_config, add_dinat_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    from uenc.modeling.matcher import HungarianMatcher
    flat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "cfg_cityscapes_swin_t.json")))["cfg"]
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_dinat_config(cfg); add_uni_encoder_config(cfg)
    opts = []
    for k, v in flat.items():
        opts += [k, v]
    cfg.merge_from_list(opts)
    crit = C.build_criterion(cfg)
    base = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    want = dict(base)
    for i in range(9):                                   # DEC_LAYERS 10, DEEP_SUPERVISION
        want.update({f"{k}_{i}": v for k, v in base.items()})
    assert crit.weight_dict == want
    assert crit.eos_coef == 0.1 and crit.num_classes == 19 and crit.losses == ["labels", "masks"]
    assert float(crit.empty_weight[-1]) == pytest.approx(0.1) and crit.empty_weight.shape == (20,) and float(crit.empty_weight[:-1].min()) == 1.0
    assert (crit.num_points, crit.oversample_ratio, crit.importance_sample_ratio) == (12544, 3.0, 0.75)
    assert crit.point_counts() == (37632, 9408, 3136)
    m = crit.matcher
    assert isinstance(m, HungarianMatcher) and (m.cost_class, m.cost_mask, m.cost_dice, m.num_points) == (2.0, 5.0, 5.0, 12544)
    cfg.merge_from_list(["MODEL.ONE_FORMER.DEEP_SUPERVISION", False])
    assert C.build_criterion(cfg).weight_dict == base


def test_contrastive_and_unknown_losses_raise(C):
    from uenc.modeling.matcher import HungarianMatcher
    m = HungarianMatcher(1, 1, 1, num_points=4)
    with pytest.raises(NotImplementedError, match="text encoder"):
        C.SetCriterion(3, m, {}, 0.1, ["labels", "masks", "contrastive"], 4, 3.0, 0.75)
    with pytest.raises(ValueError):
        C.SetCriterion(3, m, {}, 0.1, ["boxes"], 4, 3.0, 0.75)


def test_weighted_sum_uses_only_known_keys(C):
    crit = make_criterion(C, "A")
    crit.weight_dict = {"loss_ce": 2.0, "loss_dice": 3.0}
    got = crit.weighted_sum({"loss_ce": torch.tensor(1.5), "loss_mask": torch.tensor(100.0), "loss_dice": torch.tensor(0.5)})
    assert float(got) == 4.5


def test_pad_targets(C):
    g = torch.Generator().manual_seed(3)
    tg = [{"labels": torch.tensor([1, 2]), "masks": torch.rand(2, 5, 7, generator=g) > 0.5},
          {"labels": torch.tensor([0]), "masks": (torch.rand(1, 8, 4, generator=g) > 0.5).to(torch.uint8)},
          {"labels": torch.zeros(0, dtype=torch.int64), "masks": torch.zeros(0, 3, 3)}]
    out = C.pad_targets(tg, (8, 9))
    for a, b in zip(tg, out):
        assert b["masks"].shape == (a["masks"].shape[0], 8, 9) and b["masks"].dtype == a["masks"].dtype and b["labels"] is a["labels"]
        hh, ww = a["masks"].shape[1:]
        assert torch.equal(b["masks"][:, :hh, :ww], a["masks"]) and not b["masks"][:, hh:].any() and not b["masks"][:, :, ww:].any()
    assert tg[0]["masks"].shape == (2, 5, 7)             # the input is left alone
    with pytest.raises(ValueError):
        C.pad_targets(tg, (7, 9))


def test_default_draws_and_matching_on_the_cpu(C):
    """Nothing injected: the criterion matches and draws its own points; two calls draw different points."""
    inp = build("B")
    crit = make_criterion(C, "B")
    a = crit(inp["outputs"], inp["targets"])
    b = crit(inp["outputs"], inp["targets"])
    assert all(torch.isfinite(v) for v in a.values()) and set(a) == set(b)
    assert any(float(a[k].detach()) != float(b[k].detach()) for k in a if k.startswith("loss_mask"))


def test_wrong_index_layout_is_refused(C):
    inp = build("B")
    crit = make_criterion(C, "B")
    bad = [[(i[:-1], j[:-1]) if i.numel() else (i, j) for i, j in head] for head in inp["indices"]]
    with pytest.raises(ValueError):
        crit(inp["outputs"], inp["targets"], indices=bad, point_draws=inp["draws"])
    with pytest.raises(ValueError):
        crit(inp["outputs"], inp["targets"], indices=inp["indices"], point_draws={"oversampled": inp["draws"]["oversampled"][:, :, :5],
                                                                                  "random": inp["draws"]["random"]})
