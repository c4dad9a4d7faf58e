"""HungarianMatcher (uenc/modeling/matcher.py) without a GPU: the torch + scipy path against what the reference's own module computed
(tests/golden/matcher.npz, written by tools/make_matcher_golden.py), and the module's contract."""
import numpy as np
import pytest
import torch

from matcher_fixture import calls, check_assignment, load_problems, rel_l2

COST_REL_L2 = 2e-5              # fp32 torch against fp32 torch: the bar tests/test_oracle_golden.py holds the oracle to


@pytest.fixture(scope="module")
def M():
    import uenc.modeling.matcher as m
    return m


@pytest.fixture(scope="module")
def problems():
    return load_problems()


def _matcher(M, pr, **kw):
    w = pr["weights"]
    return M.HungarianMatcher(cost_class=w[0], cost_mask=w[1], cost_dice=w[2], num_points=pr["num_points"], **kw)


def test_fixture_covers_the_cases(problems):
    shapes = {tuple(pr["cost"].shape) for pr in problems}
    assert {(150, 17), (150, 40), (100, 5), (20, 31), (150, 1), (150, 0)} <= shapes
    assert any(pr["num_points"] == 12544 for pr in problems) and any(np.isnan(pr["cost_raw"]).any() for pr in problems)
    assert len({pr["weights"] for pr in problems}) >= 2 and (2.0, 5.0, 5.0) in {pr["weights"] for pr in problems}
    nonempty = [pr for pr in problems if pr["cost"].shape[1]]
    assert 2 * sum(pr["stable"] for pr in nonempty) >= len(nonempty)


def test_cpu_cost_and_indices_match_reference(M, problems):
    for outputs, targets, points, ps in calls(problems):
        m = _matcher(M, ps[0])
        costs = m.cost_matrices(outputs, targets, point_coords=points)
        indices = m(outputs, targets, point_coords=points)
        for pr, C, (i, j) in zip(ps, costs, indices):
            assert tuple(C.shape) == pr["cost"].shape and i.dtype == torch.int64 and j.dtype == torch.int64 and not i.is_cuda
            e = 0.0
            if C.numel():
                err = rel_l2(C.numpy(), pr["cost"])
                e = float(np.abs(C.numpy().astype(np.float64) - pr["cost"]).max())
                print(f"problem {pr['index']}: cost rel L2 {err:.3e}  max abs {e:.3e}")
                assert err <= COST_REL_L2, (pr["index"], err)
            check_assignment(i.numpy(), j.numpy(), pr, e)
            if pr["stable"]:
                assert np.array_equal(i.numpy(), pr["row"]) and np.array_equal(j.numpy(), pr["col"]), pr["index"]


def test_default_points_consume_the_generator_like_the_reference(M, problems):
    for outputs, targets, points, ps in calls(problems)[:3]:
        m = _matcher(M, ps[0])
        torch.manual_seed(ps[0]["seed"])
        drawn = m(outputs, targets)
        given = m(outputs, targets, point_coords=points)
        for (i, j), (i2, j2), pr in zip(drawn, given, ps):
            assert torch.equal(i, i2) and torch.equal(j, j2)
        torch.manual_seed(ps[0]["seed"])
        pts = m._points(1, len(ps), torch.device("cpu"), None)[0]
        for p, pr in zip(pts, ps):
            assert torch.equal(p, pr["points"])


def test_match_all_equals_per_head_forward(M):
    g = torch.Generator().manual_seed(3)
    bs, Q, C1, h, w, P = 2, 30, 11, 8, 12, 96
    heads = [{"pred_logits": torch.randn(bs, Q, C1, generator=g), "pred_masks": torch.randn(bs, Q, h, w, generator=g) * 3} for _ in range(4)]
    outputs = dict(heads[0], aux_outputs=heads[1:])
    targets = [{"labels": torch.randint(0, C1 - 1, (T,), generator=g), "masks": torch.rand(T, 4 * h, 4 * w, generator=g) > 0.6} for T in (7, 40)]
    pts = torch.rand(4, bs, P, 2, generator=g)
    m = M.HungarianMatcher(2, 5, 5, num_points=P)
    every = m.match_all(outputs, targets, point_coords=pts)
    assert len(every) == 4
    for k, head in enumerate(heads):
        single = m(head, targets, point_coords=pts[k])
        for (i, j), (i2, j2) in zip(every[k], single):
            assert torch.equal(i, i2) and torch.equal(j, j2)
    assert len(every[0][1][0]) == Q                      # more targets than queries: every query matched
    # drawn points: the final head first, then the auxiliary heads, one draw per image
    torch.manual_seed(11)
    a = m.match_all(outputs, targets)
    torch.manual_seed(11)
    b = [m(head, targets) for head in heads]
    for x, y in zip(a, b):
        for (i, j), (i2, j2) in zip(x, y):
            assert torch.equal(i, i2) and torch.equal(j, j2)


def test_host_solver_nan_policy(M):
    c = np.array([[1.0, np.nan, 3.0], [2.0, 0.5, np.nan]])
    i, j = M.linear_sum_assignment_with_nan(c)
    assert i.tolist() == [0, 1] and j.tolist() == [0, 1] and np.isnan(c[0, 1])          # the caller's matrix is left alone
    i, j = M.linear_sum_assignment_with_nan(np.array([[np.nan, 1.0], [1.0, np.nan], [150.0, 150.0]]))
    assert i.tolist() == [0, 1] and j.tolist() == [1, 0]                                # NaN counts as 100: dearer than 1, cheaper than 150
    i, j = M.linear_sum_assignment_with_nan(np.full((4, 3), np.nan))
    assert len(i) == 0 and len(j) == 0                                                  # all NaN: the empty assignment
    i, j = M.linear_sum_assignment_with_nan(np.zeros((5, 0)))
    assert len(i) == 0 and len(j) == 0


def test_edge_cases_on_cpu(M):
    g = torch.Generator().manual_seed(5)
    Q, C1, h, w, P = 12, 6, 6, 8, 50
    m = M.HungarianMatcher(1, 1, 1, num_points=P)
    out = {"pred_logits": torch.randn(1, Q, C1, generator=g), "pred_masks": torch.randn(1, Q, h, w, generator=g)}
    empty = [{"labels": torch.zeros(0, dtype=torch.int64), "masks": torch.zeros(0, 4 * h, 4 * w, dtype=torch.bool)}]
    (i, j), = m(out, empty)
    assert i.numel() == 0 and j.numel() == 0 and i.dtype == torch.int64
    many = [{"labels": torch.randint(0, C1 - 1, (20,), generator=g), "masks": torch.rand(20, 4 * h, 4 * w, generator=g) > 0.5}]
    (i, j), = m(out, many)
    assert i.tolist() == list(range(Q)) and len(set(j.tolist())) == Q
    bad = {"pred_logits": torch.full((1, Q, C1), float("nan")), "pred_masks": out["pred_masks"]}
    (i, j), = m(bad, many)                               # every entry NaN: the reference returns the empty assignment
    assert i.numel() == 0 and j.numel() == 0
    with pytest.raises(ValueError):
        m(out, many, solver="device")                    # CPU inputs have no device solver


def test_constructor_repr_and_exports(M):
    with pytest.raises(AssertionError, match="all costs cant be 0"):
        M.HungarianMatcher(0, 0, 0)
    m = M.HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=12544)
    assert repr(m) == "Matcher HungarianMatcher\n    cost_class: 2.0\n    cost_mask: 5.0\n    cost_dice: 5.0"
    assert (m.cost_class, m.cost_mask, m.cost_dice, m.num_points) == (2.0, 5.0, 5.0, 12544)
    d = M.HungarianMatcher()
    assert (d.cost_class, d.cost_mask, d.cost_dice, d.num_points) == (1, 1, 1, 0)
    with pytest.raises(ValueError):
        M.HungarianMatcher(solver="gpu")
    x, t = torch.tensor([[0.0, 2.0, -2.0]]), torch.tensor([[1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    s = torch.sigmoid(x)
    assert torch.allclose(M.batch_dice_loss(x, t), 1 - (2 * (s * t[None]).sum(-1) + 1) / (s.sum() + t.sum(-1) + 1))
    sp = torch.nn.functional.softplus
    assert torch.allclose(M.batch_sigmoid_ce_loss(x, t), ((sp(-x) * t[None]).sum(-1) + (sp(x) * (1 - t[None])).sum(-1)) / 3)


def test_facade_resolves_to_the_same_modules():
    import model
    import uenc.modeling
    import uenc.modeling.matcher as um
    from model.modeling.matcher import HungarianMatcher, batch_dice_loss, batch_sigmoid_ce_loss  # noqa: F401
    import model.modeling.matcher as mm
    assert model.modeling is uenc.modeling and mm is um and HungarianMatcher is um.HungarianMatcher
    from model.modeling import D2SwinTransformer  # noqa: F401  what importing `model` offered before still resolves
    assert "modeling" in model.__all__ and hasattr(model, "OneFormer") and hasattr(model, "add_common_config")
