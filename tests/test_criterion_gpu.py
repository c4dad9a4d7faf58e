"""SetCriterion on the GPU (csrc/criterion.hip behind uenc/modeling/criterion.py) against its own CPU path on the same injected draws and
host-solver indices, its default draws, the empty batch, and matcher + criterion + backward recorded in one stream capture."""
import pytest
import torch

from conftest import record_parity
from criterion_cases import CASES, EOS, build, coef_dict, counts, final_points_sorted, pairs_of, ref64, rel_l2, separate
from matcher_fixture import calls, load_problems

pytestmark = pytest.mark.gpu

REL_L2 = 1e-4                   # the project's bar for fp32 kernels


@pytest.fixture(scope="module")
def C():
    import model  # noqa: F401  loads libuenc_hip.so
    import uenc.modeling.criterion as c
    return c


def criterion(C, num_classes, P, over, imp, weights):
    from uenc.modeling.matcher import HungarianMatcher
    return C.SetCriterion(num_classes, HungarianMatcher(2.0, 5.0, 5.0, num_points=P), weights, EOS, ["labels", "masks"], P, over, imp)


def leaves(heads, device):
    hs = [{k: v.clone().to(device).requires_grad_(True) for k, v in h.items()} for h in heads]
    return dict(hs[0], aux_outputs=hs[1:]), hs


def host_indices(crit, heads, targets, seed):
    """The matcher's host-solver indices for GPU inputs, at matcher points fixed by `seed`."""
    P = crit.matcher.num_points
    pts = torch.rand(len(heads), len(targets), P, 2, generator=torch.Generator().manual_seed(seed)).cuda()
    hs = [{k: v.cuda() for k, v in h.items()} for h in heads]
    indices = crit.matcher.match_all(dict(hs[0], aux_outputs=hs[1:]), [{k: v.cuda() for k, v in t.items()} for t in targets], point_coords=pts,
                                     solver="host")
    assert all(not qi.is_cuda for head in indices for qi, _ in head)
    return indices


def compare(tag, crit, heads, targets, indices, draws):
    """One call on the GPU and one on the CPU with the same indices and draws: all losses, all gradients of every head."""
    out_g, hs_g = leaves(heads, "cuda")
    out_c, hs_c = leaves(heads, "cpu")
    tg_g = [{k: v.cuda() for k, v in t.items()} for t in targets]
    lg = crit(out_g, tg_g, indices=indices, point_draws=draws)
    lc = crit(out_c, targets, indices=indices, point_draws=draws)
    assert set(lg) == set(lc) and len(lg) == 3 * len(heads)
    crit.weighted_sum(lg).backward()
    crit.weighted_sum(lc).backward()
    torch.cuda.synchronize()
    figs = {}
    for k in sorted(lg):
        figs[k] = abs(float(lg[k].detach()) - float(lc[k].detach())) / max(abs(float(lc[k].detach())), 1e-30)
    for i, (a, b) in enumerate(zip(hs_g, hs_c)):
        figs[f"g_masks_{i}"] = rel_l2(a["pred_masks"].grad, b["pred_masks"].grad)
        figs[f"g_logits_{i}"] = rel_l2(a["pred_logits"].grad, b["pred_logits"].grad)
    worst = max(figs.values())
    print(f"{tag}: worst relative deviation GPU vs CPU {worst:.3e} over {len(figs)} figures")
    record_parity(f"criterion_gpu_vs_cpu/{tag}", worst=worst, **{k: v for k, v in figs.items() if not k.startswith("g_") or k.endswith("_0")})
    assert worst <= REL_L2, {k: v for k, v in figs.items() if v > REL_L2}


@pytest.mark.parametrize("name", ["B", "F"])
def test_gpu_equals_cpu_on_cases(C, name):
    inp = build(name)
    P, over, imp = CASES[name][6:9]
    crit = criterion(C, inp["num_classes"], P, over, imp, coef_dict(inp)).cuda()
    # the cases' draws are separated for the cases' own fixed indices; the matcher picks other pairs, so separate again for those
    indices = host_indices(crit, inp["heads"], inp["targets"], seed=4)
    draws = separated_draws(inp["heads"], indices, P, over, imp, seed=5)
    compare(name, crit, inp["heads"], inp["targets"], indices, draws)
    out_g = dict({k: v.cuda() for k, v in inp["heads"][0].items()}, aux_outputs=[{k: v.cuda() for k, v in h.items()} for h in inp["heads"][1:]])
    # identical selected point sets, every pair of every head
    n_unc = int(imp * P)
    pg = crit.select_points(out_g, [{k: v.cuda() for k, v in t.items()} for t in inp["targets"]], indices, point_draws=draws).cpu()
    pc = crit.select_points(inp["outputs"], inp["targets"], indices, point_draws=draws)
    for i in range(len(inp["heads"])):
        assert torch.equal(final_points_sorted(pg[i], n_unc), final_points_sorted(pc[i], n_unc)), (name, i)
        assert torch.equal(pg[i][:, n_unc:], pc[i][:, n_unc:])


def separated_draws(heads, indices, P, over, imp, seed):
    gen = torch.Generator().manual_seed(seed)
    M, n_unc = int(P * over), int(imp * P)
    N = sum(qi.numel() for qi, _ in indices[0])
    ov = torch.rand(len(heads), N, M, 2, generator=gen)
    rnd = torch.rand(len(heads), N, P - n_unc, 2, generator=gen)
    for i, hd in enumerate(heads):
        src = torch.stack([hd["pred_masks"][b, q] for b, q, _ in pairs_of(indices[i])]).double()
        ov[i] = separate(src, ov[i].clone(), n_unc, 0, gen)
    return {"oversampled": ov, "random": rnd}


def test_gpu_equals_cpu_on_the_golden_matcher_problems(C):
    """The problems of tests/golden/matcher.npz, one criterion call per recorded matcher call (those with a target at all)."""
    done = 0
    for outputs, targets, _, ps in calls(load_problems()):
        if sum(t["labels"].numel() for t in targets) == 0:
            continue
        C1, P = outputs["pred_logits"].shape[-1], min(ps[0]["num_points"], 400)
        heads = [outputs]
        crit = criterion(C, C1 - 1, P, 3.0, 0.75, {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}).cuda()
        indices = host_indices(crit, heads, targets, seed=ps[0]["call"])
        draws = separated_draws(heads, indices, P, 3.0, 0.75, seed=ps[0]["call"])
        compare(f"golden_call{ps[0]['call']}", crit, heads, targets, indices, draws)
        done += 1
    assert done >= 7


def test_default_draws_are_fresh_and_finite(C):
    inp = build("B")
    P, over, imp = CASES["B"][6:9]
    crit = criterion(C, inp["num_classes"], P, over, imp, coef_dict(inp)).cuda()
    out_g, _ = leaves(inp["heads"], "cuda")
    tg_g = [{k: v.cuda() for k, v in t.items()} for t in inp["targets"]]
    a, b = crit(out_g, tg_g), crit(out_g, tg_g)          # device matcher, torch.rand on the device
    assert all(v.is_cuda and bool(torch.isfinite(v)) for v in a.values()) and set(a) == set(b) == set(coef_dict(inp))
    assert any(float(a[k].detach()) != float(b[k].detach()) for k in a if k.startswith("loss_mask"))


def test_no_targets_no_launch(C, monkeypatch):
    """Case H: every image without targets.  Exact zeros with a zero gradient to pred_masks, and no mask kernel is launched."""
    from uenc import kernels as K
    inp, ref = build("H"), ref64("H")

    def never(*a, **k):
        raise AssertionError("a mask kernel was launched for a batch without pairs")
    for fn in ("crit_point_logits", "crit_mask_loss_fwd", "crit_mask_loss_bwd"):
        monkeypatch.setattr(K, fn, never)
    P, over, imp = CASES["H"][6:9]
    crit = criterion(C, inp["num_classes"], P, over, imp, coef_dict(inp)).cuda()
    out_g, hs = leaves(inp["heads"], "cuda")
    tg_g = [{k: v.cuda() for k, v in t.items()} for t in inp["targets"]]
    losses = crit(out_g, tg_g)
    crit.weighted_sum(losses).backward()
    for i, (hd, r) in enumerate(zip(hs, ref)):
        sfx = "" if i == 0 else f"_{i - 1}"
        assert float(losses["loss_mask" + sfx]) == 0.0 and float(losses["loss_dice" + sfx]) == 0.0
        assert hd["pred_masks"].grad is not None and not hd["pred_masks"].grad.any()
        assert abs(float(losses["loss_ce" + sfx]) - r["loss_ce"]) <= REL_L2 * abs(r["loss_ce"])
        assert rel_l2(hd["pred_logits"].grad, r["g_logits"]) <= REL_L2


def test_matcher_criterion_backward_in_one_capture(C):
    """match_all(solver="device"), the criterion and backward() recorded in one torch.cuda.graph (a capture raises on any
    synchronisation) with injected draws and static buffers, replayed on two further input sets: every replay equals eager."""
    bs, Q, C1, (h, w), (H, W), Ts, P, over, imp, n_heads, _ = CASES["B"]
    Ts = (3, 4)
    M, n_unc, n_rnd = counts("B")
    N = sum(min(Q, T) for T in Ts)
    weights = coef_dict(build("B"))
    crit = criterion(C, C1 - 1, P, over, imp, weights).cuda()

    def inputs(k):
        g = torch.Generator().manual_seed(200 + k)
        hs = [{"pred_logits": torch.randn(bs, Q, C1, generator=g).cuda(), "pred_masks": (torch.randn(bs, Q, h, w, generator=g) * 3).cuda()}
              for _ in range(n_heads)]
        tg = [{"labels": torch.randint(0, C1 - 1, (T,), generator=g).cuda(), "masks": (torch.rand(T, H, W, generator=g) > 0.6).cuda()} for T in Ts]
        return hs, tg, torch.rand(n_heads, bs, P, 2, generator=g).cuda(), torch.rand(n_heads, N, M, 2, generator=g).cuda(), \
            torch.rand(n_heads, N, n_rnd, 2, generator=g).cuda()

    def step(hs, tg, mpts, ov, rnd):
        """-> losses (stacked, in key order) and the gradients of every head; the leaves' .grad is reset first."""
        for hd in hs:
            for v in hd.values():
                v.requires_grad_(True)
                v.grad = None
        outputs = dict(hs[0], aux_outputs=hs[1:])
        indices = crit.matcher.match_all(outputs, tg, point_coords=mpts, solver="device")
        losses = crit(outputs, tg, indices=indices, point_draws={"oversampled": ov, "random": rnd})
        crit.weighted_sum(losses).backward()
        return torch.stack([losses[k] for k in sorted(losses)]).detach(), [v.grad for hd in hs for v in hd.values()]

    data = [inputs(k) for k in range(3)]
    eager = []
    for d in data:
        lo, gr = step(*d)
        eager.append((lo.clone(), [g.clone() for g in gr]))
    torch.cuda.synchronize()

    static = [[{k: v.detach().clone() for k, v in hd.items()} for hd in data[0][0]], [{k: v.clone() for k, v in t.items()} for t in data[0][1]]] + \
        [x.clone() for x in data[0][2:]]

    def load(k):
        hs, tg, mpts, ov, rnd = data[k]
        with torch.no_grad():
            for dst, src in zip(static[0], hs):
                for key in dst:
                    dst[key].copy_(src[key])
            for dst, src in zip(static[1], tg):
                for key in dst:
                    dst[key].copy_(src[key])
            for dst, src in zip(static[2:], (mpts, ov, rnd)):
                dst.copy_(src)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_losses, cap_grads = step(*static)
    worst = 0.0
    for k in (0, 1, 2):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(cap_losses, eager[k][0]), k
        for a, b in zip(cap_grads, eager[k][1]):
            assert torch.equal(a, b), k
        worst = max(worst, float((cap_losses - eager[k][0]).abs().max()))
    assert not torch.equal(eager[0][0], eager[1][0])
    record_parity("criterion_capture", heads=n_heads, replays=3, losses=int(cap_losses.numel()), gradients=len(cap_grads), max_abs_vs_eager=worst)
