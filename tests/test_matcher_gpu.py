"""uenc_match_cost / uenc_lsap_solve (csrc/matcher.hip) and HungarianMatcher on the GPU, against the reference's own results
(tests/golden/matcher.npz), a float64 restatement and scipy."""
import numpy as np
import pytest
import torch

from conftest import record_parity
from matcher_fixture import STABLE_AMPLITUDE, calls, check_assignment, load_problems, rel_l2

pytestmark = pytest.mark.gpu

COST_REL_L2 = 1e-4              # the project's bar for fp32 kernels
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def M():
    import model  # noqa: F401  loads libuenc_hip.so
    import uenc.modeling.matcher as m
    return m


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module")
def problems():
    return load_problems()


def _cuda(outputs, targets, points):
    o = {k: v.cuda() for k, v in outputs.items()}
    t = [{k: v.cuda() for k, v in tg.items()} for tg in targets]
    return o, t, points.cuda()


def _matcher(M, pr, **kw):
    w = pr["weights"]
    return M.HungarianMatcher(cost_class=w[0], cost_mask=w[1], cost_dice=w[2], num_points=pr["num_points"], **kw)


@pytest.fixture(scope="module")
def measured(M, problems):
    """Per problem: the kernel's cost matrix (twice), its errors against the reference's matrix, and both solvers' indices."""
    out = {}
    for outputs, targets, points, ps in calls(problems):
        o, t, p = _cuda(outputs, targets, points)
        m = _matcher(M, ps[0])
        c1 = [c.cpu().numpy() for c in m.cost_matrices(o, t, point_coords=p)]
        c2 = [c.cpu().numpy() for c in m.cost_matrices(o, t, point_coords=p)]
        dev = m(o, t, point_coords=p, solver="device")
        host = m(o, t, point_coords=p, solver="host")
        torch.cuda.synchronize()
        for b, pr in enumerate(ps):
            ent = {"cost": c1[b], "again": c2[b], "device": dev[b], "host": host[b], "rel": 0.0, "e": 0.0}
            if c1[b].size:
                ent["rel"] = rel_l2(c1[b], pr["cost"])
                ent["e"] = float(np.abs(c1[b].astype(np.float64) - pr["cost"]).max())
            out[pr["index"]] = ent
    return out


def test_cost_matches_reference(problems, measured):
    for pr in problems:
        ent = measured[pr["index"]]
        print(f"problem {pr['index']}: shape {pr['cost'].shape}  rel L2 {ent['rel']:.3e}  max abs {ent['e']:.3e}")
        record_parity(f"matcher_cost_vs_reference/p{pr['index']}", rel_l2=ent["rel"], max_abs=ent["e"], Q=pr["cost"].shape[0], T=pr["cost"].shape[1],
                      P=pr["num_points"])
    for pr in problems:
        ent = measured[pr["index"]]
        assert ent["cost"].shape == pr["cost"].shape
        assert ent["rel"] <= COST_REL_L2, (pr["index"], ent["rel"])
        assert np.array_equal(ent["cost"], ent["again"]), pr["index"]      # two runs, the same bits


def test_indices_match_reference_both_solvers(problems, measured):
    figs = {}
    for pr in problems:
        ent = measured[pr["index"]]
        for name in ("device", "host"):
            i, j = ent[name]
            assert i.dtype == torch.int64 and j.dtype == torch.int64 and i.is_cuda == (name == "device")
            i, j = i.cpu().numpy(), j.cpu().numpy()
            excess = check_assignment(i, j, pr, ent["e"])
            same = bool(np.array_equal(i, pr["row"]) and np.array_equal(j, pr["col"]))
            figs[f"p{pr['index']}_{name}"] = {"excess": excess, "identical": same}
            print(f"problem {pr['index']} {name}: identical {same}  excess over the reference's total {excess:.3e}")
            if pr["stable"] and ent["e"] < STABLE_AMPLITUDE / 2:
                assert same, (pr["index"], name)
    record_parity("matcher_indices_vs_reference", **figs)


def test_nan_problem_device_equals_host(problems, measured):
    nan = [pr for pr in problems if np.isnan(pr["cost_raw"]).any()]
    assert nan
    for pr in nan:
        ent = measured[pr["index"]]
        assert (ent["cost"] == 100.0).sum() == np.isnan(pr["cost_raw"]).sum()
        for a, b in zip(ent["device"], ent["host"]):
            assert torch.equal(a.cpu(), b)


def _cost64(logits, masks, gt, labels, pts, w):
    """The matching cost in float64 torch (grid_sample, softplus, einsum)."""
    F = torch.nn.functional
    lg, x, t, pc = logits.double(), masks.double()[:, None], gt.double()[:, None], pts.double()[None]
    grid = (2 * pc - 1)[:, :, None]
    xs = F.grid_sample(x, grid.expand(x.shape[0], -1, -1, -1), align_corners=False)[:, 0, :, 0]
    ts = F.grid_sample(t, grid.expand(t.shape[0], -1, -1, -1), align_corners=False)[:, 0, :, 0]
    P = pts.shape[0]
    cm = (F.softplus(-xs) @ ts.T + F.softplus(xs) @ (1 - ts).T) / P
    s = xs.sigmoid()
    cd = 1 - (2 * s @ ts.T + 1) / (s.sum(-1)[:, None] + ts.sum(-1)[None] + 1)
    cc = -lg.softmax(-1)[:, labels]
    return w[1] * cm + w[0] * cc + w[2] * cd


@pytest.mark.parametrize("Q,C1,h,w,Hg,Wg,P,Ts", [(37, 7, 13, 21, 50, 83, 777, (5, 0, 19)), (150, 134, 16, 24, 64, 96, 1001, (3, 66)),
                                                 (256, 20, 9, 7, 33, 29, 65, (256, 100)), (1, 3, 5, 5, 5, 5, 1, (2, 1))])
def test_cost_against_float64(K, Q, C1, h, w, Hg, Wg, P, Ts):
    g = torch.Generator().manual_seed(Q * 1000 + P)
    wts = (2.0, 5.0, 5.0)
    probs, refs = [], []
    for T in Ts:
        logits, masks = torch.randn(Q, C1, generator=g), torch.randn(Q, h, w, generator=g) * 3
        gt = (torch.rand(T, Hg, Wg, generator=g) > 0.5).to(torch.uint8)
        labels = torch.randint(0, C1, (T,), generator=g)
        pts = torch.rand(P, 2, generator=g)
        pts[0] = torch.tensor([0.0, 0.0])                # the corners: three of the four taps fall outside the map
        pts[-1] = torch.tensor([1.0, 1.0])
        if P > 4:
            pts[1], pts[2] = torch.tensor([1.0, 0.0]), torch.tensor([0.3, 1.0])
        probs.append(tuple(a.cuda() for a in (logits, masks, pts, gt, labels)))
        refs.append(_cost64(logits, masks, gt, labels, pts, wts).numpy())
    a = K.match_cost(probs, *wts).cpu().numpy()
    b = K.match_cost(probs, *wts).cpu().numpy()
    assert a.shape == (len(Ts), Q, max(Ts)) and np.array_equal(a, b)
    worst = 0.0
    for p, T in enumerate(Ts):
        assert (a[p, :, T:] == 0).all()                  # columns beyond a problem's T are written as zero
        if T:
            worst = max(worst, rel_l2(a[p, :, :T], refs[p]))
    print(f"Q {Q} P {P} Ts {Ts}: worst rel L2 against float64 {worst:.3e}")
    record_parity(f"matcher_cost_vs_float64/Q{Q}_P{P}", rel_l2=worst)
    assert worst <= COST_REL_L2


def _scipy(c):
    from scipy.optimize import linear_sum_assignment
    return linear_sum_assignment(c)


def _solve(K, mats):
    """Matrices of one Q (any T) in one launch -> [(row, col)] as numpy."""
    Q, ld = mats[0].shape[0], max(1, max(m.shape[1] for m in mats))
    cost = torch.zeros(len(mats), Q, ld)
    for p, m in enumerate(mats):
        cost[p, :, :m.shape[1]] = torch.from_numpy(m)
    rows, cols, offs = K.lsap_solve(cost.cuda(), [m.shape[1] for m in mats])
    rows, cols = rows.cpu().numpy(), cols.cpu().numpy()
    return [(rows[offs[p]:offs[p + 1]], cols[offs[p]:offs[p + 1]]) for p in range(len(mats))]


def test_lsap_random_matrices_against_scipy(K):
    rs = np.random.RandomState(0)
    shapes = [(1, 1), (256, 256), (256, 1), (1, 256), (150, 60), (60, 150), (255, 256), (256, 255), (64, 64), (65, 63)]
    while len(shapes) < 200:
        shapes.append((int(rs.randint(1, 257)), int(rs.randint(1, 257))))
    identical, worst = 0, 0.0
    for Q, T in shapes:
        c = (rs.standard_normal((Q, T)) * rs.choice([0.1, 1.0, 30.0])).astype(np.float32)
        (i, j), = _solve(K, [c])
        i2, j2 = _scipy(c.astype(np.float64))
        n = min(Q, T)
        assert i.shape == (n,) and (np.diff(i) > 0).all() and len(set(j.tolist())) == n and j.min() >= 0 and j.max() < T and i.max() < Q
        tot, ref = c.astype(np.float64)[i, j].sum(), c.astype(np.float64)[i2, j2].sum()
        worst = max(worst, float(tot - ref))
        assert abs(tot - ref) <= 16 * EPS32 * n * float(np.abs(c).max()), (Q, T, tot, ref)
        identical += bool(np.array_equal(i, i2) and np.array_equal(j, j2))
    print(f"lsap vs scipy: {identical} of {len(shapes)} identical, largest excess of the total {worst:.3e}")
    record_parity("matcher_lsap_vs_scipy", identical_share=identical / len(shapes), largest_excess=worst, problems=len(shapes))
    assert identical == len(shapes)


def test_lsap_ties_constant_and_special_columns(K):
    rs = np.random.RandomState(1)
    for Q, T in [(40, 40), (150, 20), (20, 150), (256, 256), (7, 3)]:
        c = rs.randint(0, 4, (Q, T)).astype(np.float32)                                  # full of ties: totals equal, indices may differ
        (i, j), = _solve(K, [c])
        i2, j2 = _scipy(c.astype(np.float64))
        assert len(set(j.tolist())) == min(Q, T) and (np.diff(i) > 0).all()
        assert c[i, j].astype(np.float64).sum() == c[i2, j2].astype(np.float64).sum()
    const = np.full((30, 12), 2.5, dtype=np.float32)
    hundred = rs.standard_normal((25, 9)).astype(np.float32)
    hundred[:, 4] = 100.0
    mixed = [rs.standard_normal((30, T)).astype(np.float32) for T in (0, 1, 30, 45)]     # different T (also 0) in one launch
    for mats in ([const], [hundred], mixed):
        for c, (i, j) in zip(mats, _solve(K, mats)):
            n = min(c.shape)
            assert i.shape == (n,) and j.shape == (n,)
            if n:
                i2, j2 = _scipy(c.astype(np.float64))
                assert len(set(j.tolist())) == n and (np.diff(i) > 0).all() if n > 1 else True
                assert abs(c.astype(np.float64)[i, j].sum() - c.astype(np.float64)[i2, j2].sum()) <= 16 * EPS32 * n * float(np.abs(c).max())
    (i, j), = _solve(K, [hundred])
    assert 4 in j.tolist()                               # 25 rows, 9 columns: the dear column is still assigned


def test_argument_rejection(K):
    import ctypes
    from uenc import capi
    c = torch.zeros(1, 4, 4)
    with pytest.raises(capi.UencError):
        K.lsap_solve(c, [4])                             # CPU tensor
    with pytest.raises(capi.UencError):
        K.lsap_solve(torch.zeros(1, 257, 4).cuda(), [4])
    with pytest.raises(capi.UencError):
        K.lsap_solve(torch.zeros(1, 4, 300).cuda(), [257])
    with pytest.raises(capi.UencError):
        K.lsap_solve(torch.zeros(1, 4, 4).cuda(), [5])   # T beyond the row stride
    lib = capi.lib
    assert lib.uenc_lsap_solve(None, 1, 4, None) == -1
    _, lp = K._match_dtypes()
    row = np.zeros(1, dtype=lp)
    row[0] = (0, 0, 0, 4, 4)                             # null matrix / result pointers
    assert lib.uenc_lsap_solve(row.ctypes.data, 1, 4, None) == -1
    row[0] = (256, 256, 256, 300, 300)
    assert lib.uenc_lsap_solve(row.ctypes.data, 1, 4, None) == -1
    assert lib.uenc_match_cost(None, 1, 4, 4, 4, 4, 4, 4, 4, 4, 1.0, 1.0, 1.0, 100.0, None, 0, None, None) == -1
    assert lib.uenc_match_cost_workspace_floats(1, 257, 4, 16) == -1 and lib.uenc_match_cost_workspace_floats(1, 4, 257, 16) == -1
    g = torch.Generator().manual_seed(0)
    prob = (torch.randn(4, 3, generator=g), torch.randn(4, 5, 5, generator=g), torch.rand(8, 2, generator=g),
            torch.ones(2, 20, 20, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(capi.UencError):
        K.match_cost([prob], 1.0, 1.0, 1.0)              # CPU tensors
    torch.cuda.synchronize()


def _small_model_outputs(seeds):
    """pred_logits / pred_masks / aux_outputs of the small OneFormer (the model of smoke()) for one batch per seed."""
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
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    fill.fill_module(m)
    m.eval()
    outs = []
    for seed in seeds:
        g = torch.Generator().manual_seed(seed)
        imgs = torch.randint(0, 256, (2, 3, 64, 96), generator=g).float().cuda()
        batch = [{"left_image": imgs[i], "task": "The task is panoptic", "type": "segmentation"} for i in range(2)]
        with torch.no_grad():
            out, _ = m.forward_features(batch)
        heads = [out] + list(out.get("aux_outputs", []))
        outs.append([{"pred_logits": h["pred_logits"].detach().float().clone(), "pred_masks": h["pred_masks"].detach().float().clone()} for h in heads])
    torch.cuda.synchronize()
    return outs


def test_device_path_is_capturable(M):
    """match_all(solver="device") recorded in a stream capture (which raises on any synchronisation), replayed on two further sets of
    predictions / targets / points copied into the static buffers: every replay equals the eager result."""
    sets = _small_model_outputs([0, 1, 2])
    n_heads, Ts, P = len(sets[0]), (7, 23), 112 * 4
    Hg, Wg = 64, 96
    matcher = M.HungarianMatcher(2.0, 5.0, 5.0, num_points=P)

    def inputs(k):
        g = torch.Generator().manual_seed(100 + k)
        tg = [{"labels": torch.randint(0, 19, (T,), generator=g).cuda(), "masks": (torch.rand(T, Hg, Wg, generator=g) > 0.7).cuda()} for T in Ts]
        return tg, torch.rand(n_heads, 2, P, 2, generator=g).cuda()

    def as_outputs(heads):
        return dict(heads[0], aux_outputs=heads[1:])

    def flat(res):
        return [x.clone() for head in res for pair in head for x in pair]

    data = [(sets[k],) + inputs(k) for k in range(3)]
    eager = [flat(matcher.match_all(as_outputs(h), tg, point_coords=pts, solver="device")) for h, tg, pts in data]
    torch.cuda.synchronize()

    s_heads = [{k: v.clone() for k, v in h.items()} for h in data[0][0]]
    s_tg = [{k: v.clone() for k, v in t.items()} for t in data[0][1]]
    s_pts = data[0][2].clone()

    def load(k):
        h, tg, pts = data[k]
        for dst, src in zip(s_heads, h):
            for key in dst:
                dst[key].copy_(src[key])
        for dst, src in zip(s_tg, tg):
            for key in dst:
                dst[key].copy_(src[key])
        s_pts.copy_(pts)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        matcher.match_all(as_outputs(s_heads), s_tg, point_coords=s_pts, solver="device")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = matcher.match_all(as_outputs(s_heads), s_tg, point_coords=s_pts, solver="device")
    for k in (0, 1, 2):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        got = flat(captured)
        assert len(got) == len(eager[k]) == n_heads * 2 * 2
        for a, b in zip(got, eager[k]):
            assert torch.equal(a, b), k
    differ = sum(not torch.equal(a, b) for a, b in zip(eager[0], eager[1]))
    assert differ > 0                                    # the sets do ask for different assignments
    record_parity("matcher_capture", heads=n_heads, replays=3, results_compared=len(eager[0]), differing_between_sets=differ)
