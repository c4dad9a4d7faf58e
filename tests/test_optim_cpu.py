"""uenc.optim without a GPU: the parameter-group policy of `build_optimizer` on the CPU-built models, the CPU path of FusedAdamW against
the reference's composition (nan_to_num -> clip_grad_norm_ -> torch.optim.AdamW) run by torch in float64, and state_dict interchange
with torch.optim.AdamW in both directions."""
import copy

import pytest
import torch

SWIN = ["MODEL.BACKBONE.NAME", "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM", 64, "MODEL.SWIN.DEPTHS", [2, 2, 2, 2],
        "MODEL.SWIN.NUM_HEADS", [2, 4, 8, 16]]
DINAT = ["MODEL.BACKBONE.NAME", "D2DiNAT", "MODEL.DiNAT.EMBED_DIM", 64, "MODEL.DiNAT.MLP_RATIO", 2.0, "MODEL.DiNAT.DEPTHS", [2, 2, 2, 1],
         "MODEL.DiNAT.NUM_HEADS", [2, 4, 8, 16], "MODEL.DiNAT.KERNEL_SIZE", 3, "MODEL.DiNAT.DILATIONS", [[1, 2], [1, 2], [1, 1], [1]]]
# non-default values so that every branch of the policy and the precedence between them show
SOLVER = ["SOLVER.BASE_LR", 1e-4, "SOLVER.WEIGHT_DECAY", 0.05, "SOLVER.WEIGHT_DECAY_NORM", 0.02, "SOLVER.WEIGHT_DECAY_EMBED", 0.03,
          "SOLVER.BACKBONE_MULTIPLIER", 0.25, "SOLVER.OPTIMIZER", "ADAMW", "SOLVER.CLIP_GRADIENTS.ENABLED", True,
          "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.01]


def _cfg(backbone, extra=()):
    import model  # noqa: F401
    from uenc.config import add_common_config, add_dinat_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_dinat_config(cfg); add_uni_encoder_config(cfg)
    cfg.SOLVER.WEIGHT_DECAY_NORM = 0.0          # Detectron2's default for the key the reference reads
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", *backbone, "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 1, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 20, "MODEL.ONE_FORMER.DEC_LAYERS", 3, "MODEL.DEVICE", "cpu", *SOLVER, *extra])
    return cfg


_NORMS = (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d, torch.nn.BatchNorm3d, torch.nn.SyncBatchNorm, torch.nn.GroupNorm, torch.nn.InstanceNorm1d,
          torch.nn.InstanceNorm2d, torch.nn.InstanceNorm3d, torch.nn.LayerNorm, torch.nn.LocalResponseNorm)


def _policy(model):
    """{parameter id: (full name, lr, weight decay)} by the reference's rules, spelled out: the checks in the reference's order, a
    later one overriding an earlier one; a shared tensor is taken where named_modules() meets it first."""
    want = {}
    for mname, mod in model.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in want:
                continue
            lr = 1e-4 * 0.25 if "backbone" in mname else 1e-4
            wd = 0.05
            if "relative_position_bias_table" in pname or "absolute_pos_embed" in pname:
                wd = 0.0
            if isinstance(mod, _NORMS):
                wd = 0.02
            if isinstance(mod, torch.nn.Embedding):
                wd = 0.03
            want[id(p)] = (f"{mname}.{pname}", lr, wd)
    return want


@pytest.mark.parametrize("backbone", ["swin", "dinat"])
def test_build_optimizer_groups(backbone):
    from uenc.d2 import build_model
    from uenc.optim import FusedAdamW, build_optimizer
    cfg = _cfg(SWIN if backbone == "swin" else DINAT)
    m = build_model(cfg)
    opt = build_optimizer(cfg, m)
    assert isinstance(opt, FusedAdamW) and opt.max_grad_norm == 0.01
    want = _policy(m)
    seen = {}
    for g in opt.param_groups:
        assert len(g["params"]) == 1                         # one group per tensor
        p = g["params"][0]
        assert id(p) not in seen
        seen[id(p)] = (g["lr"], g["weight_decay"])
        assert g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
    trainable = {id(p) for p in m.parameters() if p.requires_grad}
    assert set(seen) == trainable == set(want)               # every trainable parameter exactly once
    for i, (name, lr, wd) in want.items():
        assert seen[i] == pytest.approx((lr, wd), rel=1e-12), name
    # the visible cases, by name
    by_name = {name: seen[i] for i, (name, _, _) in want.items()}

    def one(pred):
        hits = [v for k, v in by_name.items() if pred(k)]
        assert hits, "no such parameter"
        assert all(h == pytest.approx(hits[0]) for h in hits)
        return hits[0]
    mods = dict(m.named_modules())
    bb_norm = next(k for k in by_name if k.startswith("backbone") and isinstance(mods[k.rsplit(".", 1)[0]], torch.nn.LayerNorm))
    assert by_name[bb_norm] == pytest.approx((2.5e-5, 0.02))                 # backbone lr, norm decay
    bb_lin = next(k for k in by_name if k.startswith("backbone") and isinstance(mods[k.rsplit(".", 1)[0]], torch.nn.Linear)
                  and k.endswith("weight"))
    assert by_name[bb_lin] == pytest.approx((2.5e-5, 0.05))
    if backbone == "swin":
        assert one(lambda k: k.endswith("relative_position_bias_table")) == pytest.approx((2.5e-5, 0.0))
    emb = [k for k in by_name if isinstance(mods[k.rsplit(".", 1)[0]], torch.nn.Embedding)]
    assert any("query_embed" in k for k in emb)
    for k in emb:
        assert by_name[k] == pytest.approx((2.5e-5 if "backbone" in k else 1e-4, 0.03)), k
    dec_lin = next(k for k in by_name if "predictor" in k and isinstance(mods[k.rsplit(".", 1)[0]], torch.nn.Linear) and k.endswith("weight"))
    assert by_name[dec_lin] == pytest.approx((1e-4, 0.05))
    dec_norm = next(k for k in by_name if "predictor" in k and isinstance(mods[k.rsplit(".", 1)[0]], torch.nn.LayerNorm))
    assert by_name[dec_norm] == pytest.approx((1e-4, 0.02))


def test_norm_overrides_position_table_and_embedding_overrides_norm():
    """The precedence itself, on modules built for it: the name rule (decay 0) loses to the normalisation rule, which loses to the
    Embedding rule."""
    from uenc.optim import param_groups

    class NormWithTable(torch.nn.LayerNorm):
        def __init__(self):
            super().__init__(4)
            self.relative_position_bias_table = torch.nn.Parameter(torch.zeros(3))

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.backbone = torch.nn.ModuleDict({"n": NormWithTable(), "e": torch.nn.Embedding(3, 4)})
            self.head = torch.nn.Linear(4, 4)
            self.absolute_pos_embed = torch.nn.Parameter(torch.zeros(2))
            self.frozen = torch.nn.Parameter(torch.zeros(2), requires_grad=False)
            self.tied = self.head                       # the same tensors under a second name: taken once
    net = Net()
    got = {id(g["params"][0]): (g["lr"], g["weight_decay"]) for g in param_groups(_cfg(SWIN), net)}
    assert len(got) == 3 + 1 + 2 + 1
    assert got[id(net.backbone["n"].relative_position_bias_table)] == pytest.approx((2.5e-5, 0.02))
    assert got[id(net.backbone["n"].weight)] == pytest.approx((2.5e-5, 0.02))
    assert got[id(net.backbone["e"].weight)] == pytest.approx((2.5e-5, 0.03))
    assert got[id(net.head.weight)] == pytest.approx((1e-4, 0.05))
    assert got[id(net.absolute_pos_embed)] == pytest.approx((1e-4, 0.0))
    assert id(net.frozen) not in got


def test_unsupported_solver_keys_raise():
    from uenc.optim import build_optimizer
    net = torch.nn.Linear(3, 3)
    with pytest.raises(NotImplementedError, match="SOLVER.OPTIMIZER"):
        build_optimizer(_cfg(SWIN, ["SOLVER.OPTIMIZER", "SGD"]), net)
    with pytest.raises(NotImplementedError, match="SOLVER.OPTIMIZER"):
        build_optimizer(_cfg(SWIN, ["SOLVER.OPTIMIZER", "LAMB"]), net)
    for kind in ("value", "norm"):
        with pytest.raises(NotImplementedError, match="CLIP_TYPE"):
            build_optimizer(_cfg(SWIN, ["SOLVER.CLIP_GRADIENTS.CLIP_TYPE", kind]), net)
    assert build_optimizer(_cfg(SWIN, ["SOLVER.CLIP_GRADIENTS.ENABLED", False, "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "value"]), net).max_grad_norm is None
    assert build_optimizer(_cfg(SWIN, ["SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.0]), net).max_grad_norm is None


# ---- the step ---------------------------------------------------------------------------------------------------------------------
SIZES = [(1,), (3,), (7, 11), (255,), (40, 33)]


def _params(dtype):
    g = torch.Generator().manual_seed(1)
    return [torch.nn.Parameter((torch.randn(s, generator=g, dtype=torch.float64) * 0.02).float().to(dtype)) for s in SIZES] + \
        [torch.nn.Parameter(torch.ones(5, dtype=dtype))]            # never receives a gradient


def _grads(step):
    g = torch.Generator().manual_seed(100 + step)
    out = [(torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-5, 1, (1,), generator=g))).float() for s in SIZES]
    out[2][0, 1], out[3][5], out[4][3, 3] = float("nan"), float("inf"), -float("inf")
    return out


def _groups(ps, lr_scale=1.0):
    return [{"params": ps[:2], "lr": 1e-3 * lr_scale, "weight_decay": 0.05}, {"params": ps[2:], "lr": 1e-4 * lr_scale, "weight_decay": 0.0}]


def oracle_step(ps, opt, grads, max_norm):
    """The reference's composition, by torch, on float64 copies."""
    for p, g in zip(ps, grads):
        p.grad = g.to(p.dtype).clone()
    live = [p for p in ps if p.grad is not None]
    for p in live:
        torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)
    norm = torch.nn.utils.clip_grad_norm_(live, max_norm) if max_norm is not None else None
    opt.step()
    return norm


@pytest.mark.parametrize("max_norm", [0.01, 1e9, None])
def test_cpu_path_matches_the_float64_oracle(max_norm):
    from uenc.optim import FusedAdamW
    mine, ref = _params(torch.float32), _params(torch.float64)
    opt = FusedAdamW(_groups(mine), max_grad_norm=max_norm)
    ropt = torch.optim.AdamW(_groups(ref))
    for s in range(4):
        gs = _grads(s)
        for p, g in zip(mine, gs):
            p.grad = g.clone()
        for o in (opt, ropt):
            for grp in o.param_groups:
                grp["lr"] *= 0.9
        opt.step()
        oracle_step(ref, ropt, gs, max_norm)
        for p, g in zip(mine, gs):                                 # the raw gradients are left as they were
            assert torch.equal(torch.nan_to_num(p.grad, nan=7.0), torch.nan_to_num(g, nan=7.0))
    assert mine[-1].grad is None and len(opt.state.get(mine[-1], {})) == 0 and torch.equal(mine[-1].detach(), torch.ones(5))
    for a, b in zip(mine, ref):
        assert float((a.detach().double() - b.detach()).abs().max()) < 2e-7
    for a, b in zip(mine[:-1], ref[:-1]):
        for k in ("exp_avg", "exp_avg_sq"):
            r = ropt.state[b][k]
            assert float((opt.state[a][k].double() - r).abs().max()) <= 1e-6 * float(r.abs().max())
        assert float(opt.state[a]["step"]) == 4


def test_state_dict_round_trip_with_torch_adamw():
    from uenc.optim import FusedAdamW
    a, b = _params(torch.float32), _params(torch.float32)
    fa, tb = FusedAdamW(_groups(a)), torch.optim.AdamW(_groups(b))
    for s in range(2):
        for ps in (a, b):
            for p, g in zip(ps, _grads(s)):
                p.grad = torch.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5)
        fa.step(); tb.step()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # ours -> torch
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    tc = torch.optim.AdamW(_groups(c))
    tc.load_state_dict(copy.deepcopy(fa.state_dict()))
    assert tc.param_groups[0].get("decoupled_weight_decay", True) and float(tc.state[c[0]]["step"]) == 2
    # torch -> ours
    d = [torch.nn.Parameter(p.detach().clone()) for p in b]
    fd = FusedAdamW(_groups(d))
    fd.load_state_dict(tb.state_dict())
    gs = [torch.nan_to_num(g, nan=0.0, posinf=1e5, neginf=-1e5) for g in _grads(2)]
    for ps in (a, b, c, d):
        for p, g in zip(ps, gs):
            p.grad = g.clone()
    for o in (fa, tb, tc, fd):
        o.step()
    for w, x, y, z in zip(a, b, c, d):
        assert torch.equal(w, x) and torch.equal(w, y) and torch.equal(w, z)
    assert float(tb.state[b[0]]["step"]) == 3 and float(fd.state[d[0]]["step"]) == 3      # loading did not tie the two optimizers together
    assert float(tc.state[c[0]]["step"]) == 3 and float(fa.state[a[0]]["step"]) == 3


def test_zero_grad_keeps_the_buffers():
    from uenc.optim import FusedAdamW
    ps = _params(torch.float32)
    for p, g in zip(ps, _grads(0)):
        p.grad = g
    bufs = [p.grad for p in ps[:-1]]
    FusedAdamW(_groups(ps)).zero_grad()
    assert all(p.grad is b and float(b.abs().sum()) == 0 for p, b in zip(ps, bufs))
