"""uenc.optim on the GPU: the HIP kernels of csrc/optim.hip behind FusedAdamW against the reference's own composition --
torch.nan_to_num -> torch.nn.utils.clip_grad_norm_ -> torch.optim.AdamW -- run by torch on the CPU in float64 on copies of the same
parameters, gradients and state.

Tolerance, everywhere: torch's own fp32 composition runs on the GPU on the same inputs in the same test; its error against the float64
oracle is the yardstick and ours may be at most twice that, per quantity (parameters: max absolute error; each moment and the norm:
max error relative to the oracle's largest magnitude in that tensor).  The factor covers another summation order in the norm and
fused-multiply-add contraction, nothing more.

Measured on an MI355X (test_kernel_parity, five steps; ours / torch fp32): see DESIGN.md section 6 "Optimizer"."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import record_parity

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture
def U():
    from uenc import ops
    ops.CACHE.invalidate()
    yield
    ops.CACHE.invalidate()


# ---- the oracle: torch's composition, any dtype / device ------------------------------------------------------------------------------
class TorchComposition:
    """nan_to_num -> clip_grad_norm_ -> torch.optim.AdamW over copies of the given tensors (None gradient = skipped parameter)."""

    def __init__(self, params, groups, max_norm, dtype, device, state=None):
        """groups: [(indices, lr, weight_decay)]; state: optional {index: (exp_avg, exp_avg_sq, step)} to start from."""
        self.ps = [torch.nn.Parameter(p.detach().to(device=device, dtype=dtype).clone()) for p in params]
        self.opt = torch.optim.AdamW([{"params": [self.ps[i] for i in idx], "lr": lr, "weight_decay": wd} for idx, lr, wd in groups])
        self.max_norm, self.dtype, self.device = max_norm, dtype, device
        for i, (m, v, t) in (state or {}).items():
            self.opt.state[self.ps[i]] = {"step": torch.tensor(float(t), dtype=torch.float32),
                                          "exp_avg": m.detach().to(device=device, dtype=dtype).clone(),
                                          "exp_avg_sq": v.detach().to(device=device, dtype=dtype).clone()}

    def step(self, grads):
        for p, g in zip(self.ps, grads):
            p.grad = None if g is None else g.detach().to(device=self.device, dtype=self.dtype).clone()
        live = [p for p in self.ps if p.grad is not None]
        for p in live:
            torch.nan_to_num(p.grad, nan=0.0, posinf=1e5, neginf=-1e5, out=p.grad)
        norm = torch.nn.utils.clip_grad_norm_(live, self.max_norm) if self.max_norm is not None else None
        self.opt.step()
        return None if norm is None else float(norm.double())

    def moment(self, i, key):
        return self.opt.state[self.ps[i]][key]


def _errors(ps, moments, ref: TorchComposition, live):
    """(parameter max abs error, exp_avg max relative-to-largest error, exp_avg_sq likewise) against the float64 oracle `ref`."""
    ep = max(float((ps[i].detach().double().cpu() - ref.ps[i].detach()).abs().max()) for i in range(len(ps)))
    em = ev = 0.0
    for i in live:
        for key, slot in (("exp_avg", 0), ("exp_avg_sq", 1)):
            r = ref.moment(i, key)
            e = float((moments[i][slot].detach().double().cpu() - r).abs().max()) / max(float(r.abs().max()), 1e-300)
            if slot == 0:
                em = max(em, e)
            else:
                ev = max(ev, e)
    return ep, em, ev


def _assert_within_twice(test, ours, torch32, names):
    figs = {}
    for n, a, b in zip(names, ours, torch32):
        figs[f"{n}_ours"], figs[f"{n}_torch_fp32"] = a, b
    record_parity(test, **figs)
    print(test, figs)
    for n, a, b in zip(names, ours, torch32):
        assert a <= 2.0 * b, (n, a, b)


# ---- 1. kernel parity -------------------------------------------------------------------------------------------------------------------
SHAPES = [(1,), (3,), (77,), (255,), (20, 256), (1000003,), (1536, 3072), (9,)]      # the last one never receives a gradient
GROUPS = [([0, 1, 2], 1e-4, 0.05), ([3, 4, 5, 6, 7], 1e-5, 0.0)]


def _init_values():
    g = torch.Generator().manual_seed(1)
    return [(torch.randn(s, generator=g, dtype=torch.float64) * 0.02).float() for s in SHAPES]


def _step_grads(step):
    g = torch.Generator().manual_seed(100 + step)
    out = [(torch.randn(s, generator=g, dtype=torch.float64) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))).float() for s in SHAPES[:-1]]
    out[3][5], out[4][0, 7], out[5][9], out[6][3, 11], out[6][1535, 3071] = float("nan"), INF, -INF, float("nan"), INF
    return out + [None]


def _device_tensors(values, layout, salt):
    """The values as separate CUDA tensors, or as views at odd element offsets of one flat buffer (a different misalignment each)."""
    if layout == "separate":
        return [v.cuda() for v in values]
    offs, off = [], 1 + salt
    for k, v in enumerate(values):
        offs.append(off)
        off += v.numel() + 1 + (k + salt) % 3
    flat = torch.zeros(off, dtype=torch.float32, device="cuda")
    views = []
    for v, o in zip(values, offs):
        views.append(flat[o:o + v.numel()].view(v.shape))
        views[-1].copy_(v)
    return views


def _fused(params, max_norm, groups=GROUPS):
    from uenc.optim import FusedAdamW
    return FusedAdamW([{"params": [params[i] for i in idx], "lr": lr, "weight_decay": wd} for idx, lr, wd in groups], max_grad_norm=max_norm)


@pytest.mark.parametrize("layout", ["separate", "flat"])
@pytest.mark.parametrize("max_norm", [0.01, 1e9])
def test_kernel_parity(U, layout, max_norm):
    vals = _init_values()
    ps = [torch.nn.Parameter(t) for t in _device_tensors(vals, layout, 0)]
    gbufs = _device_tensors([torch.zeros(s) for s in SHAPES[:-1]], layout, 1)
    opt = _fused(ps, max_norm)
    ref = TorchComposition(vals, GROUPS, max_norm, torch.float64, "cpu")
    t32 = TorchComposition(vals, GROUPS, max_norm, torch.float32, "cuda")
    live = list(range(len(SHAPES) - 1))
    norm_err = [0.0, 0.0]
    for s in range(5):
        gs = _step_grads(s)
        for p, b, g in zip(ps, gbufs, gs):
            b.copy_(g)
            p.grad = b
        before = [b.clone() for b in gbufs]
        for o in (opt, ref.opt, t32.opt):
            for grp in o.param_groups:
                grp["lr"] *= 0.9
        opt.step()
        n_ref, n_32 = ref.step(gs), t32.step(gs)
        st = opt.device_state()
        assert st["step"] == s + 1
        norm_err = [max(norm_err[0], abs(st["grad_norm"] - n_ref) / n_ref), max(norm_err[1], abs(n_32 - n_ref) / n_ref)]
        want_coef = min(1.0, max_norm / (n_ref + 1e-6))
        assert abs(st["clip_coef"] - want_coef) <= 1e-6 * want_coef and (st["clip_coef"] < 1.0) == (max_norm == 0.01)
        for b, c in zip(gbufs, before):                             # the gradient buffers are only read: bit-identical, NaN / inf included
            assert torch.equal(b.view(torch.int32), c.view(torch.int32))
    assert ps[-1].grad is None and len(opt.state.get(ps[-1], {})) == 0 and torch.equal(ps[-1].detach().cpu(), vals[-1])
    mine = _errors(ps, {i: (opt.state[ps[i]]["exp_avg"], opt.state[ps[i]]["exp_avg_sq"]) for i in live}, ref, live)
    theirs = _errors(t32.ps, {i: (t32.moment(i, "exp_avg"), t32.moment(i, "exp_avg_sq")) for i in live}, ref, live)
    for i in live:
        assert float(opt.state[ps[i]]["step"]) == 5
        assert torch.isfinite(ps[i]).all()
    _assert_within_twice(f"optim_kernel_parity[{layout}-{max_norm}]", mine + (norm_err[0],), theirs + (norm_err[1],),
                         ("param_abs", "exp_avg_rel", "exp_avg_sq_rel", "norm_rel"))


def test_norm_is_reproducible_and_zero_gradients_are_harmless(U):
    vals = _init_values()
    ps = [torch.nn.Parameter(t) for t in _device_tensors(vals, "flat", 2)]
    gs = _step_grads(0)
    for p, g in zip(ps, gs):
        p.grad = None if g is None else g.cuda()
    opt = _fused(ps, 0.01)
    opt.step()
    first = opt._dstate.clone()
    from uenc.capi import check, lib, stream_ptr
    tab, n, tiles = opt._table[:3]
    norms = []
    for _ in range(3):                                              # the norm alone, on the same input: the same bits
        opt._partials.fill_(-1.0)
        check(lib.uenc_optim_grad_sqnorm(tab.data_ptr(), n, tiles, opt._partials.data_ptr(), opt._partials.numel(), opt._dstate.data_ptr(), 0.01,
                                         stream_ptr()))
        norms.append(opt._dstate.clone())
    assert all(torch.equal(x, first) for x in norms)
    # all-zero gradients: norm 0, coefficient 1, nothing becomes NaN
    qs = [torch.nn.Parameter(v.cuda()) for v in vals]
    for q in qs[:-1]:
        q.grad = torch.zeros_like(q)
    zopt = _fused(qs, 0.01)
    zopt.step()
    st = zopt.device_state()
    assert st["grad_norm"] == 0.0 and st["clip_coef"] == 1.0 and st["step"] == 1
    for i, (q, v) in enumerate(zip(qs[:-1], vals)):
        decay = 1 - 1e-4 * 0.05 if i < 3 else 1.0
        assert torch.isfinite(q).all() and torch.allclose(q.detach().cpu(), v * decay, rtol=1e-6, atol=0)
        assert float(zopt.state[q]["exp_avg"].abs().max()) == 0 and float(zopt.state[q]["exp_avg_sq"].abs().max()) == 0


def test_entry_points_reject_bad_arguments():
    """UENC_CHECK_ARG: null table, n <= 0, misaligned state block -> -1, nothing launched."""
    from uenc.capi import lib
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    tab, state, groups, part = buf.data_ptr(), buf.data_ptr() + 1024, buf.data_ptr() + 2048, buf.data_ptr() + 4096
    d, f = ctypes.c_double, ctypes.c_float
    assert lib.uenc_optim_advance(None, d(0.9), d(0.999), None) == -1
    assert lib.uenc_optim_advance(state + 8, d(0.9), d(0.999), None) == -1
    assert lib.uenc_optim_advance(state, d(1.0), d(0.999), None) == -1
    assert lib.uenc_optim_grad_sqnorm(None, 1, 1, part, 2048, state, f(1.0), None) == -1
    assert lib.uenc_optim_grad_sqnorm(tab, 0, 1, part, 2048, state, f(1.0), None) == -1
    assert lib.uenc_optim_grad_sqnorm(tab, 1, 0, part, 2048, state, f(1.0), None) == -1
    assert lib.uenc_optim_grad_sqnorm(tab, 1, 1, None, 2048, state, f(1.0), None) == -1
    assert lib.uenc_optim_grad_sqnorm(tab, 1, 5, part, 4, state, f(1.0), None) == -1           # too few partial slots
    assert lib.uenc_optim_grad_sqnorm(tab, 1, 1, part, 2048, state + 4, f(1.0), None) == -1
    assert lib.uenc_optim_grad_sqnorm(tab, 1, 1, part, 2048, None, f(1.0), None) == -1
    assert lib.uenc_optim_grad_sqnorm(tab, 1, 1, part, 2048, state, f(0.0), None) == -1
    assert lib.uenc_optim_adamw_step(None, 1, 1, groups, 1, state, d(0.9), d(0.999), d(1e-8), None) == -1
    assert lib.uenc_optim_adamw_step(tab, -1, 1, groups, 1, state, d(0.9), d(0.999), d(1e-8), None) == -1
    assert lib.uenc_optim_adamw_step(tab, 1, 1, None, 1, state, d(0.9), d(0.999), d(1e-8), None) == -1
    assert lib.uenc_optim_adamw_step(tab, 1, 1, groups, 0, state, d(0.9), d(0.999), d(1e-8), None) == -1
    assert lib.uenc_optim_adamw_step(tab, 1, 1, groups, 1, state + 8, d(0.9), d(0.999), d(1e-8), None) == -1
    assert lib.uenc_optim_adamw_step(tab, 1, 1, groups, 1, None, d(0.9), d(0.999), d(1e-8), None) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0                                 # nothing ran


# ---- 2. GradBuckets' flat layout ----------------------------------------------------------------------------------------------------------
def test_grad_buckets_layout_gives_identical_parameters(U):
    """The same gradients through uenc.dp.GradBuckets' flat buffer -- wrapped after a first step on separate tensors, then re-laid
    after its calibration step: two pointer changes, two table rebuilds -- and through separate tensors: bit-identical parameters."""
    from uenc.dp import GradBuckets
    from uenc.optim import FusedAdamW
    shapes = [(5,), (1000,), (33, 7), (4099,), (6,)]                   # the last parameter never receives a gradient
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(s, generator=g) * 0.02 for s in shapes]
    grads = [[torch.randn(s, generator=g) * 1e-3 for s in shapes[:-1]] for _ in range(4)]

    def net():
        m = torch.nn.Module()
        for i, v in enumerate(init):
            m.register_parameter(f"p{i}", torch.nn.Parameter(v.clone().cuda()))
        return m, [getattr(m, f"p{i}") for i in range(len(init))]
    (ma, pa), (mb, pb) = net(), net()
    oa, ob = FusedAdamW(pa, lr=1e-3, max_grad_norm=0.01), FusedAdamW(pb, lr=1e-3, max_grad_norm=0.01)
    for p, gr in zip(pb, grads[0]):                                    # twin B: separate gradient tensors throughout
        p.grad = gr.clone().cuda()
    for p, gr in zip(pa, grads[0]):
        p.grad = gr.clone().cuda()
    oa.step(); ob.step()
    gb = GradBuckets(ma, bucket_mb=0.002, listen_ops=False)
    try:
        for s in (1, 2, 3):
            gb.zero_grad()
            order = (2, 0, 3, 1) if s == 1 else (0, 1, 2, 3)             # the calibration step sees another order: the re-layout moves views
            for i in order:
                pa[i].grad.copy_(grads[s][i].cuda())
                gb.signal(pa[i])
            gb.finish()
            assert pa[-1].grad is None
            oa.step()
            for p, gr in zip(pb, grads[s]):
                p.grad.copy_(gr.cuda())
            ob.step()
            for i in range(4):
                assert pa[i].grad.data_ptr() != pb[i].grad.data_ptr() and torch.equal(pa[i].grad, pb[i].grad)
        assert oa.device_state() == ob.device_state() and oa.device_state()["step"] == 4
        for x, y in zip(pa, pb):
            assert torch.equal(x, y)
        for x, y in zip(pa[:-1], pb[:-1]):
            assert torch.equal(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])
        assert torch.equal(pa[-1].detach().cpu(), init[-1])
    finally:
        gb.close()


def test_table_rebuild_during_capture_is_refused(U, monkeypatch):
    """A moved gradient pointer while the stream is capturing: an error that says so, not a stale table (the capture state is
    simulated: the refusal is host logic and nothing may be launched)."""
    from uenc.optim import FusedAdamW
    p = torch.nn.Parameter(torch.ones(1000, device="cuda"))
    p.grad = torch.ones_like(p)
    opt = FusedAdamW([p], lr=1e-3)
    opt.step()
    other = torch.ones_like(p)
    value = p.detach().clone()
    p.grad = other
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="segment table"):
        opt.step()
    monkeypatch.undo()
    assert torch.equal(p.detach(), value) and opt.device_state()["step"] == 1
    opt.step()                                                       # eagerly the rebuild is silent
    assert opt.device_state()["step"] == 2 and float(opt.state[p]["step"]) == 2


# ---- 3. the model: cache coherence and the captured step -------------------------------------------------------------------------------------
def _small_model():
    import model  # noqa: F401  registers the architecture
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    from oracle import fill
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    cfg.SOLVER.WEIGHT_DECAY_NORM = 0.0
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM", 64,
        "MODEL.SWIN.DEPTHS", [2, 2, 2, 2], "MODEL.SWIN.NUM_HEADS", [2, 4, 8, 16], "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 6, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda",
        "SOLVER.BASE_LR", 1e-3, "SOLVER.WEIGHT_DECAY", 0.05, "SOLVER.BACKBONE_MULTIPLIER", 0.1, "SOLVER.CLIP_GRADIENTS.ENABLED", True,
        "SOLVER.CLIP_GRADIENTS.CLIP_TYPE", "full_model", "SOLVER.CLIP_GRADIENTS.CLIP_VALUE", 0.01])
    m = build_model(cfg)
    fill.fill_module(m)
    m.eval()
    return cfg, m


TASKS = ["The task is panoptic", "The task is semantic"]


def _images(seed, B=2, H=64, W=96):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float().cuda()


def _loss(out):
    from oracle import torch_ref as T
    return T.synthetic_loss(out)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_forward_after_step_sees_the_new_weights(U):
    """step() and then a forward WITHOUT ops.begin_step() (evaluation between training steps): the bf16 operand cache must not serve
    the copies of the old weights."""
    from uenc import ops
    from uenc.optim import build_optimizer
    cfg, m = _small_model()
    opt = build_optimizer(cfg, m)
    img = _images(0)
    batch = [{"left_image": img[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)]

    def forward():
        with torch.no_grad():
            out, _ = m.forward_features(batch)
        return out["pred_masks"].detach().float().clone()
    ops.begin_step(fresh_grads=True)
    out, _ = m.forward_features(batch)
    before = out["pred_masks"].detach().float().clone()
    _loss(out).backward()
    ops.flush_wgrads()
    for g in opt.param_groups:
        g["lr"] = 1e-2                                                  # large enough to matter
    casts = ops.CACHE.casts
    opt.step()
    after = forward()                                                   # no begin_step(): the cache has to notice by itself
    assert ops.CACHE.casts > casts
    ops.CACHE.invalidate()
    fresh = forward()
    ops.CACHE.invalidate()
    fresh2 = forward()
    spread = _rel(fresh2, fresh)                                        # run-to-run difference of the forward itself
    moved = _rel(after, before)
    record_parity("optim_cache_coherence", after_vs_fresh=_rel(after, fresh), fresh_run_to_run=spread, after_vs_before=moved)
    assert _rel(after, fresh) <= max(2.0 * spread, 1e-6)
    assert moved > 1e-3 and moved > 100 * max(_rel(after, fresh), 1e-9)
    # a step that calls begin_step() anyway pays no second re-cast: the one batched refresh records the new versions
    opt.step()
    ops.begin_step(fresh_grads=True)
    casts = ops.CACHE.casts
    forward()
    planned = [k for k, e in ops.CACHE._store.items() if e.plan is not None]
    assert planned and ops.CACHE.casts - casts <= len(ops.CACHE._store) - len(planned)


def _live_state(opt, params):
    return {i: (opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), float(opt.state[p]["step"]))
            for i, p in enumerate(params) if len(opt.state.get(p, {})) != 0}


def test_captured_step_with_optimizer(U):
    """GraphedTrainStep(..., optimizer=opt): each replay's update, recomputed by the float64 oracle from the parameters / optimizer
    state before the replay and the raw gradients the replay left in .grad."""
    from uenc.graphs import GraphedTrainStep
    from uenc.optim import build_optimizer
    cfg, m = _small_model()
    opt = build_optimizer(cfg, m)
    with pytest.raises(TypeError, match="FusedAdamW"):
        GraphedTrainStep(m, _loss, [{"left_image": _images(0)[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)],
                         optimizer=torch.optim.AdamW(m.parameters(), lr=1e-4))
    example = [{"left_image": _images(0)[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)]
    WARM = 2
    gs = GraphedTrainStep(m, _loss, example, warmup=WARM, optimizer=opt)
    assert opt.device_state()["step"] == WARM
    params = [g["params"][0] for g in opt.param_groups]
    groups = lambda: [([i], g["lr"], g["weight_decay"]) for i, g in enumerate(opt.param_groups)]       # noqa: E731
    worst_mine, worst_t32 = [0.0] * 4, [0.0] * 4
    for r in range(3):
        if r == 2:
            for g in opt.param_groups:                                  # a scheduler's write, no recapture
                g["lr"] *= 0.25
        snap_p = [p.detach().clone() for p in params]
        snap_s = _live_state(opt, params)
        gs.step(_images(10 + r), TASKS)
        torch.cuda.synchronize()
        grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
        live = [i for i, g in enumerate(grads) if g is not None]
        assert set(live) == set(snap_s) and len(live) > 100
        ref = TorchComposition(snap_p, groups(), 0.01, torch.float64, "cpu", snap_s)
        t32 = TorchComposition(snap_p, groups(), 0.01, torch.float32, "cuda", snap_s)
        n_ref, n_32 = ref.step(grads), t32.step(grads)
        st = opt.device_state()
        assert st["step"] == WARM + r + 1
        mine = _errors(params, {i: (opt.state[params[i]]["exp_avg"], opt.state[params[i]]["exp_avg_sq"]) for i in live}, ref, live) \
            + (abs(st["grad_norm"] - n_ref) / n_ref,)
        theirs = _errors(t32.ps, {i: (t32.moment(i, "exp_avg"), t32.moment(i, "exp_avg_sq")) for i in live}, ref, live) + (abs(n_32 - n_ref) / n_ref,)
        worst_mine = [max(a, b) for a, b in zip(worst_mine, mine)]
        worst_t32 = [max(a, b) for a, b in zip(worst_t32, theirs)]
        moved = max(float((p.detach() - q).abs().max()) for p, q in zip(params, snap_p))
        if r == 2:                                                      # the third update used the new learning rate: a quarter of the
            old = TorchComposition(snap_p, [(i, lr * 4.0, wd) for i, lr, wd in groups()], 0.01, torch.float64, "cpu", snap_s)   # step
            old.step(grads)
            stale = max(float((p.detach().double().cpu() - q.detach()).abs().max()) for p, q in zip(params, old.ps))
            assert stale > 100 * mine[0] and stale > 0.25 * moved
        assert moved > 1e-6
        for i in live:
            assert float(opt.state[params[i]]["step"]) == WARM + r + 1
    _assert_within_twice("optim_captured_step", worst_mine, worst_t32, ("param_abs", "exp_avg_rel", "exp_avg_sq_rel", "norm_rel"))


# ---- 4. the full-size parameter set -----------------------------------------------------------------------------------------------------------
def test_swin_l_parameter_set_one_step(U):
    """One step over the Swin-L OneFormer's real tensor list (shapes only; ~219 M parameters, > 2^31 bytes of table range) against the
    oracle on a random sample of tensors."""
    from oracle import torch_ref as T
    from uenc.optim import FusedAdamW
    shapes = [tuple(s) for k, s in T.model_param_shapes(T.ModelCfg(swin=T.SWIN_L)).items() if "relative_position_index" not in k]
    total = sum(int(np.prod(s)) for s in shapes)
    assert total > 2 ** 31 // 16 and len(shapes) > 400
    torch.manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, device="cuda") * 0.02) for s in shapes]
    for k, p in enumerate(ps):
        p.grad = torch.randn_like(p) * (1e-3 if k % 3 else 1e-5)
    ps[7].grad.view(-1)[0] = float("nan")
    ps[11].grad.view(-1)[-1] = INF
    ps[200].grad.view(-1)[3] = -INF
    half = len(ps) // 2
    groups = [(list(range(half)), 1e-5, 0.05), (list(range(half, len(ps))), 1e-4, 0.0)]
    max_norm = 0.01
    sq = 0.0
    for p in ps:                                                       # clip_grad_norm_ over ALL gradients, in float64
        sq += float(torch.nan_to_num(p.grad.double(), nan=0.0, posinf=1e5, neginf=-1e5).square().sum())
    norm = sq ** 0.5
    rs = np.random.RandomState(0)
    sample = sorted(set(rs.choice(len(ps), 24, replace=False).tolist()) | {7, 11, 200, int(np.argmax([p.numel() for p in ps])),
                                                                          int(np.argmin([p.numel() for p in ps]))})
    p0 = {i: ps[i].detach().clone() for i in sample}
    g0 = {i: ps[i].grad.detach().clone() for i in sample}
    opt = _fused(ps, max_norm, groups)
    opt.step()
    st = opt.device_state()
    assert abs(st["grad_norm"] - norm) <= 1e-9 * norm and st["step"] == 1
    coef = min(1.0, max_norm / (norm + 1e-6))
    worst = [0.0, 0.0]
    for i in sample:
        # this tensor's share of the composition: the gradient after nan_to_num and the full-model clip coefficient
        lr, wd = (1e-5, 0.05) if i < half else (1e-4, 0.0)
        outs = []
        for dtype, dev in ((torch.float64, "cpu"), (torch.float32, "cuda")):
            q = torch.nn.Parameter(p0[i].to(device=dev, dtype=dtype).clone())
            o = torch.optim.AdamW([q], lr=lr, weight_decay=wd)
            q.grad = torch.nan_to_num(g0[i].to(device=dev, dtype=dtype), nan=0.0, posinf=1e5, neginf=-1e5) * coef
            o.step()
            outs.append(q.detach().double().cpu())
        worst = [max(worst[0], float((ps[i].detach().double().cpu() - outs[0]).abs().max())),
                 max(worst[1], float((outs[1] - outs[0]).abs().max()))]
    _assert_within_twice("optim_swin_l_one_step", (worst[0],), (worst[1],), ("param_abs",))
