"""Capturable training step (uenc/graphs.py) and the device-side randomness under it (csrc/step_rng.hip, ops.device_rng), on the GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def U():
    import model  # noqa: F401  registers the architecture, loads libuenc_hip.so
    import uenc
    return uenc


def _rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------
# 1. the step RNG kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_branch,n_samples,n_seed", [(1, 1, 1), (7, 2, 5), (48, 4, 40)])
def test_step_rng_matches_reference(U, n_branch, n_samples, n_seed):
    from uenc import kernels as K
    dev = torch.device("cuda")
    base = 0x1234_5678_9ABC_DEF0 & (2 ** 63 - 1)
    state = torch.tensor([base, 5], dtype=torch.int64, device=dev)
    kp = np.linspace(0.5, 1.0, n_branch, dtype=np.float32)
    kp[0] = 0.7
    keep = torch.from_numpy(kp).to(dev)
    scales = torch.full((n_branch * n_samples,), -1.0, device=dev)
    seeds = torch.zeros(n_seed, dtype=torch.int32, device=dev)
    prev = None
    for step in range(6, 10):
        K.step_rng_advance(state, keep, n_branch, n_samples, scales, n_seed, seeds, advance=True)
        torch.cuda.synchronize()
        assert int(state[1]) == step
        rs, rseeds = K.step_rng_reference(base, step, kp, n_samples, n_seed)
        np.testing.assert_array_equal(scales.cpu().numpy().reshape(n_branch, n_samples), rs)
        np.testing.assert_array_equal(seeds.cpu().numpy().view(np.uint32), rseeds)
        if prev is not None:
            assert not np.array_equal(prev, rseeds)                      # consecutive steps differ
        prev = rseeds
    # advance=0 rewrites the same step's tables
    K.step_rng_advance(state, keep, n_branch, n_samples, scales, n_seed, seeds, advance=False)
    torch.cuda.synchronize()
    assert int(state[1]) == 9
    np.testing.assert_array_equal(seeds.cpu().numpy().view(np.uint32), prev)


@pytest.mark.parametrize("p", [0.1, 0.3])
def test_step_rng_keep_fraction(U, p):
    from uenc import kernels as K
    dev = torch.device("cuda")
    nb, B, steps = 16, 4, 256
    state = torch.tensor([99, 0], dtype=torch.int64, device=dev)
    keep = torch.full((nb,), 1.0 - p, device=dev)
    scales = torch.empty(nb * B, device=dev)
    seeds = torch.empty(4, dtype=torch.int32, device=dev)
    kept = torch.zeros((), device=dev)
    for _ in range(steps):
        K.step_rng_advance(state, keep, nb, B, scales, 4, seeds)
        kept += (scales > 0).sum()
    n = nb * B * steps
    frac = float(kept) / n
    sigma = (p * (1 - p) / n) ** 0.5
    assert abs(frac - (1 - p)) < 4 * sigma, (frac, 1 - p, sigma)
    v = scales[scales > 0]
    assert torch.all(v == v[0]) and abs(float(v[0]) - 1 / (1 - p)) < 1e-6


# ------------------------------------------------------------------------------------------------
# 2. seed-by-pointer twins and the index-hash dropout kernel
# ------------------------------------------------------------------------------------------------
def test_dropout_sp_matches_by_value_and_reference(U):
    from uenc import kernels as K
    dev = torch.device("cuda")
    seeds = torch.tensor([0, 12345, -7], dtype=torch.int32, device=dev)
    g = torch.Generator(device="cpu").manual_seed(0)
    x16 = torch.randn(3 * 1024 + 8, generator=g).to(dev, torch.bfloat16)
    for slot in range(3):
        s = K.SeedSlot(seeds, slot)
        a = K.dropout_bf16(x16, s.value(), 0.1)
        b = K.dropout_sp(x16, s, 0.1)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
        c = K.dropout_bf16(x16, s, 0.1)                                   # the wrapper dispatches a SeedSlot to the twin
        assert torch.equal(a.view(torch.int16), c.view(torch.int16))
        for dtype, n in ((torch.float32, 4097), (torch.bfloat16, 1029)):   # odd sizes: the scalar path
            x = torch.randn(n, generator=g).to(dev, dtype)
            y = K.dropout_sp(x, s, 0.3)
            keep = K.dropout_keep_reference((n,), 0.3, s.value()).to(dev)
            assert torch.equal(y != 0, keep & (x != 0))
            inv = float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.3)))           # the kernel's fp32 1 / (1 - p)
            ref = torch.where(keep, (x.float() * inv).to(dtype), torch.zeros_like(x))
            assert torch.equal(y, ref)


def test_mha_seed_pointer_twin_bit_identical(U):
    from uenc import kernels as K
    from uenc.capi import check, lib, stream_ptr
    dev = torch.device("cuda")
    g = torch.Generator(device="cpu").manual_seed(1)
    B, H, Lq, S = 2, 8, 150, 600
    E = H * 32
    q, k, v, do = (torch.randn(B, n, E, generator=g).to(dev, torch.bfloat16) for n in (Lq, S, S, Lq))
    seeds = torch.tensor([31337, 4242], dtype=torch.int32, device=dev)
    nws = lib.uenc_mha_fwd_workspace_floats(B, H, Lq, S)
    ws = torch.empty(max(nws, 1), device=dev)
    scale = 32 ** -0.5

    def fwd(seed):
        out = torch.empty(B, Lq, E, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, H, Lq, device=dev)
        a = (q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1), 0, 0,
             out.data_ptr(), out.stride(0), out.stride(1), lse.data_ptr(), ws.data_ptr() if nws else 0, B, H, Lq, S, scale, 0.1)
        if isinstance(seed, K.SeedSlot):
            check(lib.uenc_mha_fwd_sp(*a, seed.seeds.data_ptr(), seed.slot, stream_ptr()))
        else:
            check(lib.uenc_mha_fwd(*a, seed, stream_ptr()))
        return out, lse

    def bwd(seed, out, lse):
        dq = torch.zeros(B, Lq, E, device=dev)
        dk = torch.empty(B, S, E, dtype=torch.bfloat16, device=dev)
        dv = torch.empty(B, S, E, dtype=torch.bfloat16, device=dev)
        a = (q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(), k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1), 0, 0,
             out.data_ptr(), out.stride(0), out.stride(1), lse.data_ptr(), do.data_ptr(), do.stride(0), do.stride(1),
             dq.data_ptr(), dq.stride(0), dq.stride(1), dk.data_ptr(), dk.stride(0), dk.stride(1), dv.data_ptr(), dv.stride(0), dv.stride(1),
             B, H, Lq, S, scale, 0.1)
        if isinstance(seed, K.SeedSlot):
            check(lib.uenc_mha_bwd_sp(*a, seed.seeds.data_ptr(), seed.slot, stream_ptr()))
        else:
            check(lib.uenc_mha_bwd(*a, seed, stream_ptr()))
        return dq, dk, dv

    for slot in range(2):
        s = K.SeedSlot(seeds, slot)
        o1, l1 = fwd(s.value())
        o2, l2 = fwd(s)
        assert torch.equal(o1.view(torch.int16), o2.view(torch.int16)) and torch.equal(l1, l2)
        r1, r2 = bwd(s.value(), o1, l1), bwd(s, o1, l1)
        # dQ is accumulated with float atomics across key splits: equal up to their order; dK / dV are stored once
        assert _rel(r2[0], r1[0]) < 1e-6
        assert torch.equal(r1[1].view(torch.int16), r2[1].view(torch.int16)) and torch.equal(r1[2].view(torch.int16), r2[2].view(torch.int16))
    o3, _ = fwd(K.SeedSlot(seeds, 1))
    o4, _ = fwd(K.SeedSlot(seeds, 0))
    assert not torch.equal(o3, o4)


# ------------------------------------------------------------------------------------------------
# 3. DropPath weight gradient with device multipliers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["kept", "mixed", "dropped"])
def test_branch_wgrad_device_scales_matches_host_runs(U, pattern):
    from uenc import ops
    dev = torch.device("cuda")
    B, L, C, N = 4, 1024, 256, 512
    keep = 0.7
    sc = {"kept": [1 / keep] * B, "mixed": [1 / keep, 0.0, 1 / keep, 1 / keep], "dropped": [0.0] * B}[pattern]
    g = torch.Generator(device="cpu").manual_seed(2)
    dy = torch.randn(B * L, N, generator=g).to(dev, torch.bfloat16)
    x = torch.randn(B * L, C, generator=g).to(dev, torch.bfloat16)
    w = torch.nn.Parameter(torch.zeros(N, C, device=dev))
    b = torch.nn.Parameter(torch.zeros(N, device=dev))
    seen = []
    ops.set_grad_listener(seen.append)
    try:
        res = []
        for scales in (sc, ops.DeviceScales(torch.tensor(sc, device=dev))):
            w.grad, b.grad = torch.zeros_like(w), torch.zeros_like(b)
            seen.clear()
            ops.WGRADS.reset()
            ops._branch_wgrad(dy, x, w.grad, b.grad, (w, b), scales)
            ops.flush_wgrads()
            torch.cuda.synchronize()
            assert [id(p) for p in seen] == [id(w), id(b)]                      # one gradient-ready notification per parameter
            res.append((w.grad.clone(), b.grad.clone()))
    finally:
        ops.set_grad_listener(None)
    ref_w = ((dy.float().view(B, L, N) * torch.tensor(sc, device=dev).view(B, 1, 1)).view(-1, N).t() @ x.float())
    if pattern == "dropped":
        assert float(res[1][0].abs().max()) == 0.0 and float(res[1][1].abs().max()) == 0.0
        assert float(res[0][0].abs().max()) == 0.0
        return
    # the device path rounds the scaled gradient to bf16 once (operand path); the host path scales the fp32 accumulator
    assert _rel(res[1][0], res[0][0]) < 4e-3 and _rel(res[1][1], res[0][1]) < 4e-3
    assert _rel(res[1][0], ref_w) < 4e-3


# ------------------------------------------------------------------------------------------------
# 4. the whole small OneFormer-Swin in training mode under ops.device_rng
# ------------------------------------------------------------------------------------------------
def _small_model(drop_path=0.3):
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    from oracle import fill
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", "D2SwinTransformer", "MODEL.SWIN.EMBED_DIM", 64,
        "MODEL.SWIN.DEPTHS", [2, 2, 2, 2], "MODEL.SWIN.NUM_HEADS", [2, 4, 8, 16], "MODEL.SWIN.DROP_PATH_RATE", drop_path,
        "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 6, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    fill.fill_module(m)
    return m


TASKS = ["The task is panoptic", "The task is semantic"]


def _images(seed, B=2, H=64, W=96):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, 3, H, W), generator=g).float().cuda()


def _loss(out):
    from oracle import torch_ref as T
    return T.synthetic_loss(out)


def _snap(model, loss, out):
    s = {n: p.grad.detach().float().cpu().clone() for n, p in model.named_parameters() if p.grad is not None}
    s["loss"] = loss.detach().float().cpu().clone()
    s["pred_logits"] = out["pred_logits"].detach().float().cpu().clone()
    s["pred_masks"] = out["pred_masks"].detach().float().cpu().clone()
    return s


def _eager(model, images, tasks, rng=None, state=None):
    """One eager step (zero grads, begin_step, forward, loss, backward, flush), optionally under ops.device_rng from `state`."""
    from uenc import ops
    batch = [{"left_image": images[i], "task": tasks[i], "type": "segmentation"} for i in range(images.shape[0])]
    for p in model.parameters():
        if p.grad is not None:
            p.grad.zero_()
    if state is not None:
        rng.set_state(state)

    def run():
        ops.begin_step(fresh_grads=True)
        out, _ = model.forward_features(batch)
        loss = _loss(out)
        loss.backward()
        ops.flush_wgrads()
        return loss, out
    if rng is not None:
        with ops.device_rng(rng):
            loss, out = run()
    else:
        loss, out = run()
    torch.cuda.synchronize()
    return _snap(model, loss, out)


def _replay(gs, images, tasks=None, state=None):
    if state is not None:
        gs.rng.set_state(state)
    loss, out = gs.step(images, tasks)
    torch.cuda.synchronize()
    return _snap(gs.model, loss, out)


def _spread(runs):
    """Eager run-to-run spread: the largest relative difference of any compared tensor over the pairs (run i, run 0), i = 1..3."""
    return max(_rel(r[k], runs[0][k]) for r in runs[1:] for k in runs[0])


def _assert_close(rep, ref, spread):
    tol = max(2.0 * spread, 1e-5)
    worst = max(((k, _rel(rep[k], ref[k])) for k in ref), key=lambda t: t[1])
    assert set(rep) == set(ref) and worst[1] <= tol, (worst, tol)


def test_train_step_under_device_rng(U):
    """Training mode with every random site on the device tables, eagerly: the same RNG state gives the same step (within the eager
    run-to-run spread), the next step draws fresh tables, nothing is drawn from torch's CPU generator, and the tables equal the host
    restatement.  A backward after the next begin_step() is refused."""
    from uenc import kernels as K
    from uenc import ops
    m = _small_model()
    m.train()
    img = _images(0)
    rng = ops.DeviceRNG(7)
    _eager(m, img, TASKS, rng)                                 # registers the slots
    # 7 Swin blocks x 2 branches (the first block's DropPath rate is 0), and the decoder / encoder dropout sites
    assert len(rng.branch_keep) == 14 and rng.n_seed > 0
    st = rng.get_state()
    cpu_state = torch.get_rng_state()
    runs = [_eager(m, img, TASKS, rng, st) for _ in range(4)]
    assert torch.equal(torch.get_rng_state(), cpu_state)     # nothing was drawn from torch's CPU generator
    tab = rng.scales.clone()
    _assert_close(runs[0], runs[1], _spread(runs[1:]))
    d = _eager(m, img, TASKS, rng)                             # the next step: fresh draws
    assert not torch.equal(rng.scales, tab) and float(d["loss"]) != float(runs[0]["loss"])
    ref, rseeds = K.step_rng_reference(7, int(rng.state[1]), np.array(rng.branch_keep, dtype=np.float32), 2, rng.n_seed)
    np.testing.assert_array_equal(rng.scales[:14 * 2].cpu().numpy().reshape(14, 2), ref)
    np.testing.assert_array_equal(rng.seeds[:rng.n_seed].cpu().numpy().view(np.uint32), rseeds)
    batch = [{"left_image": img[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)]
    with ops.device_rng(rng):
        ops.begin_step(fresh_grads=True)
        out, _ = m.forward_features(batch)
        loss = _loss(out)
        ops.begin_step(fresh_grads=True)
        with pytest.raises(RuntimeError, match="begin_step"):
            loss.backward()
    ops.WGRADS.reset()
    m.eval()


@pytest.fixture(scope="module")
def eval_step(U):
    from uenc.graphs import GraphedTrainStep
    m = _small_model()
    m.eval()
    batch = [{"left_image": _images(0)[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)]
    gs = GraphedTrainStep(m, _loss, batch, warmup=2)
    yield gs
    del gs


def test_eval_capture_matches_eager(eval_step):
    gs = eval_step
    for seed in (1, 2, 3):
        img = _images(seed)
        rep = _replay(gs, img, TASKS)
        eager = [_eager(gs.model, img, TASKS) for _ in range(4)]
        _assert_close(rep, eager[0], _spread(eager))


def test_task_change_between_replays(eval_step):
    gs = eval_step
    img = _images(4)
    tasks = ["The task is instance", "The task is panoptic"]
    rep = _replay(gs, img, tasks)
    other = _replay(gs, img, TASKS)
    again = _replay(gs, img, tasks)
    eager = [_eager(gs.model, img, tasks) for _ in range(4)]
    spread = _spread(eager)
    _assert_close(rep, eager[0], spread)
    _assert_close(again, eager[0], spread)
    assert _rel(other["pred_logits"], rep["pred_logits"]) > 1e-4          # the task really changed what was computed


def test_capture_refusals(eval_step, monkeypatch):
    from uenc import ops
    from uenc.graphs import GraphedTrainStep
    gs = eval_step
    with pytest.raises(ValueError, match="shape"):
        gs.step(_images(5, H=96, W=96))
    with pytest.raises(ValueError, match="shape"):
        gs.step(_images(5, B=1))
    batch = [{"left_image": _images(0)[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)]
    ops.set_exact(True)
    try:
        with pytest.raises(RuntimeError, match="exact"):
            GraphedTrainStep(gs.model, _loss, batch)
        with pytest.raises(RuntimeError, match="exact"):
            gs.step(_images(5))
    finally:
        ops.set_exact(False)
    from uenc.capi import lib
    lib.uenc_prof_enable(1)
    try:
        with pytest.raises(RuntimeError, match="launch timers"):
            GraphedTrainStep(gs.model, _loss, batch)
    finally:
        lib.uenc_prof_enable(0)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 2)
    with pytest.raises(RuntimeError, match="world size"):
        GraphedTrainStep(gs.model, _loss, batch)


def test_train_capture_matches_eager_device_rng(U):
    from uenc.graphs import GraphedTrainStep
    m = _small_model(drop_path=0.3)
    m.train()
    batch = [{"left_image": _images(0)[i], "task": TASKS[i], "type": "segmentation"} for i in range(2)]
    gs = GraphedTrainStep(m, _loss, batch, warmup=2, seed=7)
    assert len(gs.rng.branch_keep) == 14 and gs.rng.n_seed > 0
    img = _images(6)
    st = gs.rng.get_state()
    rep = _replay(gs, img, TASKS, state=st)
    tab1 = gs.rng.scales.clone()
    rep2 = _replay(gs, img, TASKS)                                        # next replay: fresh draws on the device
    tab2 = gs.rng.scales.clone()
    assert float(rep2["loss"]) != float(rep["loss"]) and not torch.equal(tab1, tab2)
    eager = [_eager(m, img, TASKS, gs.rng, st) for _ in range(4)]
    _assert_close(rep, eager[0], _spread(eager))
    assert torch.equal(gs.rng.scales, tab1)                               # the eager step from the same state drew the replay's table
    rep3 = _replay(gs, img, TASKS, state=st)                              # replays after eager steps still match
    _assert_close(rep3, eager[0], _spread(eager))
    m.eval()
    del gs
