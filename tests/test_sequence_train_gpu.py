"""The differentiable TransDSSL depth decoder and ResNetLike pose decoder on the GPU against what the reference's own classes computed
(tests/golden/sequence_train.npz, tools/make_sequence_train_golden.py; the case is tests/sequence_train_fixture.py), and the sequence
training forward of the model.

  fp32 mode (ops.set_exact(True))   outputs and every stored gradient within relative L2 1e-4 of the fixture.
  product mode (bf16 operands)      outputs within the 2e-2 tests/test_sequence_gpu.py uses for this branch; each stored gradient within
                                    TWICE the error, against the same fixture, of the same nn.Module tree run through ATen under bf16
                                    autocast on the same GPU (the envelope).  Twice: the product keeps activations in bf16 between layers
                                    where autocast rounds only at the GEMMs.  The autocast run is not reproducible (ATen's backward sums
                                    with atomics): on the pose decoder with batch statistics its error on one and the same gradient was
                                    measured between 0.097 and 0.140 in four runs, while the product's error is the same number every
                                    time.  The envelope is therefore the MEDIAN over ENVELOPE_RUNS = 5 autocast runs, not a single draw
                                    (its smallest and largest draw are recorded beside it).  Envelope and kernel error are both recorded; an
                                    envelope above 5e-2 is flagged in the record, the bar stays twice the envelope.
  reproducibility                   two identical forward + backward passes in running-statistics mode give the same bits.
  training forward                  model(batch) in train() equals the hand composition of backbone, decoders and MonodepthLoss exactly;
                                    after backward() every parameter of the depth decoder, the pose decoder and the backbone has a finite
                                    non-zero gradient, the motion decoders' have none.
Every figure is recorded (`record_parity("sequence_train/...")`); a copy is profiles/sequence_train_parity.json."""
import json
import os
import statistics

import pytest
import torch

import sequence_train_fixture as SF
from conftest import record_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Z():
    return SF.load()


@pytest.fixture(scope="module")
def cot():
    return {k: v.cuda() for k, v in SF.cotangents().items()}


def _decoder(which):
    import model  # noqa: F401
    from uenc.modeling.pixel_decoder.transdssl import TransDSSL
    from uenc.modeling.pose_decoder.resnet_like_pose_decoder import ResNetLike
    if which == "depth":
        m = TransDSSL(None, None)
        SF.fill_decoders(m, None)
        return m.cuda().train()
    m = ResNetLike()
    SF.fill_decoders(None, m)
    return m.cuda()


def _features(which):
    return {k: v.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True) for k, v in SF.features(which).items()}


# ---- one run of a decoder: outputs, stored gradients, input gradients, gradient norm, buffers ------------------------------------------------
def _run(which, variant, cot, how):
    """how: "product" | "exact" (the module's own training path) or "autocast" (ATen under bf16 autocast)."""
    from uenc import ops
    m = _decoder(which)
    if which == "pose":
        SF.set_pose_variant(m, variant)
    f = _features(which)
    ops.set_exact(how == "exact")
    try:
        if how == "autocast":
            with torch.autocast("cuda", dtype=torch.bfloat16):
                raw = SF.aten_depth(m, f) if which == "depth" else SF.aten_pose(m, f)
        else:
            raw = m.forward_features(f) if which == "depth" else m(f)
        if which == "depth":
            out = {f"disp{s}": raw[("disp", s)] for s in range(4)}
            scalar = SF.depth_scalar(raw, cot)
        else:
            out = {"axisangle": raw[0], "translation": raw[1]}
            scalar = SF.pose_scalar(raw[0], raw[1], cot)
        scalar.backward()
        ops.flush_wgrads()
        torch.cuda.synchronize()
    finally:
        ops.set_exact(False)
    named = dict(m.named_parameters())
    missing = [n for n, p in named.items() if p.grad is None]
    assert not missing, missing
    res = {"out:" + k: v.detach().float() for k, v in out.items()}
    res.update({"grad:" + n: named[n].grad for n in (SF.DEPTH_PARAMS if which == "depth" else SF.POSE_PARAMS)})
    res.update({"dx:" + k: f[k].grad for k in SF.INPUT_GRADS})
    res["grad_norm"] = torch.tensor(SF.grad_norm(m))
    if which == "pose":
        bufs = dict(m.named_buffers())
        res.update({f"buf:{bn}.{leaf}": bufs[f"{bn}.{leaf}"].clone() for bn in SF.POSE_BNS for leaf in ("running_mean", "running_var", "num_batches_tracked")})
    return res, m


def _errors(res, Z, prefix):
    """Relative L2 error of every quantity the fixture stores under `prefix`, on the stored part."""
    figs = {}
    for k, v in res.items():
        key = prefix + k
        if key not in Z or "num_batches_tracked" in k:
            continue
        want = torch.from_numpy(Z[key])
        got = SF.sub(v).cpu() if v.dim() > 0 else v.cpu()
        assert got.shape == want.shape, (key, got.shape, want.shape)
        assert bool(torch.isfinite(got).all()), key
        figs[k] = SF.rel(got, want)
    return figs


ENVELOPE_RUNS = 5
CASES = [("depth", None)] + [("pose", v) for v in SF.POSE_VARIANTS]
_ids = [c[0] if c[1] is None else f"{c[0]}-{c[1]}" for c in CASES]


def _prefix(which, variant):
    return "depth_" if which == "depth" else f"pose_{variant}_"


def _check_buffers(res, Z, which, variant, tol):
    if which != "pose":
        return
    from oracle import fill
    for bn in SF.POSE_BNS:
        nbt = int(res[f"buf:{bn}.num_batches_tracked"])
        if variant == "bn_train":
            assert nbt == int(Z[f"pose_bn_train_buf:{bn}.num_batches_tracked"]) == 1
        else:                   # BatchNorm children in eval(): nothing is updated
            assert nbt == 0
            for leaf in ("running_mean", "running_var"):
                t = res[f"buf:{bn}.{leaf}"].cpu()
                assert torch.equal(t, fill.tensor_for(f"{SF.POSE_PREFIX}{bn}.{leaf}", t.shape)), (bn, leaf)


@pytest.mark.parametrize("which,variant", CASES, ids=_ids)
def test_exact_mode_against_the_reference(Z, cot, which, variant):
    res, _ = _run(which, variant, cot, "exact")
    figs = _errors(res, Z, _prefix(which, variant))
    tag = f"sequence_train/exact/{_ids[CASES.index((which, variant))]}"
    print(tag, {k: f"{v:.2e}" for k, v in figs.items()})
    record_parity(tag, **figs)
    expected = 4 + len(SF.DEPTH_PARAMS) + 3 if which == "depth" else 2 + len(SF.POSE_PARAMS) + 3 + (4 if variant == "bn_train" else 0)
    assert len(figs) == expected, sorted(figs)
    _check_buffers(res, Z, which, variant, 1e-4)
    bad = {k: v for k, v in figs.items() if not v <= 1e-4}
    assert not bad, bad


@pytest.mark.parametrize("which,variant", CASES, ids=_ids)
def test_product_mode_within_twice_the_autocast_envelope(Z, cot, which, variant):
    prefix = _prefix(which, variant)
    draws = [_errors(_run(which, variant, cot, "autocast")[0], Z, prefix) for _ in range(ENVELOPE_RUNS)]
    env = {k: statistics.median(d[k] for d in draws) for k in draws[0]}
    res, _ = _run(which, variant, cot, "product")
    figs = _errors(res, Z, prefix)
    tag = f"sequence_train/product/{_ids[CASES.index((which, variant))]}"
    rec = {}
    for k in figs:
        rec[k] = {"kernel": figs[k], "envelope": env[k], "envelope_min": min(d[k] for d in draws), "envelope_max": max(d[k] for d in draws),
                  "bar": 2e-2 if k.startswith(("out:", "buf:")) else 2.0 * env[k]}
        if not k.startswith(("out:", "buf:")) and env[k] > 5e-2:
            rec[k]["envelope_above_5e-2"] = True
    print(tag, json.dumps(rec, indent=1))
    record_parity(tag, **rec)
    _check_buffers(res, Z, which, variant, 2e-2)
    bad = {k: r for k, r in rec.items() if not r["kernel"] <= r["bar"]}
    assert not bad, bad


@pytest.mark.parametrize("which", ["depth", "pose"])
def test_two_passes_give_the_same_bits(cot, which):
    """Running-statistics mode (the pose decoder's BatchNorm children in eval()): nothing in either decoder's backward is an atomic sum."""
    a, _ = _run(which, "bn_eval", cot, "product")
    b, _ = _run(which, "bn_eval", cot, "product")
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff


# ---- the training forward of the model ----------------------------------------------------------------------------------------------------
H, W = 64, 96


def _model():
    import model  # noqa: F401
    from oracle import fill
    from uenc.config import add_common_config, add_dinat_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    from uenc.modeling.monodepth_loss import MonodepthLoss
    flat = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "cfg_cityscapes_swin_t.json")))["cfg"]
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_dinat_config(cfg); add_uni_encoder_config(cfg)
    opts = []
    for k, v in flat.items():
        opts += [k, v]
    cfg.merge_from_list(opts)
    # stochastic depth off: the two forwards compared below must draw nothing
    cfg.merge_from_list(["MODEL.DEVICE", "cuda", "MODEL.WEIGHTS", "", "INPUT.DEPTH_CROP.SIZE", (H, W), "MODEL.SWIN.DROP_PATH_RATE", 0.0,
                         "SOLVER.IMS_PER_BATCH", 2])
    m = build_model(cfg)
    fill.fill_module(m)
    return m, MonodepthLoss(cfg)


def _batch():
    g = torch.Generator().manual_seed(21)
    img = lambda: torch.randint(0, 256, (3, H, W), generator=g).float()
    K = torch.tensor([[0.58 * W, 0, 0.5 * W, 0], [0, 1.92 * H, 0.5 * H, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    out = []
    for i in range(2):
        d = {"type": "sequence", "left_image": img(), "left_prev_image": img(), "left_next_image": img(), "K": K, "inv_K": torch.linalg.inv(K)}
        if i == 1:                                  # the un-augmented frames, where present, are what the loss compares
            d.update({"orig_" + k: img() for k in ("left_image", "left_prev_image", "left_next_image")})
        out.append(d)
    return out


def _hand_composition(m, crit, batch):
    from uenc.d2 import ImageList
    from uenc.modeling.geometry import transformation_from_parameters
    norm = lambda key: ImageList.from_tensors([(x[key].cuda() - m.pixel_mean) / m.pixel_std for x in batch], m.size_divisibility).tensor
    f_cur, f_prev, f_next = m.backbone(norm("left_image")), m.backbone(norm("left_prev_image")), m.backbone(norm("left_next_image"))
    cat = lambda a, b: {k: torch.cat([a[k].float(), b[k].float()], 1) for k in a}
    a1, t1 = m.pose_decoder(cat(f_prev, f_cur))
    a2, t2 = m.pose_decoder(cat(f_cur, f_next))
    outputs = {("cam_T_cam", 0, -1): transformation_from_parameters(a1[:, 0], t1[:, 0], invert=True),
               ("cam_T_cam", 0, 1): transformation_from_parameters(a2[:, 0], t2[:, 0], invert=False)}
    disps = m.sem_seg_head.depth_decoder.forward_features(f_cur)
    outputs.update({("disp", 0, s): disps[("disp", s)] for s in range(4)})
    pick = lambda x, k: x.get("orig_" + k, x[k]).cuda().float() / 255
    targets = [{("color", 0, 0): pick(x, "left_image"), ("color", -1, 0): pick(x, "left_prev_image"), ("color", 1, 0): pick(x, "left_next_image"),
                "K": x["K"].cuda(), "inv_K": x["inv_K"].cuda()} for x in batch]
    return crit(outputs, targets)["loss_monodepth"]


def test_training_forward_of_the_model():
    from uenc import ops
    m, crit = _model()
    m.train()
    m.set_depth_criterion(crit)
    batch = _batch()
    before = {k: v.clone() for k, v in m.pose_decoder.state_dict().items()}
    with torch.no_grad():
        hand = _hand_composition(m, crit, batch)
    m.pose_decoder.load_state_dict(before)              # the hand composition stepped the BatchNorm statistics: same start for both
    losses = m(batch)
    assert set(losses) == {"loss_monodepth"} and losses["loss_monodepth"].requires_grad
    loss = losses["loss_monodepth"]
    figs = {"loss": float(loss.detach()), "hand_composition": float(hand), "difference": abs(float(loss.detach()) - float(hand))}
    print(figs)
    record_parity("sequence_train/model_forward", **figs)
    assert torch.isfinite(loss) and figs["difference"] == 0.0, figs
    loss.backward()
    ops.flush_wgrads()
    torch.cuda.synchronize()
    bad = {}
    for part in ("sem_seg_head.depth_decoder", "pose_decoder", "backbone"):
        mod = m.get_submodule(part)
        for n, p in mod.named_parameters():
            if not p.requires_grad:
                continue
            if p.grad is None or not bool(torch.isfinite(p.grad).all()) or float(p.grad.abs().sum()) == 0.0:
                bad[f"{part}.{n}"] = "none" if p.grad is None else "zero or not finite"
    assert not bad, bad
    assert all(p.grad is None for mod in (m.motion_decoder, m.motion_mask) for p in mod.parameters())
    # the segmentation half took no part
    assert all(p.grad is None for p in m.sem_seg_head.predictor.parameters())
