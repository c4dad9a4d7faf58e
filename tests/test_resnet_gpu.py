"""The ResNet backbone (uenc/modeling/backbone/resnet.py) against tests/golden/resnet.npz: what the reference's own resnet.py computes on
the cases of tests/resnet_fixture.py (tools/make_resnet_golden.py).

Bars (relative L2 error).  fp32 "exact" mode: 1e-4 for outputs and loss, 1e-3 for every stored gradient, 1e-5 for the running statistics
(the project's bars of tests/test_convnext_gpu.py; the reference's own fp32 rounding on these cases is below 1e-5, stored in the file).
Product mode: 1.5 * env + 2e-2 per output, env being the same quantity's error in the reference run with bf16-rounded parameters and
convolution inputs (the margin of test_backbone_product in tests/test_convnext_gpu.py on this fixture's own envelope); eval-mode gradients
the same and cosine >= env_cos - 0.01.  Train-mode gradients through bf16 at these map sizes are dominated by ReLU flips (the envelope
itself reaches 0.47): they are asserted finite and recorded beside their envelope, not barred.
"""
import numpy as np
import pytest
import torch

import resnet_fixture as RF
from conftest import record_parity

pytestmark = pytest.mark.gpu
rel, cos = RF.rel, RF.cos


@pytest.fixture(scope="module")
def U():
    import model  # noqa: F401
    import uenc
    return uenc


@pytest.fixture(scope="module")
def Z():
    return {k: (torch.from_numpy(v) if v.dtype.kind in "fi" else v) for k, v in RF.load().items()}


@pytest.fixture()
def exact():
    from uenc import ops
    ops.set_exact(True)
    yield
    ops.set_exact(False)


def _net(which, freeze_at=0):
    from uenc.modeling.backbone import resnet as R
    net = RF.build(R, which)
    net.freeze(freeze_at)
    RF.fill_module(net, which + ".")
    return net.cuda()


def _run(Z, case, freeze_at=0):
    which, mode = case.split("_")
    net = _net(which, freeze_at)
    net.train(mode == "train")
    outs = net(Z["x"].cuda())
    loss = RF.loss_of(outs)
    loss.backward()
    torch.cuda.synchronize()
    q = {"out:" + k: RF.sub_out(outs[k].detach()) for k in RF.OUTS}
    q["loss"] = loss.detach()
    for k in RF.OUTS:
        assert outs[k].dtype == torch.float32 and tuple(outs[k].shape[2:]) == RF.SIZES[k], k
    for n, p in net.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
            q["grad:" + n] = RF.sub_grad(p.grad)
        else:
            assert p.grad is None, n
    return q, net


@pytest.mark.parametrize("case", RF.CASES)
def test_backbone_exact(U, Z, exact, case):
    q, net = _run(Z, case)
    figs = {k: rel(v, Z[f"{case}_{k}"]) for k, v in q.items()}
    if case.endswith("train"):
        for n, b in net.named_buffers():
            ref = Z[f"{case}_buf:{n}"]
            if n.endswith("num_batches_tracked"):
                assert int(b) == int(ref) == 1, n
            else:
                figs["buf:" + n] = rel(b, ref)
    print({k: f"{v:.2e}" for k, v in figs.items()})
    record_parity("resnet/exact/" + case, **figs)
    for k, v in figs.items():
        assert v <= (1e-3 if k.startswith("grad:") else (1e-5 if k.startswith("buf:") else 1e-4)), (k, v)
        assert q.get(k, None) is None or q[k].shape == Z[f"{case}_{k}"].shape, k


@pytest.mark.parametrize("case", RF.CASES)
def test_backbone_product(U, Z, case):
    q, _ = _run(Z, case)
    figs = {k: rel(v, Z[f"{case}_{k}"]) for k, v in q.items()}
    coss = {k: cos(v, Z[f"{case}_{k}"]) for k, v in q.items() if k.startswith("grad:")}
    env = {k: float(Z[f"{case}_env_err:{k}"]) for k in figs}
    print({k: (f"{figs[k]:.3g}", f"env {env[k]:.3g}") for k in figs})
    record_parity("resnet/bf16/" + case, **figs, **{"cos:" + k: v for k, v in coss.items()}, **{"env:" + k: v for k, v in env.items()},
                  **{"env_cos:" + k: float(Z[f"{case}_env_cos:{k}"]) for k in coss})
    for k in figs:
        if not k.startswith("grad:"):
            assert figs[k] <= 1.5 * env[k] + 2e-2, (k, figs[k], env[k])
        elif case.endswith("eval"):
            assert figs[k] <= 1.5 * env[k] + 2e-2, (k, figs[k], env[k])
            assert coss[k] >= float(Z[f"{case}_env_cos:{k}"]) - 0.01, (k, coss[k])
        else:
            assert np.isfinite(figs[k]), k


def test_frozen_stages(U, Z, exact):
    q, net = _run(Z, "basic_train", freeze_at=2)
    trainable = [str(n) for n in Z["frozen_trainable"]]
    assert [n for n, p in net.named_parameters() if p.grad is not None] == trainable
    assert sorted(k[5:] for k in q if k.startswith("grad:")) == sorted(trainable)
    figs = {k: rel(v, Z["frozen_" + k]) for k, v in q.items()}
    record_parity("resnet/exact/frozen", **figs)
    for k, v in figs.items():
        assert v <= (1e-3 if k.startswith("grad:") else 1e-4), (k, v)
    assert list(net.state_dict().keys()) == [str(n) for n in Z["frozen_names"]]


@pytest.mark.parametrize("which", RF.NETS)
def test_batch_independence_in_eval_mode(U, Z, which):
    net = _net(which).eval()
    x = Z["x"].cuda()
    with torch.no_grad():
        both, one = net(x), net(x[:1])
    figs = {k: rel(one[k][0], both[k][0]) for k in both}
    record_parity("resnet/batch_independence/" + which, **figs)
    assert max(figs.values()) <= 1e-6, figs


@pytest.mark.parametrize("which", RF.NETS)
def test_state_dict_round_trip(U, Z, which):
    net = _net(which)
    sd = {}
    for n, s in zip(Z[which + "_names"], Z[which + "_shapes"]):
        shape = [int(v) for v in str(s).split(",")] if str(s) else []
        sd[str(n)] = torch.tensor(7) if str(n).endswith("num_batches_tracked") else RF.tensor_for("rt." + str(n), shape)
    net.load_state_dict(sd, strict=True)
    back = net.state_dict()
    assert list(back.keys()) == list(sd.keys()) and all(torch.equal(back[k].cpu(), sd[k]) for k in sd)


def test_train_mode_refusals(U, Z):
    net = _net("basic").train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        net(torch.zeros(1, 3, 2, 2, device="cuda"))                  # the stem's map is 1 x 1 with one image
    with pytest.raises(RuntimeError, match="no gradient for the image"):
        net(Z["x"].cuda().requires_grad_(True))


def test_full_model_with_resnet_backbone(U):
    from oracle import fill, torch_ref as T
    from uenc.config import add_common_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", "build_custom_resnet_backbone", "MODEL.BACKBONE.FREEZE_AT", 0,
        "MODEL.RESNETS.DEPTH", 18, "MODEL.RESNETS.RES2_OUT_CHANNELS", 64, "MODEL.RESNETS.NORM", "BN", "MODEL.RESNETS.STRIDE_IN_1X1", False,
        "MODEL.RESNETS.OUT_FEATURES", ["res2", "res3", "res4", "res5"], "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 6, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    fill.fill_module(m)
    RF.fill_module(m.backbone, "full.")
    m.eval()
    g = torch.Generator().manual_seed(0)
    batch = [{"left_image": torch.randint(0, 256, (3, 64, 96), generator=g).float(), "task": t, "type": "segmentation"}
             for t in ("The task is panoptic", "The task is semantic")]
    out, _ = m.forward_features(batch)
    T.synthetic_loss(out).backward()
    torch.cuda.synchronize()
    assert out["pred_logits"].shape == (2, 150, 20) and out["pred_masks"].shape == (2, 150, 16, 24)
    assert bool(torch.isfinite(out["pred_logits"]).all()) and bool(torch.isfinite(out["pred_masks"].float()).all())
    for n, p in m.backbone.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
