"""ConvNeXt on the GPU: the depthwise-convolution kernels against fp64 ATen on the host, `ops.convnext_block` and `D2ConvNeXt` against the
reference's fixture (tests/golden/convnext.npz), training mode, and the backbone inside the full model.

Bars (relative L2 error): fp32 "exact" mode 1e-4 for outputs and 1e-3 for gradients (tests/test_exact_gpu.py);
product mode 2^-9 + 1e-4 for a bf16-rounded fp32 value, 1.5e-2 for what passes through the bf16 GEMMs (test_swin_t_backbone_golden),
gradients against the sensitivity envelope stored in the fixture."""
import pytest
import torch
import torch.nn.functional as F

import convnext_fixture as CF
from conftest import record_parity

pytestmark = pytest.mark.gpu

SHAPES = [(2, 5, 9, 40), (1, 2, 3, 320), (1, 3, 5, 1536), (1, 16, 24, 192), (2, 7, 7, 8)]
EPS = 1e-6
rel = CF.rel


@pytest.fixture(scope="module")
def U():
    import model  # noqa: F401
    import uenc
    return uenc


@pytest.fixture(scope="module")
def Z():
    return {k: (torch.from_numpy(v) if v.dtype.kind == "f" else v) for k, v in CF.load().items()}


@pytest.fixture()
def exact():
    from uenc import ops
    ops.set_exact(True)
    yield
    ops.set_exact(False)


_OP_REF = {}


def _op_case(shape):
    """Inputs of one op case and its fp64 host reference (forward and autograd backward), computed once."""
    if shape in _OP_REF:
        return _OP_REF[shape]
    B, H, W, C = shape
    tag = "x".join(map(str, shape))
    t = {"x": CF.input_for("op_x" + tag, shape), "w": CF.tensor_for("op." + tag + ".dw", (C, 1, 7, 7)) * 4, "b": CF.tensor_for("op." + tag + ".bias", (C,)),
         "g": CF.tensor_for("op." + tag + ".weight", (C,)), "be": CF.tensor_for("op." + tag + ".beta", (C,)),
         "dh": CF.input_for("op_dh" + tag, shape), "dout": CF.input_for("op_dout" + tag, shape)}
    d = {k: v.double().requires_grad_(True) for k, v in t.items() if k not in ("dh", "dout")}
    y = F.conv2d(d["x"].permute(0, 3, 1, 2), d["w"], d["b"], padding=3, groups=C).permute(0, 2, 3, 1)
    h = F.layer_norm(y, (C,), d["g"], d["be"], EPS)
    mean = y.mean(-1)
    rstd = (y.var(-1, unbiased=False) + EPS).rsqrt()
    gx, gw, gb, gg, gbe = torch.autograd.grad(h, [d["x"], d["w"], d["b"], d["g"], d["be"]], t["dh"].double())
    ref = {"y": y.detach(), "h": h.detach(), "mean": mean.detach(), "rstd": rstd.detach(), "dx": gx + t["dout"].double(), "dx0": gx, "dw": gw,
           "db": gb, "dgamma": gg, "dbeta": gbe}
    _OP_REF[shape] = (t, ref)
    return t, ref


def _run_op(t, with_dout=True):
    from uenc import kernels as K
    c = {k: v.cuda() for k, v in t.items()}
    y, h, st = K.dwconv7_ln_fwd(c["x"], c["w"], c["b"], c["g"], c["be"], EPS)
    dg, dbe = torch.zeros_like(c["g"]), torch.zeros_like(c["be"])
    dx, dy = K.dwconv7_ln_bwd_data(c["dh"].to(K.adt()), y, st, c["g"], c["w"], dout=c["dout"] if with_dout else None, dgamma=dg, dbeta=dbe)
    dw, db = torch.zeros_like(c["w"]), torch.zeros_like(c["b"])
    K.dwconv7_bwd_weight(dy, c["x"], dw, db)
    dw2, db2 = torch.zeros_like(c["w"]), torch.zeros_like(c["b"])
    K.dwconv7_bwd_weight(dy, c["x"], dw2, db2)
    torch.cuda.synchronize()
    return dict(y=y, h=h, mean=st[:, 0].view(y.shape[:3]), rstd=st[:, 1].view(y.shape[:3]), dx=dx, dw=dw, db=db, dgamma=dg, dbeta=dbe, dw2=dw2, db2=db2)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_forward_and_backward_exact(U, exact, shape):
    t, ref = _op_case(shape)
    o = _run_op(t)
    figs = {k: rel(o[k], ref[k]) for k in ("y", "h", "mean", "rstd", "dx", "dw", "db", "dgamma", "dbeta")}
    print(shape, figs)
    record_parity("convnext/op_exact/" + "x".join(map(str, shape)), **figs)
    assert o["h"].dtype == torch.float32
    assert figs["y"] <= 1e-4 and figs["h"] <= 1e-4
    assert figs["mean"] <= 1e-5 and figs["rstd"] <= 1e-5
    for k in ("dx", "dw", "db", "dgamma", "dbeta"):
        assert figs[k] <= 1e-4, (k, figs[k])
    assert torch.equal(o["dw"], o["dw2"]) and torch.equal(o["db"], o["db2"])           # two calls: the same bits
    o0 = _run_op({**t, "dout": torch.zeros_like(t["dout"])})
    on = _run_op(t, with_dout=False)
    assert torch.equal(o0["dx"], on["dx"])
    assert rel(on["dx"], ref["dx0"]) <= 1e-4


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_op_forward_product(U, shape):
    t, ref = _op_case(shape)
    o = _run_op(t)
    figs = {k: rel(o[k], ref[k]) for k in ("y", "h", "mean", "rstd")}
    print(shape, figs)
    record_parity("convnext/op_bf16/" + "x".join(map(str, shape)), **figs)
    assert o["h"].dtype == torch.bfloat16
    assert figs["h"] <= 2.0 ** -9 + 1e-4 and figs["y"] <= 1e-4
    assert figs["mean"] <= 1e-5 and figs["rstd"] <= 1e-5
    assert torch.equal(o["dw"], o["dw2"]) and torch.equal(o["db"], o["db2"])


def test_channel_count_check(U):
    from uenc import kernels as K, ops
    x = torch.zeros(1, 4, 4, 12, device="cuda")
    with pytest.raises(ValueError):
        K.dwconv7_ln_fwd(x, torch.zeros(12, 1, 7, 7, device="cuda"), None, torch.ones(12, device="cuda"), torch.zeros(12, device="cuda"))
    with pytest.raises(ValueError):
        ops.convnext_block(x, [None] * 9)


def _block(case, dim, ls):
    from uenc.modeling.backbone.convnext import Block
    blk = Block(dim, layer_scale_init_value=ls)
    CF.fill_module(blk, case + ".")
    return blk.cuda()


def _block_run(Z, blk, record):
    from uenc import kernels as K
    x = Z["block_x"].cuda().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    y, h, _ = K.dwconv7_ln_fwd(x.detach(), blk.dwconv.weight.detach(), blk.dwconv.bias.detach(), blk.norm.weight.detach(), blk.norm.bias.detach(), EPS)
    out = blk(x)
    out.backward(Z["block_dout"].cuda().permute(0, 2, 3, 1).contiguous())
    torch.cuda.synchronize()
    figs = {"y": rel(y.permute(0, 3, 1, 2), Z["block_y"]), "h": rel(h, Z["block_h"]), "out": rel(out.permute(0, 3, 1, 2), Z["block_out"]),
            "dx": rel(x.grad.permute(0, 3, 1, 2), Z["block_dx"])}
    for n, p in blk.named_parameters():
        figs["grad:" + n] = rel(p.grad, Z["block_grad:" + n])
    print(record, figs)
    record_parity(record, **figs)
    return figs


def test_block_exact(U, Z, exact):
    figs = _block_run(Z, _block("block", CF.BLOCK_DIM, 1.0), "convnext/block_exact")
    for k, v in figs.items():
        assert v <= (1e-4 if k in ("y", "h", "out") else 1e-3), (k, v)          # "grad:gamma": the rowsum identity


def test_block_product(U, Z):
    figs = _block_run(Z, _block("block", CF.BLOCK_DIM, 1.0), "convnext/block_bf16")
    assert figs["y"] <= 1e-4 and figs["h"] <= 2.0 ** -9 + 1e-4 and figs["out"] <= 1.5e-2


@pytest.mark.parametrize("mode", ["exact", "bf16"])
def test_block_without_layer_scale(U, Z, mode):
    from uenc import ops
    blk = _block("nols", CF.NOLS_DIM, 0)
    assert blk.gamma is None
    ops.set_exact(mode == "exact")
    try:
        with torch.no_grad():
            out = blk(Z["nols_x"].cuda().permute(0, 2, 3, 1).contiguous())
    finally:
        ops.set_exact(False)
    e = rel(out.permute(0, 3, 1, 2), Z["nols_out"])
    record_parity("convnext/nols_" + mode, out=e)
    assert e <= (1e-4 if mode == "exact" else 1.5e-2)


def _net():
    from uenc.modeling.backbone.convnext import ConvNeXt
    net = ConvNeXt(**CF.NET)
    CF.fill_module(net, "net.")
    return net.cuda()


def _net_run(Z):
    net = _net()
    x = Z["net_x"].cuda().requires_grad_(True)
    outs = net(x)
    loss = sum(v.square().mean() for v in outs.values())
    loss.backward()
    torch.cuda.synchronize()
    q = {k: v.detach() for k, v in outs.items()}
    q["loss"], q["dx"] = loss.detach(), x.grad
    g = dict(net.named_parameters())
    for n in CF.NAMED:
        q["grad:" + n] = CF.rows(n, g[n].grad)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in g.values())
    return q


def test_backbone_exact(U, Z, exact):
    q = _net_run(Z)
    figs = {k: rel(v, Z["net_" + k]) for k, v in q.items()}
    print(figs)
    record_parity("convnext/net_exact", **figs)
    for k, v in figs.items():
        assert v <= (1e-4 if k.startswith("res") or k == "loss" else 1e-3), (k, v)
    for k in ("res2", "res3", "res4", "res5"):
        assert q[k].shape == Z["net_" + k].shape


def test_backbone_product(U, Z):
    q = _net_run(Z)
    figs = {k: rel(v, Z["net_" + k]) for k, v in q.items()}
    coss = {k: CF.cos(v, Z["net_" + k]) for k, v in q.items() if k.startswith("grad:") or k == "dx"}
    print(figs, coss)
    record_parity("convnext/net_bf16", **figs, **{"cos:" + k: v for k, v in coss.items()},
                  **{"env:" + k: float(Z["net_env_err:" + k]) for k in figs})
    for k in ("res2", "res3", "res4", "res5"):
        assert figs[k] <= 1.5e-2, (k, figs[k])
    for k in coss:
        assert figs[k] <= 1.5 * float(Z["net_env_err:" + k]) + 2e-2, (k, figs[k], float(Z["net_env_err:" + k]))
        assert coss[k] >= float(Z["net_env_cos:" + k]) - 0.01, (k, coss[k])


def test_backbone_batch_independence(U, Z):
    net = _net()
    x = Z["net_x"].cuda()
    with torch.no_grad():
        both, one = net(x), net(x[:1])
    figs = {k: rel(one[k][0], both[k][0]) for k in both}
    record_parity("convnext/net_batch_independence", **figs)
    assert max(figs.values()) <= 1e-6, figs


def test_block_training_mode_drop_path(U, Z):
    blk = _block("block", CF.BLOCK_DIM, 1.0)
    blk.drop_path_rate = 0.5
    blk.train()
    x = Z["block_x"].cuda().permute(0, 2, 3, 1).contiguous()
    dout = Z["block_dout"].cuda().permute(0, 2, 3, 1).contiguous()

    def run(xx, dd, dp, train):
        blk.train(train)
        for p in blk.parameters():
            p.grad = None
        xi = xx.clone().requires_grad_(True)
        out = blk(xi, dp=dp)
        out.backward(dd)
        torch.cuda.synchronize()
        return out.detach(), xi.grad, {n: p.grad.clone() for n, p in blk.named_parameters()}
    out, dx, grads = run(x, dout, [2.0, 0.0], True)
    assert torch.equal(out[1], x[1])                                   # dropped image: the input, bit for bit
    assert torch.equal(dx[1], dout[1])
    # the dropped image contributes nothing to the parameter gradients: the same as the kept image alone
    _, _, g1 = run(x[:1], dout[:1], [2.0], True)
    figs = {"dropped_share:" + n: rel(grads[n], g1[n]) for n in grads}
    assert max(figs.values()) <= 1e-5, figs
    # kept image: the eval-mode block with the branch doubled
    oe, dxe, _ = run(x[:1], dout[:1], None, False)
    figs["kept_out"] = rel(out[0] - x[0], 2.0 * (oe[0] - x[0]))
    figs["kept_dx"] = rel(dx[0] - dout[0], 2.0 * (dxe[0] - dout[0]))
    record_parity("convnext/block_train_mode", **figs)
    assert figs["kept_out"] <= 1e-2 and figs["kept_dx"] <= 1e-2, figs


def test_full_model_with_convnext_backbone(U):
    from oracle import fill, torch_ref as T
    from uenc.config import add_common_config, add_convnext_config, add_swin_config, add_uni_encoder_config
    from uenc.d2 import build_model, get_cfg
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_convnext_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", "D2ConvNeXt", "MODEL.CONVNEXT.DIMS", CF.NET["dims"],
        "MODEL.CONVNEXT.DEPTHS", CF.NET["depths"], "MODEL.CONVNEXT.DROP_PATH_RATE", 0.0, "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead",
        "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder", "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19,
        "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 6, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    fill.fill_module(m)
    CF.fill_module(m.backbone, "net.")
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
