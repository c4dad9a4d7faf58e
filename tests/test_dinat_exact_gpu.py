"""The fp32 "exact" arithmetic mode on the DiNAT path (uenc_na2d_f32_*, csrc/exact.hip) against oracle/dinat_ref.py.

The bf16 DiNAT tests (tests/test_dinat_gpu.py) bound the product mode loosely (3e-2 on backbone outputs, 8e-2 on parameter
gradients): bf16 noise of that size could hide an indexing error at a border or at a large dilation.  In exact mode every
operand, activation and accumulation is fp32, so the same paths must meet the Swin path's fp32 bars (tests/test_exact_gpu.py):
kernels 2e-5 (rpb gradient 1e-4: a sum over every query of a head), module outputs 1e-4, parameter gradients 2e-3, the
free-running small model 1e-4 on the loss, 1e-3 on logits and mask logits with >= 99.9 % mask-sign agreement.  References
run in float64 on the host, except the decoder half of the full model (oracle/torch_ref.py, fp32 as in the bf16 test).

PARITY UNPINNED as in the bf16 tests: NATTEN 0.14.4 is not available, the oracle restates its published algorithm.
"""
import os
import sys

import pytest
import torch

from conftest import mask_band_figures, record_parity

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.fixture(scope="module")
def U():
    import model  # noqa: F401
    import uenc
    return uenc


@pytest.fixture()
def exact(U):
    from uenc import ops
    ops.set_exact(True)
    yield ops
    ops.set_exact(False)


def _rand(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------------
# kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_rpb", [True, False], ids=["rpb", "no_rpb"])
@pytest.mark.parametrize("B,H,W,nH,ks,d", [(2, 13, 21, 2, 3, 1),
                                            (1, 24, 70, 3, 5, 2),       # W > 64 and not a multiple of 64
                                            (2, 28, 19, 2, 7, 1),
                                            (1, 30, 33, 4, 9, 3),
                                            (1, 13, 13, 1, 13, 1),      # window = image
                                            (1, 112, 120, 2, 7, 16)])   # DiNAT-L's largest dilation
def test_na2d_f32_kernels_vs_oracle(exact, B, H, W, nH, ks, d, with_rpb):
    """Output, log-sum-exp and the gradients of q, k, v and rpb against the float64 oracle; drpb is accumulated into."""
    from oracle import dinat_ref as D
    from uenc import kernels as K
    C = nH * 32
    scale = 32 ** -0.5
    qkv = _rand(B, H, W, 3 * C, seed=1)
    rpb = _rand(nH, 2 * ks - 1, 2 * ks - 1, seed=2, scale=0.5) if with_rpb else None
    dout = _rand(B, H, W, C, seed=3)
    x = qkv.double().reshape(B, H, W, 3, nH, 32).permute(3, 0, 4, 1, 2, 5).contiguous().requires_grad_()
    r = rpb.double().requires_grad_() if with_rpb else None
    want = D.na2d(x[0] * scale, x[1], x[2], r, ks, d).permute(0, 2, 3, 1, 4).reshape(B, H, W, C)
    want.backward(dout.double())
    dqkv_want = x.grad.permute(1, 3, 4, 0, 2, 5).reshape(B, H, W, 3 * C)
    # log-sum-exp of the scores of every window, from the oracle's neighbour lists
    ny, py = D.axis_neighbours(H, ks, d)
    nx, px = D.axis_neighbours(W, ks, d)
    xd = x.detach()
    s = torch.einsum("bhyxc,bhyixjc->bhyxij", xd[0] * scale, xd[1][:, :, ny][:, :, :, :, nx])
    if with_rpb:
        s = s + rpb.double()[:, py][:, :, :, px].permute(0, 1, 3, 2, 4)
    lse_want = s.reshape(B, nH, H, W, ks * ks).logsumexp(-1)
    del s

    rpb_d = rpb.cuda() if with_rpb else None
    out, lse = K.na2d_fwd(qkv.cuda(), rpb_d, nH, ks, d, scale)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, H, W, C)
    figs = {"out": rel(out, want), "lse": rel(lse, lse_want)}
    drpb0 = drpb = None
    if with_rpb:              # nonzero start value of the size of the gradient itself: an overwrite instead of an add fails
        drpb0 = _rand(*rpb.shape, seed=4) * float(r.grad.norm() / r.grad.numel() ** 0.5)
        drpb = drpb0.cuda()
    dqkv = K.na2d_bwd(qkv.cuda(), rpb_d, out, dout.cuda(), lse, nH, ks, d, scale, drpb)
    assert dqkv.dtype == torch.float32
    for i, name in enumerate("qkv"):
        figs["d" + name] = rel(dqkv[..., i * C:(i + 1) * C], dqkv_want[..., i * C:(i + 1) * C])
    if with_rpb:
        figs["drpb"] = rel(drpb.double().cpu() - drpb0.double(), r.grad)
    record_parity(f"exact/na2d_f32[B{B}-{H}x{W}-h{nH}-k{ks}-d{d}-{'rpb' if with_rpb else 'no_rpb'}]",
                  pinned_by="oracle/dinat_ref.py only (NATTEN 0.14.4 absent)", **figs)
    assert figs["out"] <= 2e-5 and figs["lse"] <= 2e-5, figs
    assert max(figs["dq"], figs["dk"], figs["dv"]) <= 2e-5, figs
    assert not with_rpb or figs["drpb"] <= 1e-4, figs


def test_na2d_f32_rejects_bad_arguments(exact):
    """A map smaller than kernel x dilation, an even kernel and a kernel above 13 are refused (UENC_EINVAL) before any launch."""
    from uenc import capi, kernels as K
    nH, C = 1, 32
    s = torch.cuda.current_stream().cuda_stream
    for H, W, ks, d in ((6, 20, 7, 1), (20, 20, 4, 1), (20, 20, 15, 1), (20, 13, 7, 2)):
        qkv = torch.randn(1, H, W, 3 * C, device="cuda")
        with pytest.raises(capi.UencError):
            K.na2d_fwd(qkv, None, nH, ks, d, 0.1)
        out = torch.full((1, H, W, C), 7.0, device="cuda")
        lse = torch.full((1, nH, H, W), 7.0, device="cuda")
        dqkv = torch.full_like(qkv, 7.0)
        drpb = torch.full((nH, 2 * ks - 1, 2 * ks - 1), 7.0, device="cuda")
        with pytest.raises(capi.UencError):
            K.na2d_bwd(qkv, None, out, out.clone(), lse, nH, ks, d, 0.1, drpb)
        assert capi.lib.uenc_na2d_f32_fwd(qkv.data_ptr(), None, out.data_ptr(), lse.data_ptr(), 1, H, W, nH, ks, d, 0.1, s) == -1
        assert capi.lib.uenc_na2d_f32_bwd(qkv.data_ptr(), None, out.data_ptr(), out.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                          drpb.data_ptr(), 1, H, W, nH, ks, d, 0.1, s) == -1
        torch.cuda.synchronize()
        for t in (out, lse, dqkv, drpb):                  # nothing was written: no kernel and no memset ran
            assert bool((t == 7.0).all())


@pytest.mark.parametrize("Cin,Cout,H,W,bias", [(3, 32, 33, 47, True), (64, 128, 17, 23, True), (64, 96, 15, 9, False)])
def test_conv3x3_s2_exact(exact, Cin, Cout, H, W, bias):
    """The 3x3 stride-2 convolution (ConvTokenizer / ConvDownsampler): the 3-channel image (strided-slice patches) and the HIP
    gather (Cin % 8 == 0), odd H and W, forward plus input / weight / bias gradients against float64."""
    ops = exact
    ops.CACHE.invalidate()
    x = _rand(2, H, W, Cin, seed=4).cuda().requires_grad_()
    w = torch.nn.Parameter(_rand(Cout, Cin, 3, 3, seed=5, scale=(9 * Cin) ** -0.5).cuda())
    b = torch.nn.Parameter(_rand(Cout, seed=6).cuda()) if bias else None
    dy = _rand(2, (H + 1) // 2, (W + 1) // 2, Cout, seed=7)
    y = ops.conv3x3_s2(x, w, b)
    y.backward(dy.cuda())
    ops.flush_wgrads()
    x2 = x.detach().double().cpu().requires_grad_()
    w2 = w.detach().double().cpu().requires_grad_()
    b2 = b.detach().double().cpu().requires_grad_() if bias else None
    y2 = torch.nn.functional.conv2d(x2.permute(0, 3, 1, 2), w2, b2, stride=2, padding=1).permute(0, 2, 3, 1)
    y2.backward(dy.double())
    figs = {"y": rel(y, y2), "dx": rel(x.grad, x2.grad), "dw": rel(w.grad, w2.grad)}
    if bias:
        figs["db"] = rel(b.grad, b2.grad)
    record_parity(f"exact/conv3x3_s2[{Cin}->{Cout}-{H}x{W}]", **figs)
    assert y.dtype == torch.float32 and x.grad.dtype == torch.float32
    assert all(v <= 1e-5 for v in figs.values()), figs
    ops.CACHE.invalidate()


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def _dinat_pair(cfg):
    """The product backbone and the oracle's state dict with the same deterministic weights (as tests/test_dinat_gpu.py)."""
    from oracle import dinat_ref as D, fill
    from uenc.modeling.backbone.dinat import DiNAT
    m = DiNAT(embed_dim=cfg.embed_dim, mlp_ratio=cfg.mlp_ratio, depths=list(cfg.depths), num_heads=list(cfg.num_heads),
              kernel_size=cfg.kernel_size, dilations=cfg.dilations, out_indices=cfg.out_indices)
    sd = fill.state_dict_for(D.dinat_param_shapes(cfg))
    m.load_state_dict({k[len("backbone."):]: v for k, v in sd.items()}, strict=True)
    m = m.cuda()
    m.eval()
    return m, sd


@pytest.mark.parametrize("H,W,dil", [(128, 192, ((1, 2), (1, 2), (1, 1), (1,))), (96, 64, ((1, 1), (1, 1), (1, 1), (1,)))])
def test_dinat_backbone_exact_vs_oracle(exact, H, W, dil):
    """Whole backbone forward + backward in exact mode against the float64 oracle: fused NATLayers, and NATTEN's zero-padding
    path in the last stage at 96 x 64 (3 x 2 pixels)."""
    from oracle import dinat_ref as D
    ops = exact
    ops.CACHE.invalidate()
    cfg = D.DiNATCfg(64, 2.0, (2, 2, 2, 1), (2, 4, 8, 16), 3, dil)
    m, sd = _dinat_pair(cfg)
    img = _rand(2, 3, H, W, seed=9)
    outs = m(img.cuda())
    sdg = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    want = D.dinat_backbone(img.double(), sdg, cfg)
    figs = {}
    for k in ("res2", "res3", "res4", "res5"):
        assert tuple(outs[k].shape) == tuple(want[k].shape) and outs[k].dtype == torch.float32
        figs[k] = rel(outs[k], want[k])
    w = {k: _rand(*want[k].shape, seed=20 + i) for i, k in enumerate(sorted(want))}
    sum((outs[k] * w[k].cuda()).sum() for k in w).backward()
    ops.flush_wgrads()
    sum((want[k] * w[k].double()).sum() for k in w).backward()
    gerr = {name: rel(p.grad, sdg["backbone." + name].grad) for name, p in m.named_parameters()}
    worst = max(gerr, key=gerr.get)
    record_parity(f"exact/dinat_backbone[{H}x{W}]", pinned_by="oracle/dinat_ref.py only (NATTEN 0.14.4 absent)",
                  max_param_grad_rel=gerr[worst], worst_param=worst, median_param_grad_rel=sorted(gerr.values())[len(gerr) // 2], **figs)
    assert max(figs.values()) <= 1e-4, figs
    bad = {n: e for n, e in gerr.items() if e > 2e-3}
    assert not bad, bad
    ops.CACHE.invalidate()


@pytest.mark.parametrize("H,W", [(12, 20), (4, 5)])
def test_nat_layer_drop_path_training_exact(exact, H, W):
    """Training-mode stochastic depth of one NATLayer in exact mode, fused path (12 x 20) and NATTEN's padding path (4 x 5), against
    the float64 oracle layer with the same per-sample multipliers."""
    from oracle import dinat_ref as D, fill
    from uenc.modeling.backbone.dinat import NATLayer
    ops = exact
    ops.CACHE.invalidate()
    C, nH, ks, d, B = 64, 2, 3, 2, 3
    layer = NATLayer(C, nH, ks, d, mlp_ratio=2.0, drop_path=0.2).cuda()
    p = "backbone.levels.0.blocks.0"
    fill.fill_module(layer, p + ".")
    sd = {p + "." + k: v.detach().double().cpu().clone().requires_grad_() for k, v in layer.state_dict().items()}
    x = _rand(B, H, W, C, seed=11).cuda().requires_grad_()
    dy = _rand(B, H, W, C, seed=12)
    layer.train()
    torch.manual_seed(3)
    s1, s2 = ops.drop_path_scales(B, 0.2), ops.drop_path_scales(B, 0.2)
    assert all(v in (0.0, 1 / 0.8) for v in s1 + s2)
    torch.manual_seed(3)
    y = layer(x)
    y.backward(dy.cuda())
    ops.flush_wgrads()
    x2 = x.detach().double().cpu().requires_grad_()
    y2 = D.nat_layer(x2, sd, p, nH, ks, d, branch_scale=(torch.tensor(s1, dtype=torch.float64), torch.tensor(s2, dtype=torch.float64)))
    y2.backward(dy.double())
    figs = {"y": rel(y, y2), "dx": rel(x.grad, x2.grad)}
    gerr = {n: rel(q.grad, sd[p + "." + n].grad) for n, q in layer.named_parameters() if sd[p + "." + n].grad is not None}
    record_parity(f"exact/nat_layer_drop_path[{H}x{W}]", scales=[s1, s2], max_param_grad_rel=max(gerr.values()), **figs)
    assert y.dtype == torch.float32
    assert figs["y"] <= 1e-4 and figs["dx"] <= 2e-3, figs
    bad = {n: e for n, e in gerr.items() if e > 2e-3}
    assert not bad, bad
    ops.CACHE.invalidate()


# ---------------------------------------------------------------------------------------------------------------------
# full model
# ---------------------------------------------------------------------------------------------------------------------
_DIL = [[1, 2], [1, 2], [1, 1], [1]]


def _small_dinat_model():
    """The small OneFormer-DiNAT model of tests/test_dinat_gpu.py::test_full_model_with_dinat_backbone, same cfg."""
    from oracle import fill
    from uenc.d2 import get_cfg, build_model
    from uenc.config import add_common_config, add_dinat_config, add_swin_config, add_uni_encoder_config
    cfg = get_cfg()
    add_common_config(cfg); add_swin_config(cfg); add_dinat_config(cfg); add_uni_encoder_config(cfg)
    cfg.merge_from_list([
        "MODEL.META_ARCHITECTURE", "OneFormer", "MODEL.BACKBONE.NAME", "D2DiNAT", "MODEL.DiNAT.EMBED_DIM", 64, "MODEL.DiNAT.MLP_RATIO", 2.0,
        "MODEL.DiNAT.DEPTHS", [2, 2, 2, 1], "MODEL.DiNAT.NUM_HEADS", [2, 4, 8, 16], "MODEL.DiNAT.KERNEL_SIZE", 3, "MODEL.DiNAT.DILATIONS", _DIL,
        "MODEL.SEM_SEG_HEAD.NAME", "OneFormerHead", "MODEL.SEM_SEG_HEAD.PIXEL_DECODER_NAME", "MSDeformAttnPixelDecoder",
        "MODEL.SEM_SEG_HEAD.NUM_CLASSES", 19, "MODEL.SEM_SEG_HEAD.CONVS_DIM", 256, "MODEL.SEM_SEG_HEAD.IN_FEATURES", ["res2", "res3", "res4", "res5"],
        "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", 6, "MODEL.ONE_FORMER.TRANSFORMER_IN_FEATURE", "multi_scale_pixel_decoder",
        "MODEL.ONE_FORMER.NUM_OBJECT_QUERIES", 150, "MODEL.ONE_FORMER.DEC_LAYERS", 10, "MODEL.IS_TRAIN", False,
        "MODEL.PIXEL_MEAN", [123.675, 116.280, 103.530], "MODEL.PIXEL_STD", [58.395, 57.120, 57.375], "MODEL.DEVICE", "cuda"])
    m = build_model(cfg)
    fill.fill_module(m, "")
    m.eval()
    return m


def test_full_model_with_dinat_backbone_exact(U):
    """The small FREE-RUNNING OneFormer-DiNAT model (its decoder's attention masks are thresholded intermediate predictions), forward
    + backward in both modes against the oracle: exact mode meets the Swin exact model's bars; the bf16 figures are recorded."""
    from oracle import dinat_ref as D, torch_ref as T
    from uenc import ops
    g = torch.Generator().manual_seed(21)
    imgs = [torch.randint(0, 256, (3, 128, 192), generator=g).float() for _ in range(2)]
    batch = [{"left_image": im, "task": t, "type": "segmentation"} for im, t in zip(imgs, ("The task is panoptic", "The task is semantic"))]
    res, want, wl, sd = {}, None, None, None
    for mode in ("bf16", "exact"):
        ops.set_exact(mode == "exact")
        try:
            m = _small_dinat_model()
            out, _ = m.forward_features(batch)
            loss = T.synthetic_loss(out)
            loss.backward()
            ops.flush_wgrads()
            if want is None:          # the oracle (same weights by name), once
                sd = {k: v.detach().cpu().clone().requires_grad_() for k, v in m.state_dict().items() if v.dtype.is_floating_point}
                mcfg = T.ModelCfg()
                x = T.preprocess(imgs, mcfg)
                tasks = T.task_embedding([b["task"] for b in batch], sd, mcfg)
                feats = D.dinat_backbone(x, sd, D.DiNATCfg(64, 2.0, (2, 2, 2, 1), (2, 4, 8, 16), 3, _DIL))
                mf, _, ms = T.pixel_decoder(feats, sd, mcfg.head)
                want = T.transformer_decoder(ms, mf, tasks, sd, mcfg.head)
                wl = T.synthetic_loss(want)
                wl.backward()
            gerr = {n: rel(p.grad, sd[n].grad) for n, p in m.named_parameters()
                    if n.startswith("backbone.") and p.grad is not None and sd[n].grad is not None}
            worst = max(gerr, key=gerr.get)
            res[mode] = {"loss_rel": abs(float(loss.detach()) / float(wl.detach()) - 1),
                         "pred_logits": rel(out["pred_logits"], want["pred_logits"]), "pred_masks": rel(out["pred_masks"], want["pred_masks"]),
                         "mask_sign_agreement": float(((out["pred_masks"].detach().cpu() > 0) == (want["pred_masks"].detach() > 0)).float().mean()),
                         "mask_band": mask_band_figures(out["pred_masks"], want["pred_masks"]),
                         "backbone_grad_rel_max": gerr[worst], "backbone_grad_rel_worst_param": worst,
                         "backbone_grad_rel_median": sorted(gerr.values())[len(gerr) // 2], "backbone_params_with_grad": len(gerr)}
            del m, out, loss
        finally:
            ops.set_exact(False)
    record_parity("dinat_unpinned/small_full_model_free_running_exact", pinned_by="oracle/dinat_ref.py + oracle/torch_ref.py (backbone unpinned)",
                  exact=res["exact"], bf16=res["bf16"])
    e = res["exact"]
    assert e["loss_rel"] < 1e-4 and e["pred_logits"] < 1e-3 and e["pred_masks"] < 1e-3 and e["mask_sign_agreement"] >= 0.999, e
    assert e["backbone_params_with_grad"] > 100 and e["backbone_grad_rel_max"] <= 5e-3, e


def test_full_size_dinat_l_exact_vs_bf16(U):
    """BASELINE configs[4]'s model (OneFormer with DiNAT-L: kernel 7, dilations up to 16) on one 1024 x 2048 image, forward only.
    No host oracle is feasible at this size (the gathered keys of stage 1 alone would take several GB), so exact mode -- validated
    against the oracle by the tests above -- is the reference: it must be finite and run-to-run bit-identical.  The product (bf16)
    mode is then measured against it in the contract's units and recorded, not asserted: these are the first such figures for
    configs[4]."""
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    import bench
    from oracle import fill
    from uenc import ops
    from uenc.d2 import build_model
    g = torch.Generator().manual_seed(7)
    img = torch.randint(0, 256, (3, bench.H_IMG, bench.W_IMG), generator=g).float().cuda()
    batch = [{"left_image": img, "task": "The task is panoptic", "type": "segmentation", "height": bench.H_IMG, "width": bench.W_IMG}]
    saved = bench.BACKBONE
    res = {}
    for mode in ("exact", "bf16"):
        ops.set_exact(mode == "exact")
        try:
            bench.BACKBONE = "dinat"
            try:
                m = build_model(bench.make_cfg("cuda"))
            finally:
                bench.BACKBONE = saved
            assert type(m.backbone).__name__ == "D2DiNAT"
            fill.fill_module(m, "")
            m.eval()
            with torch.no_grad():
                out, _ = m.forward_features(batch)
                res[mode] = {k: out[k].detach().float().cpu() for k in ("pred_logits", "pred_masks")}
                if mode == "exact":
                    again, _ = m.forward_features(batch)
                    for k in ("pred_logits", "pred_masks"):
                        assert torch.isfinite(res[mode][k]).all(), k
                        assert torch.equal(res[mode][k], again[k].detach().float().cpu()), k          # bit-identical repeat
                    del again
            del m, out
            torch.cuda.empty_cache()
        finally:
            ops.set_exact(False)
    e, b = res["exact"], res["bf16"]
    assert tuple(e["pred_logits"].shape) == (1, 150, 20) and tuple(e["pred_masks"].shape) == (1, 150, 256, 512)
    record_parity("dinat_unpinned/full_size_dinat_l_bf16_vs_exact", reference="exact mode (fp32), one 1024x2048 image, forward",
                  pred_logits=rel(b["pred_logits"], e["pred_logits"]), pred_masks=rel(b["pred_masks"], e["pred_masks"]),
                  mask_sign_agreement=float(((b["pred_masks"] > 0) == (e["pred_masks"] > 0)).float().mean()),
                  mask_band=mask_band_figures(b["pred_masks"], e["pred_masks"]))
