"""MonodepthLoss (uenc/modeling/monodepth_loss.py) without a GPU: the torch path against what the reference's own class computed
(tests/golden/monodepth_loss.npz, written by tools/make_monodepth_golden.py), and the module's contract."""
import ctypes

import numpy as np
import pytest
import torch

import monodepth_fixture as MF

REL_L2 = 2e-5                   # fp32 torch against fp32 torch: the bar tests/test_matcher_cpu.py and tests/test_oracle_golden.py hold


@pytest.fixture(scope="module")
def ML():
    import uenc.modeling.monodepth_loss as m
    return m


@pytest.fixture(scope="module")
def z():
    return MF.load()


def test_fixture_covers_the_cases(z):
    assert MF.CASES == {"a": (2, 24, 40), "b": (1, 16, 72)}
    for case, (B, H, W) in MF.CASES.items():
        assert z[f"{case}_disp3"].shape == (B, 1, H // 8, W // 8) and z[f"{case}_color0"].shape == (B, 3, H, W)
        if B > 1:
            assert not np.array_equal(z[f"{case}_K"][0], z[f"{case}_K"][1])             # K differs per image
        for fs in MF.FLAGSETS:
            assert float(z[f"{case}_{fs}_seedcheck"]) <= MF.SEED_CHECK_REL_L2 and float(z[f"{case}_{fs}_reference_rounding"]) <= 1e-5
            assert np.isfinite(z[f"{case}_{fs}_loss:loss"]) and float(z[f"{case}_{fs}_loss:loss"]) > 0
        sel = np.concatenate([z[f"{case}_automask_idsel{s}"].reshape(-1) for s in MF.SCALES])
        assert 0 < sel.mean() < 1                                                       # both kinds of candidate win somewhere


@pytest.mark.parametrize("case", list(MF.CASES))
@pytest.mark.parametrize("flagset", list(MF.FLAGSETS))
def test_torch_path_matches_reference(ML, z, case, flagset):
    """Every loss-dictionary entry and every gradient within 2e-5 relative L2 of the reference's."""
    losses, grads, outputs = MF.run(ML.MonodepthLoss, z, case, flagset)
    want = {k.split(":", 1)[1]: z[k] for k in z if k.startswith(f"{case}_{flagset}_loss:")}
    assert set(losses) == set(want)
    worst = 0.0
    for k, v in losses.items():
        e = MF.rel_l2(MF.to_numpy(v), want[k])
        worst = max(worst, e)
        print(f"{case} {flagset} {k}: {float(MF.to_numpy(v)):.8g} vs {float(want[k]):.8g}  rel {e:.3e}")
        assert e <= REL_L2, (k, e)
    for k, g in grads.items():
        e = MF.rel_l2(g.numpy(), z[f"{case}_{flagset}_grad:{k}"])
        print(f"{case} {flagset} grad {k}: rel L2 {e:.3e}")
        assert e <= REL_L2, (k, e)
    # the sample that leaves the image exercises border padding
    s = outputs[("sample", -1, 0)]
    assert bool((s.abs() > 1).any())
    if MF.FLAGSETS[flagset]["bool_automask"]:
        for sc in MF.SCALES:
            assert np.array_equal(outputs[f"identity_selection/{sc}"].numpy().astype(np.uint8), z[f"{case}_{flagset}_idsel{sc}"])


@pytest.mark.parametrize("flagset", list(MF.FLAGSETS))
def test_outputs_keys_match_reference(ML, z, flagset):
    _, _, outputs = MF.run(ML.MonodepthLoss, z, "b", flagset, backward=False)
    assert sorted(MF.key_name(k) for k in outputs) == list(z[f"b_{flagset}_outkeys"])


def test_constructor_flags_and_ramp(ML):
    cfg = MF.make_cfg(6, 192, 512)
    cfg.DATASETS.TRAIN = ("kitti", "cityscapes")
    m = ML.MonodepthLoss(cfg)
    assert (m.batch_size, m.height, m.width, m.device) == (3, 192, 512, "cpu")
    assert (m.bool_MotMask, m.bool_CmpFlow, m.bool_automask, m.move_Depth, m.move_CmpFlow, m.move_MotMask) == (False, False, False, True, False, False)
    assert (m.step, m.phrage, m.frame_ids) == (0, "pretrain", [-1, 1])
    assert (m.gp_prior, m.gp_tol, m.gp_max_it, m.gp_num_points_per_it, m.mask_disp_thrd) == (0.4, 0.005, 100, 5, 0.03)
    m.step, m.phrage = 1000, "finetune"                  # a trainer assigns them
    c = m.loss_coefs()
    assert c["p_photo"] == 1.0 and c["d_smooth"] == 1e-3 and c["d_ground"] == 0.1
    assert c["c_consistency"] == pytest.approx(5.0 * 3000 / 8000) and c["m_smooth"] == pytest.approx(0.1 * 0.375)
    m.phrage = "pretrain"
    assert m.loss_coefs()["m_sparsity"] == pytest.approx(0.04 * 3000 / 35000)
    m.step = 10 ** 6
    assert m.loss_coefs()["c_smooth"] == 1e-3
    with pytest.raises(ValueError):
        ML.MonodepthLoss(cfg, impl="triton")
    k = ML.MonodepthLoss(cfg, bool_automask=True, step=7, impl="kernels")
    assert k.bool_automask and k.step == 7


def test_forward_draws_when_nothing_is_injected(ML, z):
    B, H, W = MF.CASES["b"]
    res = []
    for _ in range(2):
        outputs, targets, _ = MF.make_inputs(z, "b")
        m = ML.MonodepthLoss(MF.make_cfg(B, H, W), **MF.FLAGSETS["full"], seed=5)
        out = m(outputs, targets)
        assert set(out) == {"loss_monodepth"} and out["loss_monodepth"].requires_grad
        res.append(float(out["loss_monodepth"].detach()))
    assert res[0] == res[1] and np.isfinite(res[0])      # the same seed, the same draws
    with pytest.raises(ValueError):
        outputs, targets, _ = MF.make_inputs(z, "b")
        ML.MonodepthLoss(MF.make_cfg(B, H, W), impl="kernels").generate_images_pred(outputs, targets)       # CPU tensors have no kernel path


def test_inverse3x3_is_the_inverse(ML):
    g = torch.Generator().manual_seed(0)
    A = torch.randn(50, 5, 3, generator=g, dtype=torch.float64)
    M = A.transpose(1, 2) @ A + 1e-6
    assert torch.allclose(ML._inverse3x3(M), torch.linalg.inv(M), rtol=1e-9, atol=1e-12)


def test_facade_import():
    import model  # noqa: F401
    import uenc.modeling.monodepth_loss as um
    from model.modeling.monodepth_loss import MonodepthLoss, disp_to_depth  # noqa: F401
    import model.modeling.monodepth_loss as mm
    assert mm is um and MonodepthLoss is um.MonodepthLoss
    from model.modeling.matcher import HungarianMatcher  # noqa: F401  what resolved before still does


def test_invalid_arguments_are_refused_without_a_gpu():
    from uenc import capi
    from uenc import kernels as K
    lib = capi.lib
    desc = np.zeros(K._VS_SLOTS, dtype=np.uint64)
    assert lib.uenc_view_synth_fwd(None, 4, 2, 1, 16, 16, 0, None) == -1
    assert lib.uenc_view_synth_fwd(desc.ctypes.data, 4, 2, 1, 16, 16, 0, None) == -1      # null tensors
    assert lib.uenc_view_synth_fwd(desc.ctypes.data, 5, 2, 1, 16, 16, 0, None) == -1      # more scales than the descriptor holds
    assert lib.uenc_view_synth_fwd(desc.ctypes.data, 4, 2, 1, 12, 16, 0, None) == -1      # 12 is not divisible by 8
    assert lib.uenc_view_synth_fwd(desc.ctypes.data, 4, 2, 1, 16, 16, 3, None) == -1      # no such mode
    assert lib.uenc_view_synth_bwd(desc.ctypes.data, 4, 2, 1, 16, 16, 0, None, 0, None) == -1
    assert lib.uenc_view_synth_workspace_floats(4, 3, 1, 16, 16) == -1 and lib.uenc_view_synth_workspace_floats(4, 2, 1, 16, 16) > 0
    assert lib.uenc_photo_loss_workspace_floats(4, 1, 1, 16) == -1 and lib.uenc_photo_loss_workspace_floats(4, 2, 24, 40) == 4 * 2 * 3 * 2
    assert lib.uenc_photo_loss_fwd(None, None, None, None, 4, 2, 1, 16, 16, 0, None, 0, None, None, None) == -1
    assert lib.uenc_photo_loss_bwd(None, None, None, None, 4, 2, 1, 16, 16, 0, None, None) == -1
    with pytest.raises(capi.UencError):
        K.photo_loss_fwd(torch.zeros(4, 2, 1, 3, 16, 16), torch.zeros(1, 3, 16, 16))       # CPU tensors
    assert ctypes.sizeof(ctypes.c_void_p) * K._VS_SLOTS == 536
