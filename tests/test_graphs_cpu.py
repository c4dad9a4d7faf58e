"""Capturable training step: the host restatement of the device RNG tables, the randomness entry points outside device-RNG mode, and the
capture refusals that need no GPU."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def U():
    import uenc
    return uenc


def test_new_entry_points_declared_and_bound(U):
    from uenc import capi
    hdr = open(os.path.join(ROOT, "include", "uenc.h")).read()
    for name in ("uenc_step_rng_advance", "uenc_dropout_sp", "uenc_scale_rows_bf16", "uenc_mha_fwd_sp", "uenc_mha_bwd_sp", "uenc_upload",
                 "uenc_prof_active"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.exported_symbols() and hasattr(capi.lib, name)
    assert capi.lib.uenc_prof_active() == 0


def test_mix_restatement_is_the_attention_hash(U):
    """step_rng_reference is built from the attn_keep hash: its mixing function reproduces the attention keep-mask restatement."""
    from uenc import kernels as K
    from uenc.attention import keep_mask_reference
    idx = np.arange(4096, dtype=np.uint64) | np.uint64(3 << 33)
    for seed in (0, 1, 0xDEADBEEF):
        x = K._mix32_np(np.uint64(seed), idx)
        thresh = int(np.float32(0.25) * 4294967296.0)
        keep = x >= thresh
        assert 0.70 < keep.mean() < 0.80
    # exact agreement with keep_mask_reference on the low index range
    x = K._mix32_np(np.uint64(12345), np.arange(1000, dtype=np.uint64))
    ref = keep_mask_reference(1, 1, 1, 1000, 0.3, 12345).view(-1).numpy()
    assert np.array_equal(x >= int(float(np.float32(0.3)) * 4294967296.0), ref)


def test_step_rng_reference_properties(U):
    from uenc import kernels as K
    kp = np.array([0.9, 0.7, 1.0, 0.5], dtype=np.float32)
    s1, d1 = K.step_rng_reference(7, 1, kp, 4, 6)
    s1b, d1b = K.step_rng_reference(7, 1, kp, 4, 6)
    s2, d2 = K.step_rng_reference(7, 2, kp, 4, 6)
    s3, d3 = K.step_rng_reference(8, 1, kp, 4, 6)
    assert np.array_equal(s1, s1b) and np.array_equal(d1, d1b)                # a pure function of (seed, step, slot, sample)
    assert not np.array_equal(d1, d2) and not np.array_equal(d1, d3)
    assert s1.shape == (4, 4) and d1.shape == (6,) and d1.dtype == np.uint32
    assert np.all(s1[2] == 1.0)                                              # keep_prob 1: always kept, multiplier 1
    for i, k in enumerate(kp):
        assert set(np.unique(s1[i])) <= {np.float32(0.0), np.float32(1.0) / k}
    fr = np.mean([(K.step_rng_reference(3, t, np.full(8, 0.7, np.float32), 4, 0)[0] > 0).mean() for t in range(1, 257)])
    sigma = (0.3 * 0.7 / (256 * 32)) ** 0.5
    assert abs(fr - 0.7) < 4 * sigma


def test_host_randomness_unchanged_outside_device_mode(U):
    """Outside ops.device_rng the DropPath and dropout draws are the same CPU-generator draws as before."""
    from uenc import ops
    assert not ops.device_rng_active()
    torch.manual_seed(5)
    a = ops.drop_path_scales(4, 0.3)
    s = ops.dropout_seeds(3)
    one = ops.dropout_seed()
    torch.manual_seed(5)
    keep = 0.7
    assert a == [float(v) / keep for v in torch.floor(keep + torch.rand(4)).tolist()]
    assert s == tuple(int(v) for v in torch.randint(0, 2 ** 31 - 1, (3,)).tolist())
    assert one == int(torch.randint(0, 2 ** 31 - 1, (1,)))


def test_device_rng_refuses_exact_mode(U):
    from uenc import kernels as K
    from uenc import ops
    old = K.EXACT
    K.EXACT = True
    try:
        with pytest.raises(RuntimeError, match="exact"):
            with ops.device_rng(ops.DeviceRNG.__new__(ops.DeviceRNG)):
                pass
    finally:
        K.EXACT = old
    assert not ops.device_rng_active()
class _Fake:
    def __init__(self, backbone):
        self.backbone = backbone


class D2SwinTransformer:
    pass


class D2DiNAT:
    pass


def test_graph_refusals_without_gpu(U, monkeypatch):
    from uenc import graphs
    from uenc import kernels as K
    from uenc import ops
    graphs._refuse_unsupported(_Fake(D2SwinTransformer()))                   # nothing to refuse
    with pytest.raises(ValueError, match="Swin backbone is required"):
        graphs._refuse_unsupported(_Fake(D2DiNAT()))
    monkeypatch.setattr(K, "EXACT", True)
    with pytest.raises(RuntimeError, match="exact"):
        graphs._refuse_unsupported(_Fake(D2SwinTransformer()))
    monkeypatch.setattr(K, "EXACT", False)
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_world_size", lambda *a: 4)
    with pytest.raises(RuntimeError, match="world size 4"):
        graphs._refuse_unsupported(_Fake(D2SwinTransformer()))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: False)
    ops.set_grad_listener(lambda p: None)
    try:
        with pytest.raises(RuntimeError, match="listener"):
            graphs._refuse_unsupported(_Fake(D2SwinTransformer()))
    finally:
        ops.set_grad_listener(None)


def test_sequence_inputs_refused(U):
    from uenc.graphs import GraphedTrainStep
    img = torch.zeros(3, 64, 96)
    m = _Fake(D2SwinTransformer())
    with pytest.raises(ValueError, match="sequence-branch"):
        GraphedTrainStep(m, lambda o: o, [{"left_image": img, "task": "t", "type": "sequence"}])
    with pytest.raises(ValueError, match="one shape"):
        GraphedTrainStep(m, lambda o: o, [{"left_image": img, "task": "t", "type": "segmentation"},
                                          {"left_image": torch.zeros(3, 32, 32), "task": "t", "type": "segmentation"}])
