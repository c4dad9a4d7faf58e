"""Structure and rules of the sequence branch's training forward, without a GPU: which path the decoders take in which mode, what
`OneFormer.sequence_training_losses` refuses, and where `OneFormer.forward` sends a (mode, criteria, batch)."""
import types

import pytest
import torch
import torch.nn as nn

import monodepth_fixture as MF
import sequence_train_fixture as SF


@pytest.fixture(scope="module")
def mods():
    import model  # noqa: F401
    from uenc.modeling.pixel_decoder import transdssl
    from uenc.modeling.pose_decoder import resnet_like_pose_decoder as pose
    return types.SimpleNamespace(transdssl=transdssl, pose=pose)


def _features(which, hw=(64, 96)):
    mult = 2 if which == "pose" else 1
    return {k: torch.zeros(1, c * mult, hw[0] // s, hw[1] // s) for k, c, s in zip(SF.LEVELS, SF.SWIN_T_CH, SF.STRIDES)}


def _counting_convnet(calls):
    """Stand-ins for uenc.convnet.conv_bn_act / conv: count the call and return zeros of the convolution's output shape."""
    def conv_bn_act(x, c, bn=None, relu=False, out_dtype=torch.float32):
        calls.append(c)
        st = c.stride[0]
        return torch.zeros(x.shape[0], c.out_channels, -(-x.shape[2] // st), -(-x.shape[3] // st))
    return conv_bn_act, (lambda x, c, relu=False, out_dtype=torch.float32: conv_bn_act(x, c, None, relu, out_dtype))


def _forbid_ops(monkeypatch):
    from uenc import ops
    def boom(*a, **k):
        raise AssertionError("an autograd node of the training path ran in eval mode")
    for name in ("linear", "conv3x3", "conv_bn_act", "upsample2x_ac", "softmax_gate", "soft_att_depth"):
        monkeypatch.setattr(ops, name, boom)


def test_eval_depth_decoder_runs_the_convnet_path(mods, monkeypatch):
    calls = []
    cba, conv = _counting_convnet(calls)
    monkeypatch.setattr(mods.transdssl, "conv_bn_act", cba)
    monkeypatch.setattr(mods.transdssl, "conv", conv)
    _forbid_ops(monkeypatch)
    dec = mods.transdssl.TransDSSL(None, None).eval()
    out = dec.forward_features(_features("depth"))
    convs = [m for m in dec.modules() if isinstance(m, nn.Conv2d)]
    assert len(calls) == len(convs) == 39 and set(map(id, calls)) == set(map(id, convs))          # every convolution, once
    assert [tuple(out[("disp", s)].shape) for s in range(4)] == [(1, 1, 64 >> s, 96 >> s) for s in range(4)]


def test_eval_pose_decoder_runs_the_convnet_path(mods, monkeypatch):
    calls = []
    cba, conv = _counting_convnet(calls)
    monkeypatch.setattr(mods.pose, "conv_bn_act", cba)
    monkeypatch.setattr(mods.pose, "conv", conv)
    _forbid_ops(monkeypatch)
    dec = mods.pose.ResNetLike().eval()
    axisangle, translation = dec(_features("pose"))
    convs = [m for m in dec.modules() if isinstance(m, nn.Conv2d)]
    assert len(calls) == len(convs) == 28 and set(map(id, calls)) == set(map(id, convs))
    assert axisangle.shape == translation.shape == (1, 2, 1, 3)


def test_train_mode_takes_the_autograd_nodes_and_never_the_convnet_path(mods, monkeypatch):
    """In train() the first layer of either decoder is an `ops` node; the detached, folded operands of uenc.convnet are never built."""
    from uenc import ops

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached
    def convnet(*a, **k):
        raise AssertionError("uenc.convnet ran in training mode")
    for mod in (mods.transdssl, mods.pose):
        monkeypatch.setattr(mod, "conv", convnet)
        monkeypatch.setattr(mod, "conv_bn_act", convnet)
    monkeypatch.setattr(ops, "linear", reached)
    with pytest.raises(Reached):
        mods.transdssl.TransDSSL(None, None).train().forward_features(_features("depth"))
    with pytest.raises(Reached):
        mods.pose.ResNetLike().train()(_features("pose"))


def test_motion_decoder_keeps_refusing_training_mode():
    from uenc import convnet
    bn = nn.BatchNorm2d(8).train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        convnet._bn_affine(bn)


def test_pose_block_passes_the_batchnorm_mode_on(mods, monkeypatch):
    """`train=bn.training`: a BatchNorm child put in eval() inside a decoder in train() runs on its running statistics."""
    from uenc import ops
    seen = []
    def conv_bn_act(x, weight, bn, *, kind, stride=1, residual=None, relu=False, train=False, out_dtype=torch.float32):
        seen.append((kind, stride, train, relu, residual is not None))
        return torch.zeros(x.shape[0], -(-x.shape[1] // stride), -(-x.shape[2] // stride), weight.shape[0])
    monkeypatch.setattr(ops, "conv_bn_act", conv_bn_act)
    blk = mods.pose.ResidualBlock(16, 16, stride=2).train()
    blk.forward_train(torch.zeros(1, 6, 8, 16))
    assert seen == [(3, 2, True, True, False), (1, 2, True, False, False), (3, 1, True, True, True)]
    seen.clear()
    for m in blk.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()
    assert blk.training
    blk.forward_train(torch.zeros(1, 6, 8, 16))
    assert [s[2] for s in seen] == [False, False, False]
    seen.clear()
    mods.pose.ResidualBlock(16, 16).train().forward_train(torch.zeros(1, 6, 8, 16))           # identity shortcut: the input is the residual
    assert seen == [(3, 1, True, True, False), (3, 1, True, True, True)]


# ---- OneFormer: refusals and dispatch -----------------------------------------------------------------------------------------------------
def _bare_model(with_decoders=True):
    import model  # noqa: F401
    from uenc.oneformer_model import OneFormer
    m = OneFormer.__new__(OneFormer)
    nn.Module.__init__(m)
    m.criterion = None
    m.depth_criterion = None
    m.pose_decoder = nn.Identity() if with_decoders else None
    m.sem_seg_head = nn.Module()
    m.sem_seg_head.depth_decoder = nn.Identity() if with_decoders else None
    return m


def _crit(**flags):
    from uenc.modeling.monodepth_loss import MonodepthLoss
    return MonodepthLoss(MF.make_cfg(2, 64, 96), **flags)


def _seq(**drop):
    d = {"type": "sequence", "left_image": None, "left_prev_image": None, "left_next_image": None, "K": None, "inv_K": None}
    for k in drop:
        del d[k]
    return d


def test_sequence_training_losses_refusals():
    m = _bare_model()
    with pytest.raises(RuntimeError, match="no depth criterion"):
        m.sequence_training_losses([_seq()])
    for flags in ({"bool_CmpFlow": True}, {"bool_MotMask": True}):
        m.set_depth_criterion(_crit(**flags))
        with pytest.raises(NotImplementedError, match="motion decoders"):
            m.sequence_training_losses([_seq()])
    m.set_depth_criterion(_crit())
    for key in ("left_image", "left_prev_image", "left_next_image", "K", "inv_K"):
        with pytest.raises(ValueError, match=f'"{key}"'):
            m.sequence_training_losses([_seq(), _seq(**{key: True})])
    bare = _bare_model(with_decoders=False).set_depth_criterion(_crit())
    with pytest.raises(NotImplementedError, match="without the sequence-branch decoders"):
        bare.sequence_training_losses([_seq()])
    assert m.set_depth_criterion(None).depth_criterion is None
    assert "depth_criterion" not in dict(m.named_children()) or m.depth_criterion is None


def test_forward_dispatch_table():
    """(mode, criteria, batch) -> training_losses | sequence_training_losses | inference."""
    m = _bare_model()
    calls = []
    m.training_losses = lambda batch, point_draws=None: calls.append("seg_losses") or {"loss_ce": 0}
    m.sequence_training_losses = lambda batch, tie_noise=None: calls.append("seq_losses") or {"loss_monodepth": 0}
    m._forward_segmentation = lambda batch: calls.append("seg_results") or [{}]
    m._forward_sequence = lambda batch: calls.append("seq_results") or {}
    seg = {"type": "segmentation", "pan_seg": None, "segments_info": []}
    seq, pair = _seq(), _seq(left_next_image=True)
    crit, dcrit = nn.Identity(), _crit()

    def reach(train, criterion, depth_criterion, batch):
        m.train(train)
        m.set_criterion(criterion)
        m.set_depth_criterion(depth_criterion)
        calls.clear()
        m(batch)
        return list(calls)

    assert reach(True, None, dcrit, [seq, seq]) == ["seq_losses"]
    assert reach(True, crit, dcrit, [seq]) == ["seq_losses"]
    assert reach(True, crit, dcrit, [seg]) == ["seg_losses"]
    assert reach(True, crit, None, [seq]) == ["seq_results"]                  # no depth criterion: inference, as before
    assert reach(True, None, dcrit, [seq, pair]) == ["seq_results"]           # a dict without the next frame: not a training batch
    assert reach(True, None, dcrit, [seg, seq]) == ["seg_results", "seq_results"]
    assert reach(True, None, dcrit, []) == []
    assert reach(False, crit, dcrit, [seq]) == ["seq_results"]                # eval mode
    assert reach(False, crit, dcrit, [seg]) == ["seg_results"]
    # a sequence dict mixed into a segmentation training batch still raises in training_losses
    del m.training_losses
    m.train()
    m.set_criterion(crit)
    m.set_depth_criterion(dcrit)
    with pytest.raises(ValueError, match="sequence"):
        m([seg, seq])


def test_reachable_through_the_reference_package_name():
    import model  # noqa: F401
    from model.modeling.pixel_decoder.transdssl import TransDSSL
    from model.modeling.pose_decoder.resnet_like_pose_decoder import ResNetLike
    from uenc.modeling.pixel_decoder import transdssl
    from uenc.modeling.pose_decoder import resnet_like_pose_decoder
    assert TransDSSL is transdssl.TransDSSL and ResNetLike is resnet_like_pose_decoder.ResNetLike


def test_fixture_is_what_the_generator_promises():
    z = SF.load()
    assert all(f"depth_grad:{n}" in z for n in SF.DEPTH_PARAMS) and all(f"depth_out:disp{s}" in z for s in range(4))
    for v in SF.POSE_VARIANTS:
        assert all(f"pose_{v}_grad:{n}" in z for n in SF.POSE_PARAMS) and all(f"pose_{v}_dx:{k}" in z for k in SF.INPUT_GRADS)
    assert int(z["pose_bn_train_buf:layer4.2.left.4.num_batches_tracked"]) == 1
    assert max(float(z[k]) for k in z if k.startswith("rounding:")) < 1e-5
    assert all(v.size <= 2 * SF.CAP for v in z.values())
    f = SF.features("pose")
    assert f["res5"].shape == (2, 1536, 4, 6) and abs(float(f["res2"].std()) - 1.0) < 0.01
