"""Shared by tools/make_sequence_train_golden.py and tests/test_sequence_train_gpu.py: the case of tests/golden/sequence_train.npz.
Generator of the file: `python tools/make_sequence_train_golden.py` (recorded here; tests/golden/MANIFEST.json is left as it is).

The reference's own `TransDSSL` and `ResNetLike` (build machine only) and the product's run the same case: weights from
`oracle.fill.fill_module` under the state-dict prefixes of the full model, Swin-T-shaped features of a 128 x 192 frame, B = 2, and the
cotangents of a fixed linear functional of the outputs, all drawn with `oracle.fill.tensor_for` from their names alone -- nothing of
them is stored.  At this size the last pose layer's BatchNorm sees 2 * 2 * 3 = 12 samples per channel.

    scalar = sum_s <disp_s, c_s>   (depth decoder)        scalar = <axisangle, c_a> + <translation, c_t>   (pose decoder)

The pose decoder runs in two variants: "bn_train" (BatchNorm in training mode: batch statistics, running ones updated) and "bn_eval" (the
decoder in train() with its BatchNorm children in eval(): running statistics, not updated).

Stored per decoder: the outputs, the gradients of the parameters named below and of the `res5` / `res4` inputs, the global L2 norm of all
parameter gradients, and for "bn_train" the updated running statistics of two BatchNorms.  A tensor with more than CAP values is stored
as every n-th value of its flattened form (`sub`), which is the part a test compares.

Every stored quantity is one the reference itself reproduces: the generator runs the reference in fp32 and in float64 and refuses to write
the file unless each agrees to 1e-5 relative L2.  `refinenet0.resConfUnit1.conv1.weight` is not in the list for that reason: its gradient
passes the ReLU mask of 3.1 M activations of the full-resolution map, a few of which sit within fp32 rounding of zero, and the reference's
own fp32 gradient is 5.5e-4 away from its float64 one; the unit's second convolution is stored in its place."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_train.npz")

B, FRAME = 2, (128, 192)
SWIN_T_CH = (96, 192, 384, 768)
STRIDES = (4, 8, 16, 32)
LEVELS = ("res2", "res3", "res4", "res5")
DEPTH_PREFIX, POSE_PREFIX = "sem_seg_head.depth_decoder.", "pose_decoder."
POSE_VARIANTS = ("bn_train", "bn_eval")
CAP = 2048

DEPTH_PARAMS = [
    "layers.layer1_rn.weight", "layers.layer4_rn.weight",
    "layers.refinenet4.resConfUnit2.conv1.weight", "layers.refinenet4.out_conv.weight", "layers.refinenet4.out_conv.bias",
    "layers.refinenet3.en_atten.weight", "layers.refinenet2.en_atten.weight", "layers.refinenet1.en_atten.weight",
    "layers.refinenet0.en_atten.weight", "layers.refinenet0.en_atten.bias",
    "layers.refinenet2.resConfUnit2.conv2.weight", "layers.refinenet2.resConfUnit2.conv2.bias",
    "layers.refinenet0.resConfUnit1.conv2.weight", "layers.refinenet0.out_conv.weight",
    "layers.output_conv4.0.weight", "layers.output_conv.1.weight", "layers.output_conv.1.bias",
]
POSE_PARAMS = [
    "layer1.0.weight", "layer1.1.left.0.weight", "layer1.1.left.1.weight", "layer1.1.shortcut.0.weight", "layer1.2.left.3.weight",
    "layer2.2.left.3.weight", "layer3.1.left.0.weight", "layer4.0.weight", "layer4.0.bias", "layer4.2.left.3.weight",
    "layer4.2.left.4.weight", "layer4.2.left.4.bias", "squeeze.weight", "squeeze.bias", "convs.pose_0.weight", "convs.pose_2.weight",
    "convs.pose_2.bias",
]
POSE_BNS = ["layer1.1.left.1", "layer4.2.left.4"]
INPUT_GRADS = ("res5", "res4")


def _normal(name, shape):
    """N(0, 1) values from the name alone (a 1-D non-"weight" entry of oracle.fill is 0.1 * N(0, 1))."""
    n = int(np.prod(shape))
    return (fill.tensor_for("sequence_train/" + name + ".x", (n,)) * 10.0).view(*shape)


def features(which):
    """which = "depth": the current frame's Swin-T features; "pose": the concatenated features of a frame pair (twice the channels)."""
    mult = 2 if which == "pose" else 1
    return {k: _normal(f"{which}/{k}", (B, c * mult, FRAME[0] // s, FRAME[1] // s)) for k, c, s in zip(LEVELS, SWIN_T_CH, STRIDES)}


def cotangents():
    out = {f"disp{s}": _normal(f"c/disp{s}", (B, 1, FRAME[0] >> s, FRAME[1] >> s)) for s in range(4)}
    out["axisangle"] = _normal("c/axisangle", (B, 2, 1, 3))
    out["translation"] = _normal("c/translation", (B, 2, 1, 3))
    return out


def sub(t):
    """The stored part of a tensor: every n-th value of its flattened form, n the smallest step that brings it to CAP values or fewer."""
    t = torch.as_tensor(t).detach().reshape(-1)
    return t[::max(1, -(-t.numel() // CAP))]


def fill_decoders(depth, pose):
    if depth is not None:
        fill.fill_module(depth, DEPTH_PREFIX)
    if pose is not None:
        fill.fill_module(pose, POSE_PREFIX)
        for m in pose.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.num_batches_tracked.zero_()


def set_pose_variant(pose, variant):
    pose.train()
    if variant == "bn_eval":
        for m in pose.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.eval()
    return pose


def depth_scalar(disps, cot):
    """disps: {("disp", s): (B, 1, h, w)}."""
    return sum((disps[("disp", s)].float() * cot[f"disp{s}"].to(disps[("disp", s)].device)).sum() for s in range(4))


def pose_scalar(axisangle, translation, cot):
    return (axisangle.float() * cot["axisangle"].to(axisangle.device)).sum() + (translation.float() * cot["translation"].to(translation.device)).sum()


def grad_norm(module):
    return float(torch.sqrt(sum(p.grad.detach().double().square().sum() for p in module.parameters() if p.grad is not None)))


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the product's two module trees through ATen, sharing the modules' parameters (the bf16-autocast envelope of the tests, the ATen
# legs of tools/sequence_train_bench.py)
def aten_rcu(u, x):
    return u.conv2(F.relu(u.conv1(F.relu(x)))) + x


def aten_fusion(b, *xs):
    if len(xs) == 2:
        res = xs[0] + xs[1]
        out = aten_rcu(b.resConfUnit2, res * F.softmax(b.en_atten(aten_rcu(b.resConfUnit1, xs[1])), dim=1)) + res
    else:
        out = aten_rcu(b.resConfUnit2, xs[0])
    return b.out_conv(F.interpolate(out, scale_factor=2, mode="bilinear", align_corners=True))


def aten_depth(m, f):
    L = m.layers
    l1, l2, l3, l4 = L.layer1_rn(f["res2"]), L.layer2_rn(f["res3"]), L.layer3_rn(f["res4"]), L.layer4_rn(f["res5"])
    p4 = aten_fusion(L.refinenet4, l4)
    p3 = aten_fusion(L.refinenet3, p4, l3)
    p2 = aten_fusion(L.refinenet2, p3, l2)
    p1 = aten_fusion(L.refinenet1, p2, l1)
    p0 = aten_fusion(L.refinenet0, p1, F.interpolate(l1, scale_factor=2, mode="bilinear", align_corners=True))
    return {("disp", s): m.attn_depth(head(p)) for s, head, p in ((3, L.output_conv4, p3), (2, L.output_conv3, p2), (1, L.output_conv2, p1),
                                                                     (0, L.output_conv, p0))}


def aten_pose(m, f):
    def run(seq, x):
        x = seq[0](x)
        for blk in list(seq)[1:]:
            x = F.relu(blk.left(x) + (blk.shortcut(x) if len(blk.shortcut) else x))
        return x
    out = run(m.layer1, f["res2"])
    for layer, k in ((m.layer2, "res3"), (m.layer3, "res4"), (m.layer4, "res5")):
        out = run(layer, torch.cat([out, f[k]], 1))
    out = F.relu(m.squeeze(out))
    out = m.convs["pose_2"](F.relu(m.convs["pose_1"](F.relu(m.convs["pose_0"](out)))))
    out = 0.01 * out.mean(3).mean(2).view(-1, m.num_frames_to_predict_for, 1, 6)
    return out[..., :3], out[..., 3:]


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
