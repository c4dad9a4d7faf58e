"""Shared by tools/make_resnet_golden.py and the ResNet tests: the cases of tests/golden/resnet.npz and their parameters.

The parameters and buffers are not stored: both sides regenerate them from the state-dict name with the project's name-hashed generator
(oracle/fill.py).  Convolution weights are N(0, 2 / fan_in) (activations keep their scale through the depth), BatchNorm weights and
running variances uniform in [0.75, 1.25], biases and running means uniform in [-0.1, 0.1] (at these ranges the reference's own fp32
rounding of the train-mode gradients stays below the 1e-5 the file is written at); batch counters stay 0.

Cases (both nets take x (2, 3, 45, 70); map sizes 23x35, 12x18, 6x9, 3x5, 2x3; all five outputs are asked for):
  basic   stem 16, BasicBlock stages 16->16 x2, 16->32 x2 (stride 2), 32->64 (stride 2), 64->128 (stride 2)
  bottle  stem 16, BottleneckBlock stages 16->32 x2 (bottleneck 8), 32->64 (16), 64->128 (32), 128->256 (64), each later stage stride 2
          in its 3x3 convolution
each run in eval mode (`<net>_eval`) and in train mode (`<net>_train`), and `frozen`: `basic` after freeze(2), run in train mode.
"""
import os

import numpy as np
import torch

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resnet.npz")
CFG_BASE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg_resnet_base.json")

X = (2, 3, 45, 70)
OUTS = ["stem", "res2", "res3", "res4", "res5"]
NETS = ["basic", "bottle"]
CASES = ["basic_eval", "basic_train", "bottle_eval", "bottle_train"]
SIZES = {"stem": (23, 35), "res2": (12, 18), "res3": (6, 9), "res4": (3, 5), "res5": (2, 3)}

# the file stays under 1 MB: an output with more than OUT_CAP values is stored as every n-th channel, a gradient with more than GRAD_CAP as
# every n-th row (n = the smallest step that gets it under the cap).  The envelope figures are taken on the stored part, the quantity a test
# compares (a few rows of a weight gradient can be several times further off than the whole: one flipped ReLU moves a whole row); the
# reference's own rounding figures on the whole tensors
OUT_CAP, GRAD_CAP = 4096, 2048


def build(mod, which: str, norm: str = "BN"):
    """The case's net from the module `mod` (the reference's resnet.py or uenc.modeling.backbone.resnet: same constructors)."""
    R = mod.ResNet
    stem = mod.BasicStem(3, 16, norm=norm)
    if which == "basic":
        B = mod.BasicBlock
        stages = [R.make_stage(B, 2, in_channels=16, out_channels=16, stride_per_block=[1, 1], norm=norm),
                  R.make_stage(B, 2, in_channels=16, out_channels=32, stride_per_block=[2, 1], norm=norm),
                  R.make_stage(B, 1, in_channels=32, out_channels=64, stride_per_block=[2], norm=norm),
                  R.make_stage(B, 1, in_channels=64, out_channels=128, stride_per_block=[2], norm=norm)]
    else:
        B = mod.BottleneckBlock
        kw = dict(norm=norm, stride_in_1x1=False)
        stages = [R.make_stage(B, 2, in_channels=16, out_channels=32, bottleneck_channels=8, stride_per_block=[1, 1], **kw),
                  R.make_stage(B, 1, in_channels=32, out_channels=64, bottleneck_channels=16, stride_per_block=[2], **kw),
                  R.make_stage(B, 1, in_channels=64, out_channels=128, bottleneck_channels=32, stride_per_block=[2], **kw),
                  R.make_stage(B, 1, in_channels=128, out_channels=256, bottleneck_channels=64, stride_per_block=[2], **kw)]
    return R(stem, stages, out_features=list(OUTS))


def tensor_for(name: str, shape) -> torch.Tensor:
    shape = tuple(int(s) for s in shape)
    rng = fill._rng("resnet/" + name)
    leaf = name.split(".")[-1]
    if len(shape) == 4:
        out = np.sqrt(2.0 / (shape[1] * shape[2] * shape[3])) * rng.standard_normal(shape)
    elif leaf in ("weight", "running_var"):
        out = rng.uniform(0.75, 1.25, shape)
    else:
        out = rng.uniform(-0.1, 0.1, shape)
    return torch.from_numpy(np.asarray(out, dtype=np.float32))


@torch.no_grad()
def fill_module(module: torch.nn.Module, prefix: str) -> None:
    """Parameters and floating-point buffers by name (the same values whether a norm is a BatchNorm or already frozen)."""
    for name, t in list(module.named_parameters()) + list(module.named_buffers()):
        if t.is_floating_point():
            t.copy_(tensor_for(prefix + name, t.shape))


def input_x() -> torch.Tensor:
    """Multiples of 1/64 in [-2, 2) (they compress well in the file)."""
    rng = fill._rng("resnet/input/x")
    return torch.from_numpy((rng.integers(-128, 128, X) / 64.0).astype(np.float32))


def step(numel: int, cap: int) -> int:
    return max(1, -(-int(numel) // cap))


def sub_out(t):
    """The stored part of an output (B, C, H, W): every n-th channel."""
    return t[:, ::step(t.numel(), OUT_CAP)]


def sub_grad(t):
    """The stored part of a parameter gradient: every n-th row."""
    return t[::step(t.numel(), GRAD_CAP)]


def loss_of(outs):
    return sum(outs[k].square().mean() for k in OUTS)


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def cos(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).detach().double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


def rows(name: str, g):
    return sub_grad(g)


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
