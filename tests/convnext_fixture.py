"""Shared by tools/make_convnext_golden.py and the ConvNeXt tests: the cases of tests/golden/convnext.npz and their parameters.

The parameters are not stored (the `net` case has 1.4 M of them): both sides regenerate them from the state-dict name with the
project's name-hashed generator (oracle/fill.py), with distributions that exercise bias, layer-scale and LayerNorm paths:
matrices / filters N(0, 0.05), LayerNorm weights and layer-scale gamma uniform in [0.5, 1.5], biases uniform in [-0.2, 0.2].
"""
import os

import numpy as np
import torch

from oracle import fill

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext.npz")

NET = dict(in_chans=3, depths=[2, 1, 2, 1], dims=[40, 80, 160, 320], drop_path_rate=0.0, layer_scale_init_value=1.0)
NET_X = (2, 3, 64, 96)
BLOCK_DIM, BLOCK_X = 40, (2, 40, 5, 9)
NOLS_DIM, NOLS_X = 16, (1, 16, 3, 5)

# parameters of `net` whose gradient the file holds
NAMED = ["downsample_layers.0.0.weight", "stages.0.0.dwconv.weight", "stages.0.0.dwconv.bias", "stages.0.0.norm.weight", "stages.0.1.gamma",
         "stages.0.0.pwconv1.weight", "stages.2.1.pwconv2.weight", "downsample_layers.2.1.weight", "stages.3.0.dwconv.weight", "norm3.weight"]
# the two largest of them are stored as every n-th output row (the file stays under 1 MB)
ROW_STEP = {"stages.2.1.pwconv2.weight": 4, "downsample_layers.2.1.weight": 2}


def tensor_for(name: str, shape) -> torch.Tensor:
    shape = tuple(int(s) for s in shape)
    rng = fill._rng("convnext/" + name)
    leaf = name.split(".")[-1]
    if len(shape) >= 2:
        out = 0.05 * rng.standard_normal(shape)
    elif leaf in ("weight", "gamma"):
        out = rng.uniform(0.5, 1.5, shape)
    else:
        out = rng.uniform(-0.2, 0.2, shape)
    return torch.from_numpy(np.asarray(out, dtype=np.float32))


@torch.no_grad()
def fill_module(module: torch.nn.Module, prefix: str) -> None:
    for name, p in module.named_parameters():
        p.copy_(tensor_for(prefix + name, p.shape))


def input_for(name: str, shape) -> torch.Tensor:
    """Inputs and upstream gradients: multiples of 1/64 in [-2, 2) (they compress well in the file)."""
    rng = fill._rng("convnext/input/" + name)
    return torch.from_numpy((rng.integers(-128, 128, tuple(shape)) / 64.0).astype(np.float32))


def rows(name: str, g):
    return g[::ROW_STEP[name]] if name in ROW_STEP else g


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def cos(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu().flatten(), torch.as_tensor(b).detach().double().cpu().flatten()
    return float(a @ b / (a.norm() * b.norm()).clamp_min(1e-300))


def load():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
