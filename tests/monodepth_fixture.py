"""Shared by the MonodepthLoss tests and tools/make_monodepth_golden.py: the cases of tests/golden/monodepth_loss.npz, the three flag sets,
and one function that runs a MonodepthLoss-like class on a case and returns its loss dictionary, gradients and `outputs`."""
import os
import types

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monodepth_loss.npz")
CASES = {"a": (2, 24, 40), "b": (1, 16, 72)}            # B, H, W; the scale-3 maps are 3 x 5 and 2 x 9
FRAMES = (-1, 1)
SCALES = (0, 1, 2, 3)
OFF = dict(bool_MotMask=False, bool_CmpFlow=False, bool_automask=False, move_Depth=False, move_CmpFlow=False, move_MotMask=False,
           step=0, phrage="pretrain")
FLAGSETS = {
    "rigid": dict(OFF),
    "automask": dict(OFF, bool_automask=True),
    "full": dict(bool_MotMask=True, bool_CmpFlow=True, bool_automask=True, move_Depth=True, move_CmpFlow=True, move_MotMask=True,
                 step=40000, phrage="finetune"),
}
SEED_CHECK_REL_L2 = 2.5e-5


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    n = float(np.linalg.norm(b))
    return float(np.linalg.norm(a - b)) / n if n > 0 else float(np.linalg.norm(a - b))


def load():
    z = np.load(GOLDEN, allow_pickle=False)
    return {k: z[k] for k in z.files}


def make_cfg(B, H, W, device="cpu"):
    ns = types.SimpleNamespace
    return ns(SOLVER=ns(IMS_PER_BATCH=B), DATASETS=ns(TRAIN=("kitti",)), INPUT=ns(DEPTH_CROP=ns(SIZE=(H, W))), MODEL=ns(DEVICE=device))


def leaf_names(flagset):
    """The differentiable inputs a flag set reaches."""
    names = [f"disp{s}" for s in SCALES] + [f"T{f}" for f in FRAMES]
    if FLAGSETS[flagset]["bool_CmpFlow"]:
        names += [f"cflow{f}_{s}" for f in FRAMES for s in SCALES]
    if FLAGSETS[flagset]["bool_MotMask"]:
        names += [f"mask{f}_{s}" for f in FRAMES for s in SCALES] + [f"prob{f}_{s}" for f in FRAMES for s in SCALES]
    return names


def make_inputs(z, case, dtype=torch.float32, device="cpu"):
    """-> outputs, targets, leaves (name -> tensor with requires_grad)."""
    B, H, W = CASES[case]
    t = lambda name: torch.from_numpy(z[f"{case}_{name}"]).to(device=device, dtype=dtype)
    leaves, outputs = {}, {}

    def leaf(name):
        leaves[name] = t(name).requires_grad_(True)
        return leaves[name]

    for s in SCALES:
        outputs[("disp", 0, s)] = leaf(f"disp{s}")
        for f in FRAMES:
            outputs[("complete_flow", f, s)] = leaf(f"cflow{f}_{s}")
            outputs[("motion_mask", f, s)] = leaf(f"mask{f}_{s}")
            outputs[("motion_prob", f, s)] = leaf(f"prob{f}_{s}")
    for f in FRAMES:
        outputs[("cam_T_cam", 0, f)] = leaf(f"T{f}")
    K, inv_K = t("K"), t("invK")
    color = {f: t(f"color{f}") for f in (-1, 0, 1)}
    targets = [dict({("color", f, 0): color[f][b] for f in (-1, 0, 1)}, K=K[b], inv_K=inv_K[b]) for b in range(B)]
    return outputs, targets, leaves


def run(cls, z, case, flagset, dtype=torch.float32, device="cpu", ctor_kwargs=None, set_attrs=False, backward=True):
    """Runs generate_images_pred + compute_losses of `cls` with the recorded noise / sample indices.  `set_attrs`: assign the flags as
    attributes after construction (the reference's protocol) instead of passing keywords."""
    B, H, W = CASES[case]
    flags = FLAGSETS[flagset]
    outputs, targets, leaves = make_inputs(z, case, dtype, device)
    cfg = make_cfg(B, H, W, device)
    if set_attrs:
        m = cls(cfg, **(ctor_kwargs or {}))
        for k, v in flags.items():
            setattr(m, k, v)
    else:
        m = cls(cfg, **flags, **(ctor_kwargs or {}))
    kw = {}
    if not set_attrs:
        if flags["bool_automask"]:
            kw["tie_noise"] = [torch.from_numpy(z[f"{case}_{flagset}_noise{s}"]).to(device=device, dtype=dtype) for s in SCALES]
        if flags["bool_MotMask"]:
            kw["ground_samples"] = [torch.from_numpy(z[f"{case}_{flagset}_ground{s}"]).to(device) for s in SCALES]
    m.generate_images_pred(outputs, targets)
    losses = m.compute_losses(targets, outputs, **kw)
    grads = {}
    if backward:
        names = leaf_names(flagset)
        got = torch.autograd.grad(losses["loss"], [leaves[n] for n in names], allow_unused=True)
        grads = {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, got)}
    return losses, grads, outputs


def to_numpy(v):
    return v.detach().double().cpu().numpy() if torch.is_tensor(v) else np.float64(v)


def key_name(k):
    return "/".join(str(p) for p in k) if isinstance(k, tuple) else str(k)
