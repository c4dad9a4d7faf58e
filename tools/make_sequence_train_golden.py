"""tests/golden/sequence_train.npz: what the REFERENCE's TransDSSL and ResNetLike compute, forward and backward, in training mode on the case
of tests/sequence_train_fixture.py.

Build machine only (needs the reference checkout); never run where the GPU tests run.  The reference's modules are loaded through
`oracle.ref_loader.load_sequence()` and run as they are, on the CPU in fp32, single-threaded; nothing of their text is restated.  Weights
(`oracle.fill.fill_module`), features and cotangents (`oracle.fill.tensor_for`) are regenerated from names by both sides and not stored.

  depth_out:disp<s>                 the four disparities                      (every stored tensor: sequence_train_fixture.sub)
  depth_grad:<name>, depth_dx:<res5|res4>, depth_grad_norm
  pose_<variant>_out:<axisangle|translation>, pose_<variant>_grad:<name>, pose_<variant>_dx:<res5|res4>, pose_<variant>_grad_norm
  pose_bn_train_buf:<bn>.<running_mean|running_var|num_batches_tracked>        after the step
  rounding:<key>                    relative L2 error of the fp32 run against the same run in float64; the file is written only if every
                                    one is below 1e-5 (a tenth of the 1e-4 the fp32 mode is held to)

    python tools/make_sequence_train_golden.py
"""
import os
import sys
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import sequence_train_fixture as SF  # noqa: E402
from oracle import ref_loader  # noqa: E402

torch.set_num_threads(1)        # one summation order wherever the file is made


def run_depth(ref, dtype):
    depth = ref.transdssl.TransDSSL(None, None)
    SF.fill_decoders(depth, None)
    depth.to(dtype).train()
    feats = {k: v.to(dtype).requires_grad_(True) for k, v in SF.features("depth").items()}
    cot = {k: v.to(dtype) for k, v in SF.cotangents().items()}
    disps = depth.forward_features(feats)
    sum((disps[("disp", s)] * cot[f"disp{s}"]).sum() for s in range(4)).backward()
    named = dict(depth.named_parameters())
    out = {f"depth_out:disp{s}": disps[("disp", s)] for s in range(4)}
    out.update({f"depth_grad:{n}": named[n].grad for n in SF.DEPTH_PARAMS})
    out.update({f"depth_dx:{k}": feats[k].grad for k in SF.INPUT_GRADS})
    out["depth_grad_norm"] = torch.tensor(SF.grad_norm(depth))
    return out


def run_pose(ref, variant, dtype):
    pose = ref.pose.ResNetLike()
    SF.fill_decoders(None, pose)
    SF.set_pose_variant(pose.to(dtype), variant)
    feats = {k: v.to(dtype).requires_grad_(True) for k, v in SF.features("pose").items()}
    cot = {k: v.to(dtype) for k, v in SF.cotangents().items()}
    axisangle, translation = pose(feats)
    ((axisangle * cot["axisangle"]).sum() + (translation * cot["translation"]).sum()).backward()
    named, bufs = dict(pose.named_parameters()), dict(pose.named_buffers())
    pre = f"pose_{variant}_"
    out = {pre + "out:axisangle": axisangle, pre + "out:translation": translation}
    out.update({pre + f"grad:{n}": named[n].grad for n in SF.POSE_PARAMS})
    out.update({pre + f"dx:{k}": feats[k].grad for k in SF.INPUT_GRADS})
    out[pre + "grad_norm"] = torch.tensor(SF.grad_norm(pose))
    for bn in SF.POSE_BNS:
        for leaf in ("running_mean", "running_var", "num_batches_tracked"):
            t = bufs[f"{bn}.{leaf}"]
            if variant == "bn_train":
                out[pre + f"buf:{bn}.{leaf}"] = t
            else:                       # BatchNorm children in eval(): the statistics are the filled ones, the counter stays 0
                assert leaf != "num_batches_tracked" or int(t) == 0
    return out


def main():
    warnings.filterwarnings("ignore")
    assert ref_loader.available(), "needs the reference checkout"
    ref = ref_loader.load_sequence()
    arrs, rounding = {}, {}
    for run in (lambda dt: run_depth(ref, dt), *(lambda dt, v=v: run_pose(ref, v, dt) for v in SF.POSE_VARIANTS)):
        r32, r64 = run(torch.float32), run(torch.float64)
        for k, v in r32.items():
            if "num_batches_tracked" not in k:
                rounding[k] = SF.rel(v, r64[k])
            arrs[k] = SF.sub(v).numpy() if v.dim() > 0 else v.numpy()
    worst = max(rounding, key=rounding.get)
    print(f"largest fp32-vs-float64 relative error of the reference: {rounding[worst]:.3g} ({worst})")
    assert rounding[worst] < 1e-5, (worst, rounding[worst])
    arrs.update({"rounding:" + k: np.float64(v) for k, v in rounding.items()})
    np.savez_compressed(SF.GOLDEN, **arrs)
    print(f"sequence_train: {len(arrs)} entries, {os.path.getsize(SF.GOLDEN) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
