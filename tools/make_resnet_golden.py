"""tests/golden/resnet.npz: what the REFERENCE's ResNet (model/modeling/backbone/resnet.py) computes on the cases of tests/resnet_fixture.py.

Build container only (needs the reference checkout).  The reference's module is loaded through oracle.ref_loader and run as it is, on
the CPU, single-threaded; nothing of its text is restated.  On top of ref_loader's name holders this file adds the few more of
detectron2 that resnet.py imports, with detectron2's documented behaviour: `detectron2.layers.CNNBlockBase` (with `freeze()`),
`ModulatedDeformConv = None`, a `get_norm` that knows "BN" / "FrozenBN", and `detectron2.modeling.backbone.{backbone, build}`.
Parameters and buffers come from tests/resnet_fixture.py (name-hashed, not stored).

For each case c in resnet_fixture.CASES (basic | bottle, eval | train):
  c_out:<k>            the outputs k = stem, res2 .. res5 (every n-th channel of the large ones: resnet_fixture.sub_out)
  c_loss               sum_k mean(out_k^2)
  c_grad:<name>        every parameter gradient (every n-th row of the large ones: resnet_fixture.sub_grad)
  c_buf:<name>         train mode: running_mean / running_var / num_batches_tracked after the step
  c_env_err:<key>, c_env_cos:<key>   relative L2 error and cosine, against the above (the stored part), of the same quantity from the reference run with every
                       parameter rounded to bf16 and the input of every Conv2d rounded to bf16 (<key> = out:<k>, loss, grad:<name>)
  c_rounding_out, c_rounding_grad    largest relative L2 error of the reference in fp32 against itself in fp64; the file is written only if
                       every one is below 1e-5
<net>_names / <net>_shapes: the whole state dict.  x: the input.
frozen_*: the `basic` net after freeze(2), train mode: frozen_out:<k>, frozen_loss, frozen_grad:<name> for the parameters that still receive
a gradient, frozen_trainable (their names), frozen_names / frozen_shapes (no num_batches_tracked under the frozen stages).

    python tools/make_resnet_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import resnet_fixture as RF  # noqa: E402
from oracle import ref_loader  # noqa: E402

torch.set_num_threads(1)        # one summation order wherever the file is made


def load_reference():
    from uenc.d2 import CNNBlockBase, FrozenBatchNorm2d          # detectron2's behaviour (not the reference's), as the product's shim has it
    ref_loader._install_stubs()
    layers = sys.modules["detectron2.layers"]

    def get_norm(norm, out_channels):
        if norm is None or norm == "":
            return None
        return {"BN": nn.BatchNorm2d, "FrozenBN": FrozenBatchNorm2d, "GN": lambda c: nn.GroupNorm(32, c)}[norm](out_channels)
    layers.CNNBlockBase, layers.ModulatedDeformConv, layers.get_norm = CNNBlockBase, None, get_norm
    d2m = sys.modules["detectron2.modeling"]
    ref_loader._mod("detectron2.modeling.backbone")
    ref_loader._mod("detectron2.modeling.backbone.backbone", Backbone=d2m.Backbone)
    ref_loader._mod("detectron2.modeling.backbone.build", BACKBONE_REGISTRY=d2m.BACKBONE_REGISTRY)
    return ref_loader._load("model.modeling.backbone.resnet", "modeling/backbone/resnet.py")


def run(mod, which, mode, dtype, x, bf16=False, freeze_at=0):
    net = RF.build(mod, which)
    net.freeze(freeze_at)
    RF.fill_module(net, which + ".")
    if bf16:
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(p.to(torch.bfloat16).float())
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                m.register_forward_pre_hook(lambda _, inp: (inp[0].to(torch.bfloat16).to(inp[0].dtype),))
    net = net.to(dtype)
    net.train(mode == "train")
    outs = net(x.to(dtype))
    loss = RF.loss_of(outs)
    loss.backward()
    q = {"out:" + k: outs[k].detach() for k in RF.OUTS}
    q["loss"] = loss.detach()
    for n, p in net.named_parameters():
        if p.grad is not None:
            q["grad:" + n] = p.grad
    return q, net


def stored(key, t):
    return RF.sub_out(t) if key.startswith("out:") else (RF.sub_grad(t) if key.startswith("grad:") else t)


def main():
    mod = load_reference()
    x = RF.input_x()
    d = {"x": x.numpy()}
    for which in RF.NETS:
        for mode in ("eval", "train"):
            c = f"{which}_{mode}"
            q32, net = run(mod, which, mode, torch.float32, x)
            q64, _ = run(mod, which, mode, torch.float64, x)
            env, _ = run(mod, which, mode, torch.float32, x, bf16=True)
            r_out = max(RF.rel(q32[k], q64[k]) for k in q32 if not k.startswith("grad:"))
            r_grad = max(RF.rel(q32[k], q64[k]) for k in q32 if k.startswith("grad:"))
            print(f"{c}: reference fp32 vs fp64: outputs {r_out:.3g}, gradients {r_grad:.3g}")
            if not (r_out < 1e-5 and r_grad < 1e-5):
                raise SystemExit("the reference's own rounding on this case is too large: not written")
            d[c + "_rounding_out"], d[c + "_rounding_grad"] = np.float64(r_out), np.float64(r_grad)
            errs = {}
            for k, v in q32.items():
                d[f"{c}_{k}"] = stored(k, v).numpy()
                # the envelope of the STORED part: what a test can compare is the stored rows / channels, and one flipped ReLU moves a whole
                # row of a weight gradient, so the figure of a few rows can be several times that of the whole tensor
                se, sv = stored(k, env[k]), stored(k, v)
                d[f"{c}_env_err:{k}"], d[f"{c}_env_cos:{k}"] = np.float64(RF.rel(se, sv)), np.float64(RF.cos(se, sv))
                errs[k] = d[f"{c}_env_err:{k}"]
            eo = [v for k, v in errs.items() if not k.startswith("grad:")]
            eg = sorted(v for k, v in errs.items() if k.startswith("grad:"))
            print(f"   envelope: outputs {min(eo):.3g} .. {max(eo):.3g}; gradients median {eg[len(eg) // 2]:.3g}, worst {eg[-1]:.3g}")
            if mode == "train":
                for n, b in net.named_buffers():
                    d[f"{c}_buf:{n}"] = b.detach().numpy()
            sd = net.state_dict()
            d[which + "_names"] = np.array(list(sd.keys()))
            d[which + "_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    q, net = run(mod, "basic", "train", torch.float32, x, freeze_at=2)
    for k, v in q.items():
        d["frozen_" + k] = stored(k, v).numpy()
    d["frozen_trainable"] = np.array([n for n, p in net.named_parameters() if p.requires_grad])
    sd = net.state_dict()
    d["frozen_names"] = np.array(list(sd.keys()))
    d["frozen_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])

    import json
    import yaml                                     # the reference's base YAML: its MODEL.BACKBONE / MODEL.RESNETS settings, nothing else
    base = os.path.join(ref_loader.REF_ROOT, "configs", "cityscapes", "Base-Cityscapes-UnifiedSegmentation.yaml")

    class L(yaml.SafeLoader):
        pass
    L.add_constructor("tag:yaml.org,2002:python/object/apply:eval", lambda loader, node: None)
    with open(base) as f:
        y = yaml.load(f, Loader=L)
    with open(RF.CFG_BASE, "w") as f:
        json.dump({"MODEL": {"BACKBONE": y["MODEL"]["BACKBONE"], "RESNETS": y["MODEL"]["RESNETS"]}}, f, indent=1, sort_keys=True)
        f.write("\n")

    np.savez_compressed(RF.GOLDEN, **d)
    print(f"wrote {RF.GOLDEN}: {os.path.getsize(RF.GOLDEN)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
