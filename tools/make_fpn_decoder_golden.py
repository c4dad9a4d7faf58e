"""tests/golden/fpn_pixel_decoder.npz: what the REFERENCE's BasePixelDecoder and TransformerEncoderPixelDecoder
(model/modeling/pixel_decoder/fpn.py) compute on the cases of tests/fpn_decoder_fixture.py.

Build container only (needs the reference checkout).  The reference's module is loaded through oracle.ref_loader and run as it is, in
eval mode, on the CPU, single-threaded; nothing of its text is restated.  Parameters come from tests/fpn_decoder_fixture.py (name-hashed,
not stored).

  x:<k>                 the inputs k = res2 .. res5
For each case c in (base, tenc):
  c_out:<k>             k = ms0, ms1, ms2 (the three multi-scale maps, coarse to fine), mask (the mask features), enc (tenc: the encoder
                        features); every n-th channel of the large ones (fpn_decoder_fixture.sub_out)
  c_loss                sum_k mean(out_k^2)
  c_grad:<name>         every parameter gradient (every n-th row of the large ones: fpn_decoder_fixture.sub_grad)
  c_env_err:<key>, c_env_cos:<key>   relative L2 error and cosine, against the above (the stored part), of the same quantity from the
                        reference run with every parameter rounded to bf16 and the input of every Conv2d / Linear rounded to bf16
  c_rounding_out, c_rounding_grad    largest relative L2 error of the reference in fp32 against itself in fp64; the file is written only
                        if every one is below 1e-5
  c_names / c_shapes    the whole state dict

    python tools/make_fpn_decoder_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import fpn_decoder_fixture as FX  # noqa: E402
from oracle import ref_loader  # noqa: E402

torch.set_num_threads(1)        # one summation order wherever the file is made


def run(mod, ns, case, dtype, x, bf16=False):
    net = FX.build(mod, case, ns.ShapeSpec)
    FX.fill_module(net, case)
    if bf16:
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(p.to(torch.bfloat16).float())
        for m in net.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                m.register_forward_pre_hook(lambda _, inp: (inp[0].to(torch.bfloat16).to(inp[0].dtype),))
    net = net.to(dtype).eval()
    q = FX.quantities(*net.forward_features({k: v.to(dtype) for k, v in x.items()}))
    loss = FX.loss_of(q)
    loss.backward()
    q = {k: v.detach() for k, v in q.items()}
    q["loss"] = loss.detach()
    for n, p in net.named_parameters():
        q["grad:" + n] = p.grad if p.grad is not None else torch.zeros_like(p)
    return q, net


def main():
    ns = ref_loader.load()
    mod = ref_loader._load("model.modeling.pixel_decoder.fpn", "modeling/pixel_decoder/fpn.py")
    x = FX.inputs()
    d = {"x:" + k: v.numpy() for k, v in x.items()}
    for c in FX.CASES:
        q32, net = run(mod, ns, c, torch.float32, x)
        q64, _ = run(mod, ns, c, torch.float64, x)
        env, _ = run(mod, ns, c, torch.float32, x, bf16=True)
        r_out = max(FX.rel(q32[k], q64[k]) for k in q32 if not k.startswith("grad:"))
        r_grad = max(FX.rel(q32[k], q64[k]) for k in q32 if k.startswith("grad:"))
        print(f"{c}: reference fp32 vs fp64: outputs {r_out:.3g}, gradients {r_grad:.3g}")
        if not (r_out < 1e-5 and r_grad < 1e-5):
            raise SystemExit("the reference's own rounding on this case is too large: not written")
        d[c + "_rounding_out"], d[c + "_rounding_grad"] = np.float64(r_out), np.float64(r_grad)
        errs = {}
        for k, v in q32.items():
            d[f"{c}_{k}"] = FX.stored(k, v).numpy()
            se, sv = FX.stored(k, env[k]), FX.stored(k, v)
            d[f"{c}_env_err:{k}"], d[f"{c}_env_cos:{k}"] = np.float64(FX.rel(se, sv)), np.float64(FX.cos(se, sv))
            errs[k] = d[f"{c}_env_err:{k}"]
        eo = [v for k, v in errs.items() if not k.startswith("grad:")]
        eg = sorted(v for k, v in errs.items() if k.startswith("grad:"))
        print(f"   envelope: outputs {min(eo):.3g} .. {max(eo):.3g}; gradients median {eg[len(eg) // 2]:.3g}, worst {eg[-1]:.3g}")
        sd = net.state_dict()
        d[c + "_names"] = np.array(list(sd.keys()))
        d[c + "_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    np.savez_compressed(FX.GOLDEN, **d)
    print(f"wrote {FX.GOLDEN}: {os.path.getsize(FX.GOLDEN)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
