"""tests/golden/convnext.npz: what the REFERENCE's ConvNeXt (model/modeling/backbone/convnext.py) computes on three small cases.

Build container only (needs the reference checkout).  The reference's module is loaded through oracle.ref_loader and run as it is, on
the CPU, single-threaded; nothing of its text is restated.  Parameters come from tests/convnext_fixture.py (name-hashed, not stored).

  net    ConvNeXt(3, depths [2,1,2,1], dims [40,80,160,320], drop_path 0, layer scale 1.0) on x (2,3,64,96): net_x, net_res2..5,
         net_loss = sum_k mean(res_k^2), net_dx, net_grad:<name> for convnext_fixture.NAMED (the two largest as every n-th row,
         convnext_fixture.ROW_STEP), net_names / net_shapes (the whole state dict).  Stages 3 and 4 are smaller than the 7x7 filter.
         net_env_err:<key> / net_env_cos:<key>: relative L2 error and cosine, against the above, of the same quantity from the reference
         run with every parameter rounded to bf16 (the sensitivity envelope of tests/test_model_gpu.py); <key> = res2..5, loss, dx,
         grad:<name>.
  block  Block(40) on (2,40,5,9): block_x, block_y (after dwconv), block_h (after norm), block_out, block_dout (upstream gradient),
         block_dx, block_grad:<parameter>.
  nols   Block(16, layer_scale_init_value=0) on (1,16,3,5): nols_x, nols_out.
  net_rounding_out / net_rounding_grad: largest relative L2 error of the reference in fp32 against itself in fp64 over the outputs /
  over all parameter gradients and dx.  The file is written only if both are below 1e-5.

    python tools/make_convnext_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import convnext_fixture as CF  # noqa: E402
from oracle import ref_loader  # noqa: E402

torch.set_num_threads(1)        # one summation order wherever the file is made


def run_net(mod, x, dtype, round_bf16=False):
    net = mod.ConvNeXt(**CF.NET)
    CF.fill_module(net, "net.")
    if round_bf16:
        with torch.no_grad():
            for p in net.parameters():
                p.copy_(p.to(torch.bfloat16).float())
    net = net.to(dtype)
    xi = x.detach().clone().to(dtype).requires_grad_(True)
    outs = net(xi)
    loss = sum(v.square().mean() for v in outs.values())
    loss.backward()
    q = {k: v.detach() for k, v in outs.items()}
    q["loss"] = loss.detach()
    q["dx"] = xi.grad
    for n, p in net.named_parameters():
        q["grad:" + n] = p.grad
    return q, net


def main():
    ref_loader._install_stubs()
    mod = ref_loader._load("model.modeling.backbone.convnext", "modeling/backbone/convnext.py")
    d = {}
    x = CF.input_for("net", CF.NET_X)
    q32, net = run_net(mod, x, torch.float32)
    q64, _ = run_net(mod, x, torch.float64)
    env, _ = run_net(mod, x, torch.float32, round_bf16=True)
    r_out = max(CF.rel(q32[k], q64[k]) for k in ("res2", "res3", "res4", "res5", "loss"))
    r_grad = max(CF.rel(q32[k], q64[k]) for k in q32 if k == "dx" or k.startswith("grad:"))
    print(f"reference fp32 vs fp64 on net: outputs {r_out:.3g}, gradients {r_grad:.3g}")
    if not (r_out < 1e-5 and r_grad < 1e-5):
        raise SystemExit("the reference's own rounding on this case is too large: not written")
    d["net_rounding_out"], d["net_rounding_grad"] = np.float64(r_out), np.float64(r_grad)
    d["net_x"] = x.numpy()
    for k in ("res2", "res3", "res4", "res5", "loss", "dx"):
        d["net_" + k] = q32[k].numpy()
        d["net_env_err:" + k], d["net_env_cos:" + k] = np.float64(CF.rel(env[k], q32[k])), np.float64(CF.cos(env[k], q32[k]))
    for n in CF.NAMED:
        d["net_grad:" + n] = CF.rows(n, q32["grad:" + n]).numpy()
        d["net_env_err:grad:" + n] = np.float64(CF.rel(env["grad:" + n], q32["grad:" + n]))
        d["net_env_cos:grad:" + n] = np.float64(CF.cos(env["grad:" + n], q32["grad:" + n]))
    sd = net.state_dict()
    d["net_names"] = np.array(list(sd.keys()))
    d["net_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])

    blk = mod.Block(CF.BLOCK_DIM, layer_scale_init_value=1.0)
    CF.fill_module(blk, "block.")
    bx = CF.input_for("block", CF.BLOCK_X).requires_grad_(True)
    dout = CF.input_for("block_dout", CF.BLOCK_X)
    y = blk.dwconv(bx)
    h = blk.norm(y.permute(0, 2, 3, 1))
    out = blk(bx)
    out.backward(dout)
    d.update(block_x=bx.detach().numpy(), block_y=y.detach().numpy(), block_h=h.detach().numpy(), block_out=out.detach().numpy(),
             block_dout=dout.numpy(), block_dx=bx.grad.numpy())
    for n, p in blk.named_parameters():
        d["block_grad:" + n] = p.grad.numpy()

    nols = mod.Block(CF.NOLS_DIM, layer_scale_init_value=0)
    assert nols.gamma is None
    CF.fill_module(nols, "nols.")
    nx = CF.input_for("nols", CF.NOLS_X)
    with torch.no_grad():
        d.update(nols_x=nx.numpy(), nols_out=nols(nx).numpy())

    np.savez_compressed(CF.GOLDEN, **d)
    print(f"wrote {CF.GOLDEN}: {os.path.getsize(CF.GOLDEN)} bytes, {len(d)} arrays")


if __name__ == "__main__":
    main()
