"""tests/golden/monodepth_loss.npz: what the REFERENCE's MonodepthLoss (model/modeling/monodepth_loss.py) computes on two small cases.

Build container only (needs the reference checkout).  The reference's class is loaded through oracle.ref_loader.load_sequence().geometry
and run as it is, on the CPU; nothing of its text is restated.  While it runs, here only,
  * `.cuda()` of modules and tensors is the identity (its constructor hard-wires it),
  * `torch.randn` and `np.random.choice` are wrapped so that the auto-mask tie noise and the RANSAC point indices it draws are recorded.

Cases (tests/monodepth_fixture.py): a = 2 images of 24 x 40, b = 1 image of 16 x 72; K differs per image; the poses move some samples out
of the image; the images are low-frequency sinusoids plus mild texture.  Flag sets: rigid, automask, full.  Per case the file holds the
inputs ({case}_disp{s}, {case}_T{f}, {case}_cflow{f}_{s}, {case}_mask{f}_{s}, {case}_prob{f}_{s}, {case}_color{f}, {case}_K, {case}_invK),
per case and flag set the recorded draws ({..}_noise{s}, {..}_ground{s}), every loss-dictionary entry ({..}_loss:<key>), the gradient of
`loss` with respect to every differentiable input ({..}_grad:<input>), the identity selection ({..}_idsel{s}), the keys of `outputs`
({..}_outkeys) and {..}_seedcheck: the largest relative L2 error of a gradient or loss entry of our restatement in fp32 against fp64.  A seed is kept
only if that figure is <= 2.5e-5 and the reference's own fp32 loss entries are within 1e-5 of fp64 ({..}_reference_rounding) for every flag set, so that fp32 rounding flips no bilinear cell and no minimum on the fixture.

    python tools/make_monodepth_golden.py            (scans seeds from the start: about ten minutes; --skip 123 3 resumes at the kept ones)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "uni-encoder-code_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import monodepth_fixture as MF  # noqa: E402

torch.set_num_threads(1)        # one summation order wherever the file is made

OUT = MF.GOLDEN


def smooth(g, shape, k=5):
    """Low-pass noise in roughly [-1, 1]."""
    x = torch.randn(shape, generator=g)
    pad = k // 2
    for _ in range(2):
        x = F.avg_pool2d(F.pad(x, (pad, pad, pad, pad), mode="replicate"), k, 1)
    return x / x.abs().max().clamp(min=1e-6)


def make_case(seed, B, H, W):
    g = torch.Generator().manual_seed(seed)
    d = {}
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    # images: one scene seen with a small shift per frame; dark (around 0.25) so that E[x^2] - E[x]^2 of the fp32 SSIM loses fewer digits
    tex = 0.05 * smooth(g, (B, 3, H, W), 3)
    for f in (-1, 0, 1):
        img = torch.empty(B, 3, H, W)
        for b in range(B):
            for c in range(3):
                a, bb, ph = 0.19 + 0.05 * c + 0.03 * b, 0.23 - 0.04 * c, 0.9 * c + 0.5 * b
                sx = xx + 3.0 * f
                img[b, c] = 0.25 + 0.11 * torch.sin(a * sx + 0.11 * yy + ph) + 0.08 * torch.cos(bb * yy - 0.07 * sx + 2 * ph)
        d[f"color{f}"] = (img + tex + 0.02 * smooth(g, (B, 3, H, W), 3)).clamp(0.02, 0.98)
    # intrinsics: KITTI-like, different per image
    K = torch.zeros(B, 4, 4)
    for b in range(B):
        K[b] = torch.tensor([[(0.58 + 0.04 * b) * W, 0, (0.5 - 0.02 * b) * W, 0], [0, (1.92 - 0.1 * b) * H, (0.5 + 0.015 * b) * H, 0],
                             [0, 0, 1, 0], [0, 0, 0, 1]])
    d["K"], d["invK"] = K, torch.linalg.inv(K.double()).float()
    for s in MF.SCALES:
        h, w = H >> s, W >> s
        rows = torch.linspace(0, 1, h)[None, None, :, None]
        d[f"disp{s}"] = (0.12 + 0.30 * rows + 0.08 * smooth(g, (B, 1, h, w), 3)).clamp(0.04, 0.9)      # nearer towards the bottom
        for f in MF.FRAMES:
            d[f"cflow{f}_{s}"] = 0.05 * smooth(g, (B, 3, h, w), 3) + torch.tensor([0.03 * f, 0.0, -0.04 * f])[None, :, None, None]
            d[f"mask{f}_{s}"] = torch.sigmoid(2.5 * smooth(g, (B, 1, h, w), 3))
            d[f"prob{f}_{s}"] = 2.0 * smooth(g, (B, 1, h, w), 3)
    for f in MF.FRAMES:
        aa = 0.05 * torch.randn(B, 1, 3, generator=g) + torch.tensor([0.0, 0.04 * f, 0.0])
        tr = 0.06 * torch.randn(B, 1, 3, generator=g) + torch.tensor([0.08 * f, 0.0, -0.12 * f])
        d[f"T{f}"] = transformation(aa, tr)
    return {k: v.contiguous().numpy() for k, v in d.items()}


def transformation(axisangle, translation):
    from uenc.modeling.geometry import transformation_from_parameters
    return transformation_from_parameters(axisangle, translation).float()


class Recorder:
    """Wraps torch.randn / np.random.choice while the reference runs."""

    def __init__(self):
        self.noise, self.choice = [], []

    def __enter__(self):
        self.randn, self.np_choice = torch.randn, np.random.choice
        self.mod_cuda, self.t_cuda = torch.nn.Module.cuda, torch.Tensor.cuda

        def randn(*a, **k):
            r = self.randn(*a, **k)
            self.noise.append(r.clone())
            return r

        def choice(*a, **k):
            r = self.np_choice(*a, **k)
            self.choice.append(np.array(r, dtype=np.int64))
            return r

        torch.randn, np.random.choice = randn, choice
        torch.nn.Module.cuda = lambda m, *a, **k: m
        torch.Tensor.cuda = lambda t, *a, **k: t
        return self

    def __exit__(self, *exc):
        torch.randn, np.random.choice = self.randn, self.np_choice
        torch.nn.Module.cuda, torch.Tensor.cuda = self.mod_cuda, self.t_cuda


def run_reference(ref, z, case, flagset, seed):
    B, H, W = MF.CASES[case]
    torch.manual_seed(seed)
    np.random.seed(seed)
    with Recorder() as rec:
        losses, grads, outputs = MF.run(ref.MonodepthLoss, z, case, flagset, set_attrs=True)
    out = {}
    if MF.FLAGSETS[flagset]["bool_automask"]:
        assert len(rec.noise) == 4 and all(tuple(n.shape) == (B, 2, H, W) for n in rec.noise)
        for s in MF.SCALES:
            out[f"noise{s}"] = rec.noise[s].numpy()
            out[f"idsel{s}"] = outputs[f"identity_selection/{s}"].numpy().astype(np.uint8)
    if MF.FLAGSETS[flagset]["bool_MotMask"]:
        assert len(rec.choice) == 4 * B
        for s in MF.SCALES:
            out[f"ground{s}"] = np.stack(rec.choice[s * B:(s + 1) * B])
    for k, v in losses.items():
        out[f"loss:{k}"] = MF.to_numpy(v).astype(np.float32 if torch.is_tensor(v) else np.float64)
    for k, v in grads.items():
        out[f"grad:{k}"] = v.numpy()
    out["outkeys"] = np.array(sorted(MF.key_name(k) for k in outputs))
    return out


REFERENCE_ROUNDING = 1e-5       # half the bar tests/test_monodepth_cpu.py holds the torch path to


def seed_check(z, case, flagset):
    """-> (ours, reference): the largest relative L2 error of a gradient or loss entry of our restatement in fp32 against fp64, and of
    the REFERENCE's own fp32 loss entries against that fp64 run.  The second figure matters for d_ground: its RANSAC winner and the
    LAPACK inverse of a fit through nearly collinear points (the 3 x 5 map has one ground row) can make the recorded value rounding
    noise, which would pin nothing."""
    from uenc.modeling.monodepth_loss import MonodepthLoss
    l32, g32, _ = MF.run(MonodepthLoss, z, case, flagset, dtype=torch.float32)
    l64, g64, _ = MF.run(MonodepthLoss, z, case, flagset, dtype=torch.float64)
    figs = [MF.rel_l2(g32[k].numpy(), g64[k].numpy()) for k in g64 if float(g64[k].abs().max()) > 0] or [float("inf")]
    figs += [MF.rel_l2(MF.to_numpy(l32[k]), MF.to_numpy(l64[k])) for k in l64]
    ref = [MF.rel_l2(z[f"{case}_{flagset}_loss:{k}"], MF.to_numpy(l64[k])) for k in l64]
    return max(figs), max(ref)


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip", type=int, nargs=2, default=(0, 0), metavar=("A", "B"),
                    help="seeds of case a / b to skip from the start of the scan (to resume one: the file in the tree is --skip 123 3)")
    skip = dict(zip(MF.CASES, ap.parse_args().skip))
    from oracle.ref_loader import load_sequence
    ref = load_sequence().geometry
    z = {}
    for ci, (case, (B, H, W)) in enumerate(MF.CASES.items()):
        for attempt in range(skip[case], 3000):
            seed = 20250000 + 10000 * ci + attempt
            cand = {f"{case}_{k}": v for k, v in make_case(seed, B, H, W).items()}
            results, worst = {}, 0.0
            for fs in ("full", "automask", "rigid"):         # the flag set that fails most often first
                res = run_reference(ref, cand, case, fs, seed)
                for k, v in res.items():
                    cand[f"{case}_{fs}_{k}"] = v
                fig, ref_fig = seed_check(cand, case, fs)
                cand[f"{case}_{fs}_seedcheck"] = np.float64(fig)
                cand[f"{case}_{fs}_reference_rounding"] = np.float64(ref_fig)
                results[fs] = (fig, ref_fig)
                worst = max(worst, fig, ref_fig * (MF.SEED_CHECK_REL_L2 / REFERENCE_ROUNDING))
                if worst > MF.SEED_CHECK_REL_L2:
                    break
            print(f"case {case} seed {seed}: fp32 vs fp64 (ours, the reference's loss entries) {results}")
            if worst <= MF.SEED_CHECK_REL_L2:
                cand[f"{case}_seed"] = np.int64(seed)
                z.update(cand)
                break
        else:
            raise SystemExit(f"case {case}: no seed passed the fp32 / fp64 check")
        x = torch.from_numpy(z[f"{case}_full_grad:T-1"])
        print(f"case {case}: loss {z[case + '_full_loss:loss']}  |dT| {float(x.abs().max()):.3e}")
    np.savez_compressed(OUT, **z)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT}: {size} bytes, {len(z)} arrays")
    assert size < (1 << 20)


if __name__ == "__main__":
    main()
