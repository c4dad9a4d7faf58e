"""Cases and float64 references of the three kernel pairs of csrc/depth_head.hip (x2 align-corners upsample, softmax gate, soft-attention
depth head).  Shared by tests/test_depth_head_cases_cpu.py (which checks the references themselves) and
tests/test_depth_head_kernels_gpu.py (which holds the kernels against them).

Every reference is a torch composition (`F.interpolate(..., align_corners=True)`, `F.softmax`) differentiated by autograd; it runs in
float64 on the CPU (r64) or, unchanged, in fp32 on the GPU (t32, whose error against r64 sets the fp32 bar).  Variant "bf16": the
inputs are rounded to bf16 first, so r64 is the exact result for the values the kernel reads."""
import torch
import torch.nn.functional as F

VARIANTS = ("f32", "bf16")

UPSAMPLE_SHAPES = [(1, 1, 1, 8), (1, 1, 5, 8), (2, 2, 3, 8), (1, 5, 7, 16), (1, 16, 24, 256), (1, 33, 31, 264)]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _round(t, variant):
    """The values the kernel reads: fp32, or fp32 that is exactly representable in bf16."""
    return t if variant == "f32" else t.bfloat16().float()


def shape_id(s):
    return "x".join(map(str, s))


# ---- upsample ------------------------------------------------------------------------------------------------------------------------
def upsample_inputs(shape, variant):
    B, H, W, C = shape
    g = _gen(1000 + H * 131 + W * 17 + C)
    return {"x": _round(torch.randn(B, H, W, C, generator=g), variant), "dy": _round(torch.randn(B, 2 * H, 2 * W, C, generator=g), variant)}


def upsample2x(x_nhwc):
    return F.interpolate(x_nhwc.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


def upsample_reference(t, dtype=torch.float64, device="cpu"):
    x = t["x"].to(device=device, dtype=dtype).requires_grad_(True)
    y = upsample2x(x)
    (dx,) = torch.autograd.grad(y, x, t["dy"].to(device=device, dtype=dtype))
    return {"y": y.detach().contiguous(), "dx": dx.contiguous()}


# ---- softmax gate ----------------------------------------------------------------------------------------------------------------------
def gate_cases():
    cases = [{"id": f"{P}x{C}", "P": P, "C": C, "logits": "normal"} for P, C in ((1, 8), (63, 256), (65, 256), (130, 264))]
    cases.append({"id": "65x256_pm80", "P": 65, "C": 256, "logits": "pm80"})
    cases.append({"id": "63x256_equal", "P": 63, "C": 256, "logits": "equal"})
    return cases


def _logits(kind, P, C, g):
    if kind == "pm80":
        return (torch.rand(P, C, generator=g) * 2 - 1) * 80.0
    if kind == "equal":
        return torch.full((P, C), 1.25)
    return torch.randn(P, C, generator=g) * 2.0


def gate_inputs(case, variant):
    P, C = case["P"], case["C"]
    g = _gen(2000 + P * 7 + C + len(case["logits"]))
    r = lambda: _round(torch.randn(P, C, generator=g), variant)
    return {"a": r(), "b": r(), "z": _round(_logits(case["logits"], P, C, g), variant), "dg": r(), "dres": r()}


def gate_reference(t, second, dtype=torch.float64, device="cpu"):
    """second: whether a gradient already arrives at `res` (the fusion block adds `res` again behind resConfUnit2)."""
    a, b, z, dg, dres = (t[k].to(device=device, dtype=dtype) for k in ("a", "b", "z", "dg", "dres"))
    a.requires_grad_(True), b.requires_grad_(True), z.requires_grad_(True)
    res = a + b
    g = res * F.softmax(z, dim=-1)
    s = (g * dg).sum() + ((res * dres).sum() if second else 0.0)
    da, db, dz = torch.autograd.grad(s, (a, b, z))
    return {"res": res.detach(), "g": g.detach(), "d_res": da, "d_res_b": db, "d_z": dz}


# ---- soft-attention depth head -----------------------------------------------------------------------------------------------------------
ALPHA, BETA = 0.01, 1.0


def depth_grid(D, kind):
    """The grid of SoftAttDepth (reference pixel_decoder/transdssl.py:187-222) as fp32, "UD" uniform or "SID" log-spaced."""
    if kind == "SID":
        k = torch.arange(D, dtype=torch.float32)
        return torch.exp(torch.log(torch.tensor(ALPHA)) + torch.log(torch.tensor(BETA / ALPHA)) * k / D)
    return torch.linspace(ALPHA, BETA, D)


def head_cases():
    cases = [{"id": f"{P}x{D}_{kind}", "P": P, "D": D, "grid": kind, "logits": "normal"}
             for P, D in ((1, 32), (255, 32), (257, 32), (100, 8), (70, 64)) for kind in ("UD", "SID")]
    cases.append({"id": "257x32_UD_pm80", "P": 257, "D": 32, "grid": "UD", "logits": "pm80"})
    return cases


def head_inputs(case, variant):
    P, D = case["P"], case["D"]
    g = _gen(3000 + P * 3 + D + len(case["grid"]))
    return {"z": _round(_logits(case["logits"], P, D, g), variant), "grid": depth_grid(D, case["grid"]), "ddisp": torch.randn(P, generator=g)}


def head_reference(t, dtype=torch.float64, device="cpu"):
    z = t["z"].to(device=device, dtype=dtype).requires_grad_(True)
    disp = (F.softmax(z, dim=-1) * t["grid"].to(device=device, dtype=dtype)).sum(-1)
    (dz,) = torch.autograd.grad(disp, z, t["ddisp"].to(device=device, dtype=dtype))
    return {"disp": disp.detach(), "dz": dz}
