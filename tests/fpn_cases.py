"""Shared by tests/test_fpn_cases_cpu.py and tests/test_fpn_kernels_gpu.py: the case tables of the seven kernels of csrc/fpn.hip
(channels-last GroupNorm forward / backward, the bilinear top-down merge and its adjoint, im2col / col2im of the 3x3 convolutions at
stride 1 and 2), their inputs and their references.

Nothing here imports `uenc`.  Inputs come from a seeded CPU generator.  Every reference is a plain torch composition that takes the
dtype and device of its arguments: the tests run it in float64 on the CPU (the reference proper, `r64`) and once more in fp32 on the GPU
(`t32`), whose distance from `r64` is what the kernels' error is judged against.
"""
import torch
import torch.nn.functional as F

EPS = 1e-5
VARIANTS = ("f32", "bf16")          # x, dy, y and dx all fp32 / all bf16 (as the branch uses them); gamma, beta, stats, src stay fp32

# ---- GroupNorm ----------------------------------------------------------------------------------------------------------------
# (B, HW, C, G): what each geometry reaches in gn_reduce / gn_stats / gn_bwd_coef / gn_apply
GN_GEOMS = [
    (2, 37, 8, 2),            # one channel quad per group, 128 token rows per workgroup
    (1, 300, 64, 4),          # 16 channels per group, 3 chunks with a ragged last one
    (3, 960, 256, 32),        # the model's own C and G; three images through the dgamma / dbeta atomics
    (1, 130, 1024, 16),       # 256 channel quads = one token row per workgroup, 64 channels per group, 16 column blocks in the coefficient kernel
    (2, 129, 4, 1),           # a single channel quad
    (1, 132000, 64, 16),      # chunk count capped at 1024 and the apply grid capped at 8192 workgroups: both grid-stride loops
]
RELU_MAX_ELEMS = 8192
RELU_MARGIN = 1e-4
# ReLU cases: ((B, HW, C, G), seed).  At most RELU_MAX_ELEMS elements, and a seed for which the float64 pre-activation stays at least
# RELU_MARGIN away from zero for both dtype variants (tests/test_fpn_cases_cpu.py asserts it): fp32 rounding of the pre-activation is
# below 1e-5 at these magnitudes, so no mask bit can differ between kernel and reference and no element has to be excused.
GN_RELU = [((2, 37, 8, 2), 1), ((2, 129, 4, 1), 1), ((1, 32, 256, 32), 9), ((1, 120, 64, 4), 1)]

# (Hs, Ws) -> (H, W) of the bilinear merge: exact 2x, the odd 13 -> 25 rows of the real FPN, exact 4x, a single source pixel, the
# identity, a ratio just above 1 on one axis only, and a large non-integer ratio
MERGE_SIZES = [((12, 20), (24, 40)), ((13, 21), (25, 42)), ((7, 9), (28, 36)), ((1, 1), (5, 7)), ((3, 5), (3, 5)), ((5, 4), (6, 4)),
               ((2, 3), (37, 50))]
MERGE_CG = [(8, 2), (256, 32)]
MERGE_B = 2

ADJOINT_SIZES = MERGE_SIZES + [((16, 24), (32, 48))]
ADJOINT_C = (4, 8, 256)
ADJOINT_DTYPES = ("f32", "bf16")
ADJOINT_B = 2
ADJOINT_IDENTITY_CAP = (1, 128, 132, 1024)        # (B, H, W, C) with Hs == H, Ws == W: more than 16384 * 256 channel quads

# ---- 3x3 gathers --------------------------------------------------------------------------------------------------------------
GATHER_MAPS = [(1, 1), (1, 9), (9, 1), (2, 2), (13, 21), (16, 24)]
GATHER_MAPS_S2 = GATHER_MAPS + [(5, 8), (8, 5)]     # stride 2: with the maps above, every parity combination of (H, W)
GATHER_B = (1, 3)
GATHER_C = (8, 64, 264)
IM2COL_CAP = (1, 256, 256, 232)                     # B*H*W*9*C/8 = 17.1 M work items > 65536 * 256

# ---- argument checks ------------------------------------------------------------------------------------------------------------
# (C, G, why) that uenc_groupnorm_tokens_fwd / _bwd must refuse
GN_REJECT = [(96, 12, "C/4 = 24 does not divide 256"), (2048, 32, "C > 1024"), (256, 2, "C/G = 128 does not divide 64"),
             (24, 4, "C/G = 6 is no multiple of 4")]
# ((Hs, Ws), (H, W), C, why) that uenc_upsample_bilinear_tokens_bwd must refuse
ADJOINT_REJECT = [((5, 4), (4, 4), 8, "H < Hs"), ((4, 5), (4, 4), 8, "W < Ws"), ((2, 2), (4, 4), 6, "C % 4 != 0")]
GATHER_REJECT_C = (4, 12)                            # C % 8 != 0


def gn_shape_ok(C: int, G: int) -> bool:
    """The shape contract of uenc_groupnorm_tokens_fwd / _bwd as include/uenc.h states it."""
    return C % G == 0 and (C // G) % 4 == 0 and 64 % (C // G) == 0 and C % 4 == 0 and 256 % (C // 4) == 0 and C <= 1024


def gn_cases():
    """Every GroupNorm case: dict(id, B, HW, C, G, relu, seed, merge) with merge = None or ((Hs, Ws), (H, W))."""
    out = []
    for i, (B, HW, C, G) in enumerate(GN_GEOMS):
        out.append(dict(id=f"plain-{B}x{HW}x{C}g{G}", B=B, HW=HW, C=C, G=G, relu=False, seed=100 + i, merge=None))
    for (B, HW, C, G), seed in GN_RELU:
        out.append(dict(id=f"relu-{B}x{HW}x{C}g{G}", B=B, HW=HW, C=C, G=G, relu=True, seed=seed, merge=None))
    for i, ((Hs, Ws), (H, W)) in enumerate(MERGE_SIZES):
        for C, G in MERGE_CG:
            out.append(dict(id=f"merge-{Hs}x{Ws}to{H}x{W}-c{C}", B=MERGE_B, HW=H * W, C=C, G=G, relu=False, seed=200 + i,
                            merge=((Hs, Ws), (H, W))))
    return out


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def gn_inputs(case, variant: str):
    """fp32 CPU tensors (x and dy bf16 for the bf16 variant).  Channels differ in scale and offset and gamma in sign, so that a wrong
    channel, group or image index changes the result; dgamma / dbeta start from a non-zero prefill (they are accumulated into)."""
    B, HW, C = case["B"], case["HW"], case["C"]
    g = _gen(case["seed"])
    scale = 0.5 + 1.5 * torch.rand(C, generator=g)
    shift = 2.0 * torch.rand(C, generator=g) - 1.0
    x = torch.randn(B, HW, C, generator=g) * scale + shift
    dy = torch.randn(B, HW, C, generator=g)
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    t = dict(x=x, dy=dy, gamma=sign * (0.5 + torch.rand(C, generator=g)), beta=torch.rand(C, generator=g) - 0.5,
             pre_dgamma=torch.randn(C, generator=g), pre_dbeta=torch.randn(C, generator=g))
    if case["merge"] is not None:
        (Hs, Ws), _ = case["merge"]
        t["src"] = torch.randn(B, Hs, Ws, C, generator=g)
    if variant == "bf16":
        t["x"], t["dy"] = t["x"].bfloat16(), t["dy"].bfloat16()
    return t


def upsample(src, size):
    """(B, Hs, Ws, C) -> (B, H, W, C), bilinear, align_corners=False."""
    return F.interpolate(src.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


def upsample_adjoint(d, Hs: int, Ws: int):
    """d (B, H, W, C) -> (B, Hs, Ws, C): autograd adjoint of `upsample` alone."""
    B, H, W, C = d.shape
    s = torch.zeros(B, Hs, Ws, C, dtype=d.dtype, device=d.device, requires_grad=True)
    return torch.autograd.grad(upsample(s, (H, W)), s, d)[0]


def gn_reference(t, case, dtype=torch.float64, device="cpu"):
    """F.group_norm on the NCHW view [+ F.interpolate(src)] [ReLU] with autograd, in `dtype` on `device`, from the inputs `t` of
    gn_inputs.  Returns y, z (the value in front of the ReLU), mean, rstd, dx, dgamma / dbeta (prefill + gradient) and dsrc."""
    B, HW, C, G = case["B"], case["HW"], case["C"], case["G"]
    H, W = case["merge"][1] if case["merge"] is not None else (HW, 1)
    v = {k: a.to(device=device, dtype=dtype, copy=True) for k, a in t.items()}
    leaves = [v[k].requires_grad_(True) for k in ("x", "gamma", "beta")]
    z = F.group_norm(v["x"].permute(0, 2, 1).reshape(B, C, H, W), G, v["gamma"], v["beta"], EPS)
    if case["merge"] is not None:
        leaves.append(v["src"].requires_grad_(True))
        z = z + F.interpolate(v["src"].permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    y = F.relu(z) if case["relu"] else z
    tok = lambda a: a.reshape(B, C, HW).permute(0, 2, 1)
    grads = torch.autograd.grad(tok(y), leaves, v["dy"])
    xg = v["x"].detach().reshape(B, HW, G, C // G)
    var, mean = torch.var_mean(xg, dim=(1, 3), unbiased=False)
    out = dict(y=tok(y).detach(), z=tok(z).detach(), mean=mean, rstd=(var + EPS).rsqrt(), dx=grads[0],
               dgamma=v["pre_dgamma"] + grads[1], dbeta=v["pre_dbeta"] + grads[2])
    if case["merge"] is not None:
        out["dsrc"] = grads[3]
    return out


def adjoint_inputs(Hs, Ws, H, W, C, dtype: str, B: int = ADJOINT_B):
    g = _gen(7 + 1000 * Hs + 100 * Ws + 10 * H + W + C)
    d = torch.randn(B, H, W, C, generator=g)
    return dict(d=d.bfloat16() if dtype == "bf16" else d, src=torch.randn(B, Hs, Ws, C, generator=g), x=torch.randn(B, H * W, C, generator=g))


# ---- im2col / col2im ----------------------------------------------------------------------------------------------------------------
def gather_input(B, H, W, C, seed=0):
    return torch.randn(B, H, W, C, generator=_gen(seed + 31 * H + W + 7 * C + B)).bfloat16()


def gather_dcol(B, H, W, C, stride: int, seed=1):
    Ho, Wo = (H, W) if stride == 1 else ((H + 1) // 2, (W + 1) // 2)
    return torch.randn(B * Ho * Wo, 9 * C, generator=_gen(seed + 31 * H + W + 7 * C + B)).bfloat16()


def im2col_ref(x, stride: int):
    """x (B, H, W, C) of any dtype -> (B * Ho * Wo, 9 * C): zero-pad, nine shifted slices concatenated in (ky, kx, c) order."""
    B, H, W, C = x.shape
    Ho, Wo = (H, W) if stride == 1 else ((H + 1) // 2, (W + 1) // 2)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    taps = [xp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] for ky in range(3) for kx in range(3)]
    return torch.cat(taps, dim=-1).reshape(B * Ho * Wo, 9 * C)


def col2im_ref(dcol, B, H, W, C, stride: int):
    """dcol (B * Ho * Wo, 9 * C) bf16 -> (B, H, W, C) fp32: nine shifted fp32 adds in ascending tap order k = ky * 3 + kx, the order in
    which the kernels accumulate the (at most nine) taps of an element, so the result is the kernel's bit for bit."""
    Ho, Wo = (H, W) if stride == 1 else ((H + 1) // 2, (W + 1) // 2)
    d = dcol.float().view(B, Ho, Wo, 9, C)
    dxp = torch.zeros(B, stride * (Ho - 1) + 3, stride * (Wo - 1) + 3, C, dtype=torch.float32, device=dcol.device)
    for k in range(9):
        ky, kx = divmod(k, 3)
        dxp[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride] += d[:, :, :, k]
    return dxp[:, 1:1 + H, 1:1 + W].contiguous()


def col2im_expected(dcol, B, H, W, C, stride: int):
    """What the kernels store: stride 1 rounds the fp32 sum to bf16 (nearest even), stride 2 keeps fp32."""
    r = col2im_ref(dcol, B, H, W, C, stride)
    return r.bfloat16() if stride == 1 else r


def gather_cases(stride: int):
    return [(B, H, W, C) for (H, W) in (GATHER_MAPS if stride == 1 else GATHER_MAPS_S2) for B in GATHER_B for C in GATHER_C]
