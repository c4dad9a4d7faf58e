"""Shared by tests/test_monodepth_cases_cpu.py and tests/test_monodepth_kernels_gpu.py: the case tables of the four entry points of
csrc/monodepth.hip (`uenc_view_synth_fwd` / `_bwd`, `uenc_photo_loss_fwd` / `_bwd`), their inputs, float64 references, bars and the defects
the bars must see.

Nothing here imports `uenc`.  Inputs come from a seeded CPU generator in float64 and are rounded to fp32 once, so every reference sees exactly
the values the kernels see.  Intrinsics are KITTI-like and differ per image (fx ~ 0.58 W, fy ~ 1.92 H, principal point at the centre, inv_K the
fp32-rounded inverse), cam_T_cam is a rotation of at most 0.05 rad plus a translation of +- `tscale` per (frame, image), disp lies in
[0.02, 0.6], images in [0.1, 0.9] with texture.

  r64   `vs_reference` / `ph_forward` / `ph_backward` with dtype = float64: plain torch, as include/uenc.h states the operations:
        F.interpolate(align_corners=False), depth = 1 / (0.01 + 9.99 d), back-projection, the three flow modes, projection divided by
        z + 1e-7, F.grid_sample(padding_mode="border", align_corners=True); SSIM over 3x3 means of the reflection-padded images with
        C1 = 1e-4, C2 = 9e-4, 0.85 mean_c SSIM + 0.15 mean_c L1, the minimum over the candidates (the first on a tie) and its mean.
        Backward by autograd: view synthesis of sum gcolor color + sum gres residual; photometric of sum_s gp[s] p_photo[s] with the
        selection held fixed.
  r32   the same functions with dtype = float32: the same torch composition in fp32 on the CPU.  Its distance from r64 sets the scale of
        every bar (RHO32), never a kernel's.

Bars.  Per element of a dense output (color, sample, sample_ego, sample_cmp, depth, residual, gdisp, gcflow, gmask, grad_color):
|kernel - r64| <= kappa 2^-24 M, M = max |r64| over the output's (scale, frame, image) item.  For the reduced outputs gT and p_photo:
kappa 2^-24 A, A = the float64 sum of the absolute per-pixel contributions.  kappa = max(2 RHO32[kind], 8): RHO32[kind] bounds
|r32 - r64| / (2^-24 M or A) over the whole table (tests/test_monodepth_cases_cpu.py asserts it, and that the constant is at most twice the
measured worst); the factor 2 is for what a kernel does and fp32 torch does not (fma contraction, its own summation order in the gathers and
block partials); the floor of 8 keeps a kind on which fp32 torch happens to be nearly exact from getting a bar below rounding noise.  Where
M or A is 0 the output must be exactly 0.

Discontinuities are handled by conditions on the INPUTS; no output element is excused.
  view-synthesis backward   a full-resolution pixel is fragile if its float64 sample coordinate, un-normalised, lies within 2^-10 of an
        integer inside the image or of the clip edges 0, W - 1, H - 1 (there floor() or the clip's gradient stop may fall either way).
        gcolor is the test's own input: it is 0 at fragile pixels, for reference and kernel alike.  At most 2 % of a run's pixels may be
        fragile; with H W >= 256 at least 10 % are clipped and 25 % unclipped.
  cam_T_cam gradient        A sums whole pixels; a pixel's contribution is itself a sum over the three colour channels.  Per element, the sum
        of the absolute per-pixel-and-channel contributions is at most 2.5 A (MAX_CHANNEL_CANCELLATION): inputs whose channel terms cancel
        inside the one or two live pixels of a tiny image are ill-conditioned for any fp32 evaluation and are not in the table.
  photometric argmin        compared where the two smallest float64 candidate values differ by more than twice the per-pixel value bar
        (kappa[photo_value] 2^-24 max |value| of the (scale, image)); at most 1 % of a case's pixels may be unjudged.  p_photo is continuous
        and compared everywhere.  The designed exact ties (two bit-identical warped candidates; automask with zero noise and src
        bit-identical to color) are compared everywhere.
  photometric backward      argmin is an input: the reference's map, a seeded random map, all-identity under automask.
"""
import math

import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
DELTA = 2.0 ** -10                  # fragile band around an integer sample coordinate / a clip edge
VS_THREADS = 256                    # pixels per block of the view-synthesis kernels
PH_TX, PH_TY = 32, 8                # photometric tile
MIN_ABS_Z = 0.05                    # every projection's |z + 1e-7| in float64: nearer is ill-conditioned and outside the contract
MAX_FRAGILE, MIN_CLIPPED, MIN_UNCLIPPED, MAX_UNJUDGED = 0.02, 0.10, 0.25, 0.01
MAX_CHANNEL_CANCELLATION = 2.5      # per cam_T_cam element: sum over pixels AND colour channels of |contribution| / A (see VS_CASES)
TIE_NOISE_SCALE = 1e-5
C1, C2 = 1e-4, 9e-4

# Largest |r32 - r64| / (2^-24 M or A) of the fp32 torch composition over the whole table, rounded up to two digits
# (tests/test_monodepth_cases_cpu.py::test_rho32_is_the_measured_maximum prints the measurement)
RHO32 = {
    "color": 64.0, "sample": 6.7, "sample_ego": 6.7, "sample_cmp": 6.6, "depth": 3.2, "residual": 33.0,
    "gdisp": 220.0, "gcflow": 60.0, "gmask": 110.0, "gT": 9.6,
    "photo_value": 890.0, "p_photo": 210.0, "grad_color": 600.0,
}
KAPPA = {k: max(2.0 * v, 8.0) for k, v in RHO32.items()}

# leading dimensions that index an output's items (lists of per-(scale, frame) tensors are stacked first)
LEAD = {"color": 3, "sample": 3, "sample_ego": 3, "sample_cmp": 3, "depth": 2, "residual": 2, "gdisp": 2, "gcflow": 2, "gmask": 2,
        "grad_color": 3, "photo_value": 2}


def vs_outputs(mode, backward=True):
    """The outputs a mode writes."""
    fwd = ("color", "sample", "depth") + (("sample_ego", "sample_cmp", "residual") if mode >= 1 else ())
    bwd = ("gdisp", "gT") + (("gcflow",) if mode >= 1 else ()) + (("gmask",) if mode == 2 else ())
    return fwd + (bwd if backward else ())


# ---- case tables --------------------------------------------------------------------------------------------------------------------
# view synthesis: (id, B, H, W, S, NF, tscale): tscale = the translation's range, chosen per case so that clipped and unclipped samples are
# both well populated while every projection keeps |z| >= MIN_ABS_Z
_VS_TABLE = [
    ("min2x2", 1, 2, 2, 1, 1, 0.05),            # the smallest legal shape
    ("s3-1x1", 1, 8, 8, 4, 2, 0.10),            # the scale-3 map is 1 x 1: up_index with n = 1
    ("one-block", 1, 16, 16, 4, 1, 0.10),       # H W = 256: exactly one block, NF = 1
    ("ragged-2blk", 2, 8, 40, 4, 2, 0.10),      # 320 pixels: nblk = 2, the second block ragged, feeding the cam_T_cam partials
    ("s3-b3", 3, 12, 20, 3, 2, 0.10),           # S = 3, B = 3, K and T distinct per item: the item -> (s, f, b) decode; H W < 256
    ("odd-s1", 1, 9, 33, 1, 1, 0.10),           # odd sizes, S = 1, just above 256 pixels
    ("wide", 1, 8, 72, 4, 2, 0.10),             # wide; the scale-3 map has one row (1 x 9); three blocks
]
# (B, H, W, S, NF) = (1, 8, 66, 4, 2) is wide with a one-row scale-3 map too, but 66 is no multiple of 2^(S - 1): 66 >> 3 = 8 columns would
# be upsampled by 8.25, no integer factor, which include/uenc.h excludes.  The entry points must REFUSE it (UENC_EINVAL, nothing written).
VS_REFUSED = [dict(id="wide-66", B=1, H=8, W=66, S=4, NF=2)]
VS_CASES = [dict(id=i, B=B, H=H, W=W, S=S, NF=NF, tscale=ts, behind=False, seed=2000 + n) for n, (i, B, H, W, S, NF, ts) in enumerate(_VS_TABLE)]
# With four pixels, of which one or two are unclipped, a cam_T_cam element can be ONE pixel's contribution, and that is a sum over the three
# colour channels and over the terms of the projection's gradient (K_02 dcx + K_12 dcy + dcz, which cancel as the sample nears the
# principal point).  Where these cancel inside the pixel (seed 2000, mode 0: the channel terms to 1 / 39 of their absolute sum) no fp32
# evaluation in any order meets a bar scaled by A, which only sees whole pixels (the kernel was 41 units of 2^-24 A off there, fp32
# torch 8, and with other seeds 29).  So the smallest case is conditioned on the reference alone: the first seed from 2000 on at which, in all three modes, an unclipped pixel exists,
# none is fragile, MAX_CHANNEL_CANCELLATION holds (every other run of the table is at 1.9 or below) and fp32 torch stays under HALF of every
# RHO32 -- the smallest case sets no constant (tests/test_monodepth_cases_cpu.py asserts all four).
VS_CASES[0]["seed"] = 2005
# a few points behind the camera: S = 1 (no upsampling between the near and the far population), translation z = -0.3
VS_CASES.append(dict(id="behind", B=2, H=10, W=36, S=1, NF=2, tscale=0.1, behind=True, seed=2100))
VS_BY_ID = {c["id"]: c for c in VS_CASES}

# runs: (case, mode, gres) with gres in "all" | "none" | "some" (which of the S * NF residual gradients are given; mode 0 takes none)
VS_RUNS = [(c["id"], m, "all" if m else "none") for c in VS_CASES if not c["behind"] for m in (0, 1, 2)]
VS_RUNS += [("behind", 0, "none")]
VS_RUNS += [(cid, m, g) for cid in ("ragged-2blk",) for m in (1, 2) for g in ("none", "some")]


def vs_run_id(run):
    return f"{run[0]}/m{run[1]}/gres-{run[2]}"


def vs_blocks(case):
    return -(-case["H"] * case["W"] // VS_THREADS)


def gres_given(case, which):
    n = case["S"] * case["NF"]
    return [which == "all" or (which == "some" and i % 2 == 0) for i in range(n)]


# photometric loss: (id, S, NF, B, H, W, automask, special)
_PH_TABLE = [
    ("min2x2", 1, 1, 1, 2, 2, 0, None),             # the smallest legal shape: every window is reflections
    ("refl3x3", 1, 2, 1, 3, 3, 1, None),            # reflected pixels counted two and three times
    ("one-tile", 2, 2, 2, 8, 32, 1, None),          # exactly one 32 x 8 tile
    ("edge-tiles", 1, 1, 1, 9, 33, 0, None),        # 2 x 2 tiles, each edge tile one pixel wide or high
    ("sub-tile", 1, 2, 1, 7, 31, 1, None),          # smaller than one tile
    ("seams", 4, 2, 2, 16, 64, 1, None),            # 2 x 2 full tiles: seams in the interior
    ("wide-short", 3, 1, 3, 3, 70, 0, None),        # very wide and short: three tiles, overhang in both directions
    ("flat-patch", 1, 2, 1, 12, 40, 0, "flat"),     # candidate 0 and target bit-identical on a block: variance 0, |df| = 0, SSIM on the clamp
    ("tie-warped", 2, 2, 2, 9, 33, 0, "tie_warped"),        # two bit-identical warped candidates: index 0 wins everywhere
    ("tie-identity", 2, 1, 2, 9, 33, 1, "tie_identity"),    # zero noise, src bit-identical to color: the identity candidate wins
                                                            # (NF = 1: no second identity candidate that could come near the first)
]
PH_CASES = [dict(id=i, S=S, NF=NF, B=B, H=H, W=W, automask=a, special=sp, seed=3000 + n)
            for n, (i, S, NF, B, H, W, a, sp) in enumerate(_PH_TABLE)]
PH_BY_ID = {c["id"]: c for c in PH_CASES}


def ph_tiles(case):
    return -(-case["W"] // PH_TX), -(-case["H"] // PH_TY)


def ph_maps(case):
    """The argmin maps the backward is run with."""
    return ("reference", "random") + (("identity",) if case["automask"] else ())


# defect -> the runs / cases it is aimed at, and the outputs it must push past their bar there
VS_DEFECTS = {
    "up_align_corners": ([("wide", 0, "none"), ("s3-b3", 2, "all")], ("color", "depth", "gdisp")),
    "gather_row_short": ([("ragged-2blk", 2, "all"), ("s3-1x1", 1, "all")], ("gdisp", "gcflow")),
    "clip_without_gradient_stop": ([("ragged-2blk", 0, "none"), ("odd-s1", 1, "all")], ("gdisp",)),
    "tap_beyond_last_column_read": ([("s3-b3", 0, "none"), ("wide", 1, "all"), ("ragged-2blk", 1, "all")], ("color",)),
    "mode1_through_T": ([("odd-s1", 1, "all"), ("ragged-2blk", 1, "none")], ("color", "sample", "gdisp")),
    "residual_ego_sign": ([("s3-b3", 1, "all"), ("ragged-2blk", 2, "some")], ("residual", "gT")),
    "gres_ignored": ([("ragged-2blk", 1, "all"), ("ragged-2blk", 2, "some")], ("gcflow", "gT")),
}
PH_DEFECTS = {
    "reflect_counted_once_bwd": (["refl3x3", "edge-tiles", "min2x2"], ("grad_color",)),
    "ssim_replicate_pad": (["refl3x3", "wide-short"], ("p_photo", "grad_color")),
    "second_wins_ties": (["tie-warped", "tie-identity"], ("argmin",)),
    "noise_on_warped": (["refl3x3", "one-tile", "sub-tile"], ("p_photo",)),
    "l1_sign_plus_at_zero": (["flat-patch"], ("grad_color",)),
    "mean_without_B": (["one-tile", "wide-short"], ("p_photo",)),
}
DEFECTS = sorted(VS_DEFECTS) + sorted(PH_DEFECTS)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def _field(g, lead, h, w):
    """lead + (h, w) float64 in [-1, 1]: three random plane waves (70 %) plus white noise (30 %)."""
    y = (torch.arange(h, dtype=torch.float64) / max(h, 2)).view(h, 1)
    x = (torch.arange(w, dtype=torch.float64) / max(w, 2)).view(1, w)
    r = lambda: torch.rand(tuple(lead) + (1, 1), generator=g, dtype=torch.float64)
    f = sum(torch.sin((1 + 7 * r()) * y * 2 * math.pi * 0.5 + (1 + 9 * r()) * x * 2 * math.pi * 0.5 + 2 * math.pi * r()) for _ in range(3)) / 3
    return 0.7 * f + 0.3 * (2 * torch.rand(tuple(lead) + (h, w), generator=g, dtype=torch.float64) - 1)


def _image(g, lead, h, w):
    return (0.5 + 0.4 * _field(g, lead, h, w)).clamp(0.1, 0.9)


def _skew(a):
    z = torch.zeros_like(a[..., 0])
    return torch.stack([torch.stack([z, -a[..., 2], a[..., 1]], -1), torch.stack([a[..., 2], z, -a[..., 0]], -1),
                        torch.stack([-a[..., 1], a[..., 0], z], -1)], -2)


def vs_raw_inputs(case):
    """Everything of a view-synthesis case but gcolor's fragile zeros (those depend on the mode): fp32 CPU tensors."""
    B, H, W, S, NF = (case[k] for k in ("B", "H", "W", "S", "NF"))
    g = _gen(case["seed"])
    u = lambda *shape: 2 * torch.rand(shape, generator=g, dtype=torch.float64) - 1
    K = torch.eye(4, dtype=torch.float64).repeat(B, 1, 1)
    K[:, 0, 0] = 0.58 * W * (1 + 0.06 * u(B))
    K[:, 1, 1] = 1.92 * H * (1 + 0.06 * u(B))
    K[:, 0, 2], K[:, 1, 2] = 0.5 * W, 0.5 * H
    K32 = K.float()
    invK32 = torch.linalg.inv(K32.double()).float()
    axis = u(NF, B, 3)
    axis = axis / axis.norm(dim=-1, keepdim=True) * 0.05 * torch.rand(NF, B, 1, generator=g, dtype=torch.float64)
    T = torch.eye(4, dtype=torch.float64).repeat(NF, B, 1, 1)
    T[..., :3, :3] = torch.linalg.matrix_exp(_skew(axis))
    T[..., :3, 3] = case["tscale"] * u(NF, B, 3)
    if case["behind"]:
        T[..., 2, 3] = -0.3
    disp, cflow, mask = [], [], []
    for s in range(S):
        h, w = H >> s, W >> s
        if case["behind"]:
            near = torch.rand(B, 1, h, w, generator=g, dtype=torch.float64) < 0.12
            depth = torch.where(near, 0.17 + 0.04 * torch.rand(B, 1, h, w, generator=g, dtype=torch.float64),
                                0.45 + 3.5 * torch.rand(B, 1, h, w, generator=g, dtype=torch.float64))
            disp.append(((1 / depth - 0.01) / 9.99).float())
        else:
            disp.append((0.31 + 0.29 * _field(g, (B, 1), h, w)).float())
        for f in range(NF):
            cflow.append((0.04 * _field(g, (B, 3), h, w)).float())
            mask.append((0.5 + 0.5 * _field(g, (B, 1), h, w)).float())
    src = _image(g, (NF, B, 3), H, W).float()
    gcolor = torch.randn(S, NF, B, 3, H, W, generator=g, dtype=torch.float64).float()
    gres = [torch.randn(B, 3, H, W, generator=g, dtype=torch.float64).float() for _ in range(S * NF)]
    return dict(K=K32, invK=invK32, T=T.float(), disp=disp, cflow=cflow, mask=mask, src=src, gcolor=gcolor, gres=gres)


_VS_INPUTS = {}


def vs_inputs(run):
    """(t, cond) of one run: the inputs with gcolor zeroed at the run's fragile pixels and gres reduced to the tensors that are given
    (None elsewhere); cond = the shares of fragile / clipped / unclipped pixels and the smallest |z + 1e-7|, all from float64."""
    if run not in _VS_INPUTS:
        cid, mode, which = run
        case = VS_BY_ID[cid]
        t = vs_raw_inputs(case)
        fwd = vs_reference(t, case, mode, backward=False)
        H, W = case["H"], case["W"]
        ix = (fwd["sample"][..., 0] + 1) / 2 * (W - 1)                   # (S, NF, B, H, W)
        iy = (fwd["sample"][..., 1] + 1) / 2 * (H - 1)

        def axis_state(v, n):
            inside = (v > 0) & (v < n - 1)
            near_edge = (v.abs() < DELTA) | ((v - (n - 1)).abs() < DELTA)
            return inside, near_edge | (inside & ((v - v.round()).abs() < DELTA))

        in_x, fr_x = axis_state(ix, W)
        in_y, fr_y = axis_state(iy, H)
        fragile = fr_x | fr_y
        t["gcolor"] = t["gcolor"] * (~fragile)[:, :, :, None].float()
        given = gres_given(case, which) if mode >= 1 else [False] * (case["S"] * case["NF"])
        t["gres"] = [a if k else None for a, k in zip(t["gres"], given)]
        cond = dict(fragile=float(fragile.double().mean()), clipped=float((~(in_x & in_y)).double().mean()),
                    unclipped=float((in_x & in_y).double().mean()), min_abs_z=fwd["min_abs_z"], behind=fwd["behind"])
        _VS_INPUTS[run] = (t, cond)
    return _VS_INPUTS[run]


def ph_inputs(case):
    """color (S, NF, B, 3, H, W), target (B, 3, H, W), src (NF, B, 3, H, W), noise (S, B, NF, H, W) (both None without automask), gp (S,):
    fp32 CPU tensors.  Every candidate is the target plus a perturbation whose amplitude varies over the image, so every candidate wins
    somewhere.  The tie noise is 2 + N(0, 1): with a mean, noise added to the wrong candidates moves p_photo past its bar."""
    S, NF, B, H, W = (case[k] for k in ("S", "NF", "B", "H", "W"))
    g = _gen(case["seed"])
    target = _image(g, (B, 3), H, W)
    pert = lambda lead: (target + (0.03 + 0.3 * (0.5 + 0.5 * _field(g, lead + (1,), H, W))) * _field(g, lead + (3,), H, W)).clamp(0.1, 0.9)
    color = pert((S, NF, B)).float()
    target = target.float()
    src = noise = None
    if case["automask"]:
        src = pert((NF, B)).float()
        noise = (2 + torch.randn(S, B, NF, H, W, generator=g, dtype=torch.float64)).float()
    sp = case["special"]
    if sp == "flat":
        color[0, 0, :, :, 2:9, 5:37] = target[:, :, 2:9, 5:37]
    elif sp == "tie_warped":
        color[:, 1] = color[:, 0]
    elif sp == "tie_identity":
        color = src[None].expand(S, NF, B, 3, H, W).contiguous()
        noise = torch.zeros_like(noise)
    gp = (0.5 + torch.rand(S, generator=g, dtype=torch.float64)).float()
    return dict(color=color, target=target, src=src, noise=noise, gp=gp)


def ph_argmin_map(case, which, ref_argmin):
    """(S, B, H, W) uint8: the reference's own map, a seeded random map over 0 .. NC - 1, or all-identity (candidate 0) under automask."""
    if which == "reference":
        return ref_argmin
    if which == "identity":
        return torch.zeros_like(ref_argmin)
    nc = case["NF"] * (2 if case["automask"] else 1)
    return torch.randint(0, nc, ref_argmin.shape, generator=_gen(case["seed"] + 77)).to(torch.uint8)


# ---- view synthesis reference ---------------------------------------------------------------------------------------------------------
def up_matrix(n, N, dtype=torch.float64):
    """(n, N): the weight of low-resolution index i in the bilinearly upsampled value at full-resolution index y (align_corners = False)."""
    return F.interpolate(torch.eye(n, dtype=dtype)[None], size=N, mode="linear", align_corners=False)[0]


def sample_border(src_all, f, grid, stop_gradient=True, beyond=False):
    """grid_sample(src_all[f], grid, padding_mode="border", align_corners=True) restated tap by tap, for the defects: `stop_gradient` =
    False lets the gradient through the border clip; `beyond` = True READS the taps one past the last column / row from flat memory (whatever
    follows there; NaN behind the end of the buffer, as the GPU test's guard has it) instead of giving them the value 0."""
    NF, B, _, H, W = src_all.shape
    flat = torch.cat([src_all.reshape(-1), torch.full((W + 2,), math.nan, dtype=src_all.dtype)])

    def clip(v, n):
        c = v.clamp(0, n - 1)
        return torch.where((v > 0) & (v < n - 1), v, c.detach()) if stop_gradient else v + (c - v).detach()

    ix, iy = clip((grid[..., 0] + 1) / 2 * (W - 1), W), clip((grid[..., 1] + 1) / 2 * (H - 1), H)          # (B, H, W)
    x0, y0 = ix.detach().floor().long(), iy.detach().floor().long()
    tx, ty = (ix - x0)[:, None], (iy - y0)[:, None]
    base = ((f * B + torch.arange(B).view(B, 1, 1, 1)) * 3 + torch.arange(3).view(1, 3, 1, 1)) * H * W

    def tap(yk, xk):
        idx = base + (yk * W + xk)[:, None]
        ok = ((yk < H) & (xk < W))[:, None]
        if beyond:
            return flat[idx]
        return torch.where(ok, flat[torch.where(ok, idx, torch.zeros_like(idx))], torch.zeros((), dtype=flat.dtype))

    return (tap(y0, x0) * (1 - tx) * (1 - ty) + tap(y0, x0 + 1) * tx * (1 - ty) + tap(y0 + 1, x0) * (1 - tx) * ty
            + tap(y0 + 1, x0 + 1) * tx * ty)


def vs_reference(t, case, mode, dtype=torch.float64, backward=True, defect=None):
    """All outputs of uenc_view_synth_fwd and (with `backward`) uenc_view_synth_bwd in the kernel's layouts, per-(scale, frame) lists
    stacked: color (S, NF, B, 3, H, W), sample / sample_ego / sample_cmp (S, NF, B, H, W, 2), depth (S, B, 1, H, W), residual
    (S NF, B, 3, H, W); gdisp: S tensors (B, 1, h, w), gcflow / gmask: S NF tensors, gT and its absolute companion A_gT (NF, B, 4, 4);
    min_abs_z = the smallest |z + 1e-7| of any projection."""
    B, H, W, S, NF = (case[k] for k in ("B", "H", "W", "S", "NF"))
    HW = H * W
    cv = lambda a: a.to(dtype)
    K, invK, src = cv(t["K"]), cv(t["invK"]), cv(t["src"])
    low = dict(disp=[cv(a) for a in t["disp"]], cflow=[cv(a) for a in t["cflow"]] if mode >= 1 else [],
               mask=[cv(a) for a in t["mask"]] if mode == 2 else [])
    Tpp = cv(t["T"])[None, :, :, None].expand(S, NF, B, HW, 4, 4).clone()                    # one copy per pixel: per-pixel contributions
    gather_defect = defect == "gather_row_short"
    up = lambda a: F.interpolate(a, (H, W), mode="bilinear", align_corners=defect == "up_align_corners")
    if backward:
        Tpp.requires_grad_(True)
        if not gather_defect:
            for v in low.values():
                for a in v:
                    a.requires_grad_(True)
    ups = {k: [up(a) for a in v] for k, v in low.items()}
    if backward and gather_defect:                                          # the gradient of the UPSAMPLED maps; stage B is restated below
        ups = {k: [a.detach().requires_grad_(True) for a in v] for k, v in ups.items()}
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing="ij")
    rays = invK[:, :3, :3] @ torch.stack([xs.reshape(-1), ys.reshape(-1), torch.ones(HW, dtype=dtype)], 0)[None]       # (B, 3, HW)
    zs, nbehind = [], [0]

    def xform(Tm, X):                                                       # (B, HW, 4, 4), (B, 3, HW) -> (B, 4, HW)
        P = (Tm[..., :3] * X.permute(0, 2, 1)[:, :, None, :]).sum(-1) + Tm[..., 3]
        return P.permute(0, 2, 1)

    def proj(P4):
        cam = K[:, :3, :] @ P4
        z = cam[:, 2] + 1e-7
        zs.append(float(z.detach().abs().min()))
        nbehind[0] += int((z.detach() < 0).sum())
        px, py = cam[:, 0] / z, cam[:, 1] / z
        return torch.stack([(px / (W - 1) - 0.5) * 2, (py / (H - 1) - 0.5) * 2], -1).view(B, H, W, 2)

    hom = lambda X3: torch.cat([X3, torch.ones_like(X3[:, :1])], 1)
    out = {n: [] for n in ("color", "sample", "sample_ego", "sample_cmp", "depth", "residual")}
    for s in range(S):
        depth = 1 / (0.01 + 9.99 * ups["disp"][s])
        out["depth"].append(depth)
        X = depth.reshape(B, 1, HW) * rays
        for f in range(NF):
            sf = s * NF + f
            Pe = xform(Tpp[s, f], X)
            if mode == 0:
                sample = proj(Pe)
            else:
                ego = Pe[:, :3] - X
                cf = ups["cflow"][sf].reshape(B, 3, HW)
                res = cf + ego if defect == "residual_ego_sign" else cf - ego
                out["sample_ego"].append(proj(Pe))
                Pc = hom(X + cf)
                cmpl = proj(Pc)
                out["sample_cmp"].append(cmpl)
                out["residual"].append(res.reshape(B, 3, H, W))
                if mode == 1:
                    sample = proj(xform(Tpp[s, f], X + cf)) if defect == "mode1_through_T" else cmpl
                else:
                    sample = proj(xform(Tpp[s, f], X + res * ups["mask"][sf].reshape(B, 1, HW)))
            out["sample"].append(sample)
            if defect == "clip_without_gradient_stop":
                color = sample_border(src, f, sample, stop_gradient=False)
            elif defect == "tap_beyond_last_column_read":
                color = sample_border(src, f, sample, beyond=True)
            else:
                color = F.grid_sample(src[f], sample, padding_mode="border", align_corners=True)
            out["color"].append(color)
    r = dict(color=torch.stack(out["color"]).view(S, NF, B, 3, H, W), depth=torch.stack(out["depth"]))
    r["sample"] = torch.stack(out["sample"]).view(S, NF, B, H, W, 2)
    if mode >= 1:
        r["sample_ego"] = torch.stack(out["sample_ego"]).view(S, NF, B, H, W, 2)
        r["sample_cmp"] = torch.stack(out["sample_cmp"]).view(S, NF, B, H, W, 2)
        r["residual"] = torch.stack(out["residual"])
    res = {k: v.detach() for k, v in r.items()}
    res["min_abs_z"] = min(zs)
    res["behind"] = nbehind[0]                                             # projections with z < 0
    if not backward:
        return res
    per_channel = (cv(t["gcolor"]) * r["color"]).sum((0, 1, 2, 4, 5))              # the three colour channels' shares of the loss
    loss = per_channel.sum()
    if mode >= 1 and defect != "gres_ignored":
        for sf, gr in enumerate(t["gres"]):
            if gr is not None:
                loss = loss + (cv(gr) * r["residual"][sf]).sum()
    if defect is None and dtype == torch.float64:
        # the same sum with every pixel's contribution split into its colour channels (and the rest): what cancels INSIDE a pixel
        grad_T = lambda v: torch.autograd.grad(v, Tpp, retain_graph=True, allow_unused=True)[0]
        parts = [g if g is not None else torch.zeros_like(Tpp) for g in map(grad_T, per_channel)]
        whole = grad_T(loss)
        rest = (whole if whole is not None else torch.zeros_like(Tpp)) - sum(parts)
        res["A_gT_channels"] = (sum(p.abs() for p in parts) + rest.abs()).sum((0, 3))
    leaves = [Tpp] + [a for k in ("disp", "cflow", "mask") for a in (ups if gather_defect else low)[k]]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(a) for g, a in zip(grads, leaves)]
    res["gT"], res["A_gT"] = grads[0].sum((0, 3)), grads[0].abs().sum((0, 3))
    g = iter(grads[1:])
    for k, name in (("disp", "gdisp"), ("cflow", "gcflow"), ("mask", "gmask")):
        res[name] = [next(g) for _ in low[k]]
        if gather_defect:                                                   # stage B restated, its footprint one row short at the top
            for i, gu in enumerate(res[name]):
                s = i if k == "disp" else i // NF
                h, w, rr = H >> s, W >> s, 1 << s
                Wy, Wx = up_matrix(h, H, dtype), up_matrix(w, W, dtype)
                if s >= 1:
                    for lo in range(1, h):
                        Wy[lo, rr * lo - rr // 2] = 0
                res[name][i] = torch.einsum("iy,bcyx,jx->bcij", Wy, gu, Wx)
    for name in ("gcflow", "gmask"):
        if not res[name]:
            del res[name]
    return res


def item_scale(name, r64):
    """M: max |r64| over every (scale, frame, image) item of a dense output, broadcastable against r64."""
    lead = LEAD[name]
    m = r64.abs().flatten(lead).amax(-1)
    return m.view(m.shape + (1,) * (r64.dim() - lead))


def share_of_bar(got, r64, scale, kappa):
    """(largest |got - r64| / (kappa 2^-24 scale), largest |got - r64|); where the scale is 0 the output must be exactly r64 (share 0 or
    inf); a NaN or inf in `got` is inf."""
    err = (got.double() - r64).abs()
    err = torch.where(err.isfinite(), err, torch.full_like(err, math.inf))
    bar = (kappa * U24 * scale).expand_as(err)
    share = torch.where(bar > 0, err / bar.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, math.inf)))
    return float(share.max()), float(err.max())


def judge(name, got, r64, A=None, kappa=None):
    """Worst share of the bar of one output (a tensor, or a list of per-item-index tensors of shape (B, ...))."""
    kappa = KAPPA[name] if kappa is None else kappa
    if A is not None:
        return share_of_bar(got, r64, A, kappa)
    if isinstance(r64, (list, tuple)):
        figs = [share_of_bar(g, r, item_scale(name, r[None])[0], kappa) for g, r in zip(got, r64)]
        return max(f[0] for f in figs), max(f[1] for f in figs)
    return share_of_bar(got, r64, item_scale(name, r64), kappa)


# ---- photometric reference ------------------------------------------------------------------------------------------------------------
def ssim_loss(x, y, pad="reflect"):
    x, y = F.pad(x, (1, 1, 1, 1), mode=pad), F.pad(y, (1, 1, 1, 1), mode=pad)
    mu_x, mu_y = F.avg_pool2d(x, 3, 1), F.avg_pool2d(y, 3, 1)
    sigma_x = F.avg_pool2d(x ** 2, 3, 1) - mu_x ** 2
    sigma_y = F.avg_pool2d(y ** 2, 3, 1) - mu_y ** 2
    sigma_xy = F.avg_pool2d(x * y, 3, 1) - mu_x * mu_y
    n = (2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)
    d = (mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2)
    return torch.clamp((1 - n / d) / 2, 0, 1)


def reprojection(pred, target, pad="reflect"):
    """(B, H, W): 0.85 mean_c SSIM + 0.15 mean_c L1."""
    return 0.85 * ssim_loss(pred, target, pad).mean(1) + 0.15 * (target - pred).abs().mean(1)


def ph_forward(t, case, dtype=torch.float64, defect=None):
    """values (S, NC, B, H, W), argmin (S, B, H, W) uint8 (the first on a tie), gap (S, B, H, W) = second smallest - smallest (inf with one
    candidate), p_photo (S,) and A (S,) = sum |minimum| / (B H W)."""
    S, NF, B, H, W = (case[k] for k in ("S", "NF", "B", "H", "W"))
    pad = "replicate" if defect == "ssim_replicate_pad" else "reflect"
    color, target = t["color"].to(dtype), t["target"].to(dtype)
    vals = []
    for s in range(S):
        warped = [reprojection(color[s, f], target, pad) for f in range(NF)]
        cands = warped
        if case["automask"]:
            ident = [reprojection(t["src"][f].to(dtype), target, pad) for f in range(NF)]
            nz = [t["noise"][s, :, f].to(dtype) * TIE_NOISE_SCALE for f in range(NF)]
            if defect == "noise_on_warped":
                warped = [v + n for v, n in zip(warped, nz)]
            else:
                ident = [v + n for v, n in zip(ident, nz)]
            cands = ident + warped
        vals.append(torch.stack(cands))
    vals = torch.stack(vals)
    best, arg = vals[:, 0].clone(), torch.zeros(S, B, H, W, dtype=torch.uint8)
    for c in range(1, vals.shape[1]):
        take = vals[:, c] <= best if defect == "second_wins_ties" else vals[:, c] < best
        best = torch.where(take, vals[:, c], best)
        arg = torch.where(take, torch.full_like(arg, c), arg)
    srt = vals.sort(1).values
    gap = srt[:, 1] - srt[:, 0] if vals.shape[1] > 1 else torch.full_like(best, math.inf)
    count = H * W if defect == "mean_without_B" else B * H * W
    return dict(values=vals, argmin=arg, gap=gap, p_photo=best.sum((1, 2, 3)) / count, A=best.abs().sum((1, 2, 3)) / (B * H * W))


def judged_pixels(fwd64, kappa=None):
    """(S, B, H, W) bool: where the argmin is compared -- the two smallest float64 values differ by more than twice the per-pixel value bar."""
    kappa = KAPPA["photo_value"] if kappa is None else kappa
    vmax = fwd64["values"].abs().amax((1, 3, 4))                                                  # (S, B)
    return fwd64["gap"] > 2 * kappa * U24 * vmax[:, :, None, None]


def _reflect_index(n):
    i = torch.arange(-1, n + 1).abs()
    return torch.where(i >= n, 2 * n - 2 - i, i)


def ph_backward(t, case, argmin, dtype=torch.float64, defect=None):
    """grad_color (S, NF, B, 3, H, W) = d(sum_s gp[s] p_photo[s]) / d color with the selection `argmin` held fixed."""
    S, NF, B, H, W = (case[k] for k in ("S", "NF", "B", "H", "W"))
    color = t["color"].to(dtype).clone().requires_grad_(True)
    target, gp = t["target"].to(dtype), t["gp"].to(dtype)
    first = NF if case["automask"] else 0
    pad = "replicate" if defect == "ssim_replicate_pad" else "reflect"
    sel = torch.stack([torch.stack([(argmin[s] == first + f) for f in range(NF)]) for s in range(S)]).to(dtype)       # (S, NF, B, H, W)
    w = sel * (gp / (B * H * W)).view(S, 1, 1, 1, 1)
    if defect == "reflect_counted_once_bwd":
        # SSIM from explicit 3x3 patches, so that the fold back to the image can drop the second copy of a reflected pixel
        x = color.detach().flatten(0, 2)
        y = target[None, None].expand(S, NF, B, 3, H, W).flatten(0, 2)
        patches = lambda a: F.pad(a, (1, 1, 1, 1), mode="reflect").unfold(2, 3, 1).unfold(3, 3, 1)
        Px, Py = patches(x).clone().requires_grad_(True), patches(y)
        mu_x, mu_y = Px.mean((-1, -2)), Py.mean((-1, -2))
        sx, sy, sxy = (Px ** 2).mean((-1, -2)) - mu_x ** 2, (Py ** 2).mean((-1, -2)) - mu_y ** 2, (Px * Py).mean((-1, -2)) - mu_x * mu_y
        l = torch.clamp((1 - (2 * mu_x * mu_y + C1) * (2 * sxy + C2) / ((mu_x ** 2 + mu_y ** 2 + C1) * (sx + sy + C2))) / 2, 0, 1)
        (gP,) = torch.autograd.grad((0.85 * l.mean(1) * w.flatten(0, 2)).sum(), Px)                # (N, 3, H, W, 3, 3)
        ry, rx = _reflect_index(H), _reflect_index(W)
        grad = torch.zeros_like(x)
        for dy in range(3):                                                 # tap row = centre + dy - 1
            keep_y = torch.ones(H, dtype=dtype)
            if dy == 0:
                keep_y[0] = 0                                               # centre 0: the taps above and below are the same pixel
            if dy == 2:
                keep_y[H - 1] = 0
            for dx in range(3):
                keep_x = torch.ones(W, dtype=dtype)
                if dx == 0:
                    keep_x[0] = 0
                if dx == 2:
                    keep_x[W - 1] = 0
                gk = gP[..., dy, dx] * keep_y.view(H, 1) * keep_x.view(1, W)
                rows = torch.zeros_like(x).index_add_(2, ry[dy:dy + H], gk)
                grad += torch.zeros_like(x).index_add_(3, rx[dx:dx + W], rows)
        l1 = (0.15 * (target - color).abs().mean(3) * w).sum()
        (g1,) = torch.autograd.grad(l1, color)
        return grad.view(S, NF, B, 3, H, W) + g1
    loss = sum((reprojection(color[s, f], target, pad) * w[s, f]).sum() for s in range(S) for f in range(NF))
    (grad,) = torch.autograd.grad(loss, color)
    if defect == "l1_sign_plus_at_zero":
        grad = grad + (color.detach() == target).to(dtype) * (0.15 / 3) * w[:, :, :, None]
    return grad


def selected_near(case, argmin):
    """(S, NF, B, 1, H, W) bool: a window centre within one pixel selected warped frame f (elsewhere its gradient is exactly 0)."""
    NF = case["NF"]
    first = NF if case["automask"] else 0
    sel = torch.stack([(argmin == first + f) for f in range(NF)], 1).float()                     # (S, NF, B, H, W)
    return (F.max_pool2d(sel.flatten(0, 1), 3, 1, 1) > 0).view(sel.shape)[:, :, :, None]
