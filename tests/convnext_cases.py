"""Shared by tests/test_convnext_cases_cpu.py and tests/test_convnext_kernels_gpu.py: the case tables of the ConvNeXt kernels (the fused
7x7 depthwise convolution + LayerNorm of csrc/dwconv.hip, its two backward kernels, the layer-scale gradient step, and `ops.conv2x2_s2`),
their seeded inputs and their references.

Nothing here imports `uenc` at module level.  Inputs come from the name-hashed generators of tests/convnext_fixture.py: activations and
upstream gradients are multiples of 1/64 in [-2, 2) (exact in bf16), parameters are fp32 draws.  Every reference is a plain torch
composition (F.conv2d(groups=C) + F.layer_norm + autograd) that runs in the dtype it is asked for: float64 is the reference proper, fp32
on the CPU is the yardstick for the outputs whose rounding error has no closed bound.  Each reference also returns the absolute-value
companion of every output whose error is bounded in closed form (the same sum with every term replaced by its magnitude).
"""
import numpy as np
import torch
import torch.nn.functional as F

import convnext_fixture as CF

EPS = 1e-6
U24 = 2.0 ** -24

# the kernels' tiling constants (csrc/dwconv.hip), restated: the CPU tests compute every reachability claim from them
TH = TW = 8
CS = 32
HALO_FLOATS = (TH + 6) * (TW + 6) * CS
YLDS_MAX_C = 384
NACC = 50
WGRAD_MAX_BLOCKS = 256
LDS_LIMIT_BYTES = 160 * 1024

# ---- depthwise convolution + LayerNorm: (B, H, W, C) ------------------------------------------------------------------------------
ORIGINAL = [(2, 5, 9, 40), (1, 2, 3, 320), (1, 3, 5, 1536), (1, 16, 24, 192), (2, 7, 7, 8)]          # tests/test_convnext_gpu.py SHAPES
CASE_A = (1, 136, 128, 8)        # 17 x 16 = 272 full tiles > 256: sixteen workgroups of the weight gradient take a second tile
CASE_B = (3, 77, 75, 8)          # 3 x 10 x 10 = 300 tiles: the stride crosses images; last tile row 5 rows, last tile column 3 columns
CASE_C = (2, 17, 9, 384)         # widest LDS-resident y tile, 3 x 2 tiles, both edges ragged by one pixel
CASE_D = (2, 17, 9, 392)         # first width on the L2 re-read path, same geometry; the last slab has 8 active lanes
CASE_E = (1, 9, 17, 1536)        # L2 path, NV = 8 LayerNorm backward, 2 x 3 tiles
CASE_F = (1, 40, 40, 192)        # M = 1600: 400 LayerNorm-backward blocks x 384 > 131072, partials stored, ln_bwd_param_kernel runs
CASE_G1 = (1, 8, 8, 40)          # exactly one full tile
CASE_G2 = (1, 1, 1, 8)           # one pixel
NEW = [CASE_A, CASE_B, CASE_C, CASE_D, CASE_E, CASE_F, CASE_G1, CASE_G2]
DW_CASES = NEW + ORIGINAL
STRIDING = [CASE_A, CASE_B]      # the weight-gradient tile walk takes a second trip

# ---- layer scale: (N, K) x pointer pattern ---------------------------------------------------------------------------------------
LS_SHAPES = [(5, 160), (3, 256), (4, 257), (2, 1280)]
# name -> which of (db2p, b2, gw2, gb2, ggamma) are passed
LS_PATTERNS = {
    "all": dict(db2p=True, b2=True, gw2=True, gb2=True, ggamma=True),
    "no_gw2": dict(db2p=True, b2=True, gw2=False, gb2=True, ggamma=True),
    "no_gb2_db2p": dict(db2p=False, b2=True, gw2=True, gb2=False, ggamma=True),
    "no_b2": dict(db2p=True, b2=False, gw2=True, gb2=True, ggamma=True),
    "only_ggamma": dict(db2p=True, b2=True, gw2=False, gb2=False, ggamma=True),
}

# ---- conv2x2_s2: (B, H, W, Cin, Cout, input dtype) ---------------------------------------------------------------------------------
C2_CASES = [(2, 8, 12, 40, 80, "f32"), (1, 9, 12, 16, 24, "f32"), (1, 8, 13, 16, 24, "f32"), (2, 7, 5, 8, 16, "f32"),
            (1, 9, 13, 16, 24, "bf16")]

# ---- accept / reject tables: (id, entry point, (B, H, W, C), what is wrong, expected status) ----------------------------------------
OK, EINVAL = 0, -1
TINY = (1, 2, 3, 8)
DW_STATUS = [
    ("fwd-ok", "fwd", TINY, None, OK),
    ("fwd-ok-no-bias", "fwd", TINY, "no:b", OK),
    ("fwd-c-not-8", "fwd", (1, 2, 3, 12), None, EINVAL),
    ("fwd-c-6152", "fwd", (1, 1, 1, 6152), None, EINVAL),
    ("fwd-b-65536", "fwd", (65536, 1, 1, 8), None, EINVAL),
    ("fwd-x-misaligned", "fwd", TINY, "misalign:x", EINVAL),
    ("fwd-y-misaligned", "fwd", TINY, "misalign:y", EINVAL),
    ("fwd-h-dtype", "fwd", TINY, "h_dtype:2", EINVAL),
    ("bwd-ok", "bwd_data", TINY, None, OK),
    ("bwd-ok-no-dout-no-params", "bwd_data", TINY, "no:dout,dgamma,dbeta", OK),
    ("bwd-c-6152", "bwd_data", (1, 1, 1, 6152), None, EINVAL),
    ("bwd-b-65536", "bwd_data", (65536, 1, 1, 8), None, EINVAL),
    ("bwd-dh-misaligned", "bwd_data", TINY, "misalign:dh", EINVAL),
    ("bwd-y-misaligned", "bwd_data", TINY, "misalign:y", EINVAL),
    ("bwd-dy-is-dx", "bwd_data", TINY, "alias:dx=dy", EINVAL),
    ("bwd-dgamma-without-dbeta", "bwd_data", TINY, "no:dbeta", EINVAL),
    ("bwd-dbeta-without-dgamma", "bwd_data", TINY, "no:dgamma", EINVAL),
    ("wgrad-ok", "bwd_weight", TINY, None, OK),
    ("wgrad-ok-no-db", "bwd_weight", TINY, "no:db", OK),
    ("wgrad-c-6152", "bwd_weight", (1, 1, 1, 6152), None, EINVAL),
    ("wgrad-b-65536", "bwd_weight", (65536, 1, 1, 8), None, EINVAL),
    ("wgrad-short-workspace", "bwd_weight", TINY, "short_ws", EINVAL),
    ("wgrad-x-misaligned", "bwd_weight", TINY, "misalign:x", EINVAL),
    ("wgrad-no-dw", "bwd_weight", TINY, "no:dw", EINVAL),
]
# (id, (N, K), what is wrong, expected status)
LS_STATUS = [
    ("ls-ok", (3, 40), None, OK),
    ("ls-no-outputs", (3, 40), "no:gw2,gb2,ggamma", EINVAL),
    ("ls-gb2-without-db2p", (3, 40), "no:db2p", EINVAL),
    ("ls-in-place", (3, 40), "alias:gw2=dw2p", EINVAL),
    ("ls-n-zero", (0, 40), None, EINVAL),
    ("ls-k-zero", (3, 0), None, EINVAL),
]


def sid(shape) -> str:
    return "x".join(map(str, shape))


# ---- geometry, restated from the kernels ---------------------------------------------------------------------------------------------
def tiles(shape):
    B, H, W, _ = shape
    return B * (-(-H // TH)) * (-(-W // TW))


def wgrad_blocks(shape) -> int:
    return min(tiles(shape), WGRAD_MAX_BLOCKS)


def wgrad_trips(shape) -> int:
    """Most tiles one workgroup of dwconv7_wgrad_partial_kernel walks."""
    return -(-tiles(shape) // wgrad_blocks(shape))


def fwd_lds_bytes(C: int) -> int:
    return 4 * (HALO_FLOATS + (TH * TW * C if C <= YLDS_MAX_C else 0))


def k_y() -> int:
    """y = 49 fused multiply-adds on top of the bias, one rounding each: |error| <= ((1 + u)^49 - 1) * companion < 50 u * companion."""
    return 50


def k_mean(C: int) -> int:
    """mean = (sum over C of y) / C: y's own 50, then ceil(C / 32) slab additions per lane, 5 butterfly levels, the rounding of 1 / C and the
    multiplication by it."""
    return 50 + -(-C // CS) + 5 + 2


def k_wgrad(shape) -> int:
    """Roundings a term of dw (or db) passes through: the 8-pixel chain of a thread, one addition per tile the workgroup walks, the
    half-wave pair, two levels over the 4 waves, NB sequential additions in the final kernel, and the += into the gradient."""
    return 8 + wgrad_trips(shape) + 1 + 2 + wgrad_blocks(shape) + 1


def bf16_half_ulp(v):
    """Half a unit in the last place of bf16 (8-bit significand) at the magnitude of each element of v: 2^(floor(log2 |v|) - 8)."""
    a = v.abs()
    return torch.where(a > 0, torch.ldexp(torch.ones_like(a), torch.frexp(a).exponent - 9), torch.zeros_like(a))


def bf16_allowance(r64, bar):
    """The bar of a value stored as bf16: it is the rounding to nearest of an fp32 value v with |v - r64| <= bar, so it lies within
    half an ulp of v (at most that of |r64| + bar: the half-ulp does not decrease with the magnitude) plus bar of r64."""
    return bf16_half_ulp(r64.abs() + bar) + bar


def k_layer_scale(K: int) -> int:
    """ggamma: ceil(K / 256) multiply-adds per thread, 6 wave-butterfly levels, 2 levels over the 4 waves, product and addition of the bias
    term, and the += ."""
    return -(-K // 256) + 6 + 2 + 2 + 1


# ---- depthwise convolution + LayerNorm -----------------------------------------------------------------------------------------------
_INPUTS = {}
_REF = {}


def dw_inputs(shape):
    """fp32 CPU tensors of one case: x, dh, dout (multiples of 1/64), w (C, 1, 7, 7), b, g, be, and non-zero prefills (pre_dbeta a
    multiple of 1/64 in [2, 6), so that dbeta stays exact and no channel starts from zero)."""
    if shape not in _INPUTS:
        B, H, W, C = shape
        tag = sid(shape)
        _INPUTS[shape] = {
            "x": CF.input_for("op_x" + tag, shape), "w": CF.tensor_for("op." + tag + ".dw", (C, 1, 7, 7)) * 4,
            "b": CF.tensor_for("op." + tag + ".bias", (C,)), "g": CF.tensor_for("op." + tag + ".weight", (C,)),
            "be": CF.tensor_for("op." + tag + ".beta", (C,)), "dh": CF.input_for("op_dh" + tag, shape),
            "dout": CF.input_for("op_dout" + tag, shape),
            "pre_dgamma": CF.tensor_for("pre." + tag + ".dgamma", (C,)), "pre_dbeta": CF.input_for("pre_dbeta" + tag, (C,)) + 4,
            "pre_dw": CF.tensor_for("pre." + tag + ".dw", (C, 1, 7, 7)), "pre_db": CF.tensor_for("pre." + tag + ".db", (C,))}
    return _INPUTS[shape]


def conv(x, w, b=None):
    """x (B, H, W, C), w (C, 1, 7, 7) -> (B, H, W, C): the depthwise 7x7 cross-correlation, padding 3."""
    return F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=3, groups=x.shape[-1]).permute(0, 2, 3, 1)


def dw_reference(shape, dtype=torch.float64):
    """-> dict of y, h, mean, rstd, dy (gradient at y), dx0 (without dout), dx, dgamma, dbeta (prefill + gradient) in `dtype` on the CPU,
    computed once per (shape, dtype).  float64 also returns the companions abs_y (conv(|x|, |w|) + |b|) and abs_dbeta."""
    key = (shape, dtype)
    if key in _REF:
        return _REF[key]
    C = shape[-1]
    t = dw_inputs(shape)
    d = {k: t[k].to(dtype).requires_grad_(True) for k in ("x", "w", "b", "g", "be")}
    y = conv(d["x"], d["w"], d["b"])
    h = F.layer_norm(y, (C,), d["g"], d["be"], EPS)
    dh = t["dh"].to(dtype)
    gy, gx, gg, gbe = torch.autograd.grad(h, [y, d["x"], d["g"], d["be"]], dh)
    yd = y.detach()
    ref = {"y": yd, "h": h.detach(), "mean": yd.mean(-1), "rstd": (yd.var(-1, unbiased=False) + EPS).rsqrt(), "dy": gy, "dx0": gx,
           "dx": gx + t["dout"].to(dtype), "dgamma": t["pre_dgamma"].to(dtype) + gg, "dbeta": t["pre_dbeta"].to(dtype) + gbe,
           "var": yd.var(-1, unbiased=False)}
    if dtype == torch.float64:
        ref["abs_y"] = conv(t["x"].double().abs(), t["w"].double().abs(), t["b"].double().abs())
        ref["abs_dbeta"] = t["pre_dbeta"].double().abs() + dh.abs().sum((0, 1, 2))
    _REF[key] = ref
    return ref


def wgrad_operand(shape):
    """The weight-gradient kernel's dy operand: the float64 reference's dy rounded to fp32 (what a correct LayerNorm backward hands on)."""
    return dw_reference(shape)["dy"].float()


def wgrad_reference(shape):
    """float64 dw, db of the weight-gradient kernel on (wgrad_operand, x) with the prefill added, and their companions
    |prefill| + sum |dy| |x| per tap and |prefill| + sum |dy|."""
    key = (shape, "wgrad")
    if key not in _REF:
        t = dw_inputs(shape)
        C = shape[-1]
        dy = wgrad_operand(shape).double()
        x = t["x"].double()

        def grads(xx, dd):
            w = torch.zeros(C, 1, 7, 7, dtype=torch.float64, requires_grad=True)
            return torch.autograd.grad(conv(xx, w), w, dd)[0]
        _REF[key] = {"dw": t["pre_dw"].double() + grads(x, dy), "db": t["pre_db"].double() + dy.sum((0, 1, 2)),
                     "abs_dw": t["pre_dw"].double().abs() + grads(x.abs(), dy.abs()),
                     "abs_db": t["pre_db"].double().abs() + dy.abs().sum((0, 1, 2))}
    return _REF[key]


def conv_by_taps(x, w, b):
    """An independent statement of `conv`: 49 shifted slices of the zero-padded map, each scaled by its tap."""
    B, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 3, 3, 3, 3))
    out = b.expand(B, H, W, C).clone()
    for ky in range(7):
        for kx in range(7):
            out += xp[:, ky:ky + H, kx:kx + W] * w[:, 0, ky, kx]
    return out


def wgrad_emulated(shape):
    """dw (C, 49) and db (C) as fp32 arithmetic in the weight-gradient kernels' own summation order (without prefill): per thread an
    8-pixel multiply-add chain per tile row and tap, added to the accumulator once per tile in the order nb, nb + NB, ...; rows r and
    r + 1 of a wave (the `xor 32` pair); the 4 waves as (0 + 1) + (2 + 3); the NB partials in ascending nb.  A fused multiply-add is
    emulated as the fp32 rounding of the float64 product-sum."""
    B, H, W, C = shape
    f32 = np.float32
    x = dw_inputs(shape)["x"].numpy()
    dy = wgrad_operand(shape).numpy()
    tY, tX = -(-H // TH), -(-W // TW)
    nt, NB = B * tY * tX, wgrad_blocks(shape)
    xp = np.zeros((B, tY * TH + 6, tX * TW + 6, C), f32)
    xp[:, 3:3 + H, 3:3 + W] = x
    gp = np.zeros((B, tY * TH, tX * TW, C), f32)
    gp[:, :H, :W] = dy
    halo = np.empty((nt, TH + 6, TW + 6, C), f32)
    g = np.empty((nt, TH, TW, C), f32)
    for tile in range(nt):
        b, rem = divmod(tile, tY * tX)
        ty, tx = divmod(rem, tX)
        halo[tile] = xp[b, ty * TH:ty * TH + TH + 6, tx * TW:tx * TW + TW + 6]
        g[tile] = gp[b, ty * TH:(ty + 1) * TH, tx * TW:(tx + 1) * TW]
    per_tile = np.zeros((nt, TH, NACC, C), f32)                    # what one thread row adds to its accumulators for one tile
    gs = np.zeros((nt, TH, C), f32)
    for px in range(TW):
        gs = (gs + g[:, :, px]).astype(f32)
    per_tile[:, :, 49] = gs
    for ky in range(7):
        for kx in range(7):
            a = np.zeros((nt, TH, C), f32)
            for px in range(TW):
                a = (g[:, :, px].astype(np.float64) * halo[:, ky:ky + TH, px + kx].astype(np.float64) + a.astype(np.float64)).astype(f32)
            per_tile[:, :, ky * 7 + kx] = a
    acc = np.zeros((NB, TH, NACC, C), f32)
    for first in range(0, nt, NB):
        part = per_tile[first:first + NB]
        acc[:part.shape[0]] = (acc[:part.shape[0]] + part).astype(f32)
    pair = (acc[:, 0::2] + acc[:, 1::2]).astype(f32)                # (NB, 4 waves, 50, C)
    ws = ((pair[:, 0] + pair[:, 1]).astype(f32) + (pair[:, 2] + pair[:, 3]).astype(f32)).astype(f32)
    total = np.zeros((NACC, C), f32)
    for nb in range(NB):
        total = (total + ws[nb]).astype(f32)
    return torch.from_numpy(total[:49].T.copy()), torch.from_numpy(total[49].copy())


# ---- layer scale -------------------------------------------------------------------------------------------------------------------------
def ls_inputs(N: int, K: int):
    tag = f"ls.{N}x{K}"
    return {"dw2p": CF.tensor_for(tag + ".dw2p", (N, K)) * 8, "db2p": CF.tensor_for(tag + ".db2p", (N,)), "w2": CF.tensor_for(tag + ".w2", (N, K)) * 8,
            "b2": CF.tensor_for(tag + ".b2", (N,)), "gamma": CF.tensor_for(tag + ".gamma", (N,)),
            "gw2": CF.tensor_for(tag + ".pre_gw2", (N, K)), "gb2": CF.tensor_for(tag + ".pre_gb2", (N,)), "ggamma": CF.tensor_for(tag + ".pre_gg", (N,))}


def ls_reference(t, pattern):
    """float64 results of uenc_layer_scale_grads for the pointers `pattern` passes (prefill + gradient), and the companions."""
    d = {k: v.double() for k, v in t.items()}
    db2p = d["db2p"] if pattern["db2p"] else torch.zeros_like(d["db2p"])
    b2 = d["b2"] if pattern["b2"] else torch.zeros_like(d["b2"])
    out = {}
    if pattern["gw2"]:
        out["gw2"] = d["gw2"] + d["gamma"][:, None] * d["dw2p"]
        out["abs_gw2"] = d["gw2"].abs() + (d["gamma"][:, None] * d["dw2p"]).abs()
    if pattern["gb2"]:
        out["gb2"] = d["gb2"] + d["gamma"] * db2p
        out["abs_gb2"] = d["gb2"].abs() + (d["gamma"] * db2p).abs()
    if pattern["ggamma"]:
        out["ggamma"] = d["ggamma"] + (d["dw2p"] * d["w2"]).sum(1) + db2p * b2
        out["abs_ggamma"] = d["ggamma"].abs() + (d["dw2p"] * d["w2"]).abs().sum(1) + (db2p * b2).abs()
    return out


def ls_by_autograd(t):
    """Gradients of W2, b2, gamma through W2' = gamma[:, None] * W2, b2' = gamma * b2 with upstream (dW2', db2'), by autograd."""
    w2, b2, gamma = (t[k].double().requires_grad_(True) for k in ("w2", "b2", "gamma"))
    return torch.autograd.grad([gamma[:, None] * w2, gamma * b2], [w2, b2, gamma], [t["dw2p"].double(), t["db2p"].double()])


# ---- conv2x2_s2 ----------------------------------------------------------------------------------------------------------------------------
def c2_inputs(case):
    B, H, W, Ci, Co, dtype = case
    tag = "c2." + sid(case[:5]) + dtype
    x = CF.input_for(tag + ".x", (B, H, W, Ci))
    return {"x": x.bfloat16() if dtype == "bf16" else x, "w": CF.tensor_for(tag + ".w", (Co, Ci, 2, 2)) * 4, "b": CF.tensor_for(tag + ".b", (Co,)),
            "dy": CF.input_for(tag + ".dy", (B, H // 2, W // 2, Co))}


def c2_reference(t, round_weight: bool):
    """F.conv2d(stride=2) in float64 with autograd; round_weight: the weight as the product mode's GEMM reads it (rounded to bf16).
    -> out, dx, dw, db and their companions."""
    w = (t["w"].bfloat16() if round_weight else t["w"]).double().requires_grad_(True)
    x, b = t["x"].double().requires_grad_(True), t["b"].double().requires_grad_(True)
    run = lambda xx, ww, bb: F.conv2d(xx.permute(0, 3, 1, 2), ww, bb, stride=2).permute(0, 2, 3, 1)
    out = run(x, w, b)
    dy = t["dy"].double()
    dx, dw, db = torch.autograd.grad(out, [x, w, b], dy)
    ax, aw = x.detach().abs().requires_grad_(True), w.detach().abs().requires_grad_(True)
    aout = run(ax, aw, b.detach().abs())
    adx, adw = torch.autograd.grad(aout, [ax, aw], dy.abs())
    return {"out": out.detach(), "dx": dx, "dw": dw, "db": db, "abs_out": aout.detach(), "abs_dx": adx, "abs_dw": adw,
            "abs_db": dy.abs().sum((0, 1, 2))}


# ---- accept / reject rows as calls -------------------------------------------------------------------------------------------------------------
SENTINEL = -777.25


def _flags(what, kind):
    return [] if not what or not what.startswith(kind + ":") else what.split(":", 1)[1].split(",")


def _buf(n, device, misaligned=False, dtype=torch.float32):
    """A sentinel-filled buffer of n elements; misaligned: a view 4 bytes into a larger 16-byte-aligned allocation."""
    if not misaligned:
        return torch.full((max(n, 4),), SENTINEL, dtype=dtype, device=device)
    assert dtype == torch.float32
    return torch.full((n + 4,), SENTINEL, dtype=dtype, device=device)[1:1 + n]


def dw_status_call(row, device, stream=0):
    """Run one row of DW_STATUS with buffers on `device` -> (status, {name: output buffer}).  Every buffer has the size the row's shape asks
    for, inputs are zeros apart from rstd = 1; outputs hold SENTINEL."""
    from uenc import capi
    _, entry, (B, H, W, C), what, _ = row
    n, M = B * H * W * C, B * H * W
    mis, no = _flags(what, "misalign"), _flags(what, "no")
    zeros = lambda k, name=None: _buf(k, device, name in mis).zero_()
    p = lambda t: 0 if t is None else t.data_ptr()
    outs = {}
    if entry == "fwd":
        x, w, b, g, be = zeros(n, "x"), zeros(49 * C), None if "b" in no else zeros(C), zeros(C), zeros(C)
        outs = {"y": _buf(n, device, "y" in mis), "h": _buf(n, device), "stats": _buf(2 * M, device)}
        h_dtype = int(what.split(":")[1]) if what and what.startswith("h_dtype:") else capi.F32
        rc = capi.lib.uenc_dwconv7_ln_fwd(p(x), p(w), p(b), p(g), p(be), p(outs["y"]), p(outs["h"]), h_dtype, p(outs["stats"]), B, H, W, C,
                                          EPS, stream)
    elif entry == "bwd_data":
        dh, y, g, w = zeros(n, "dh"), zeros(n, "y"), zeros(C), zeros(49 * C)
        stats = zeros(2 * M)
        stats[1::2] = 1.0
        dout = None if "dout" in no else zeros(n)
        outs = {"dy": _buf(n, device), "dx": _buf(n, device)}
        for k in ("dgamma", "dbeta"):
            if k not in no:
                outs[k] = _buf(C, device)
        dx = outs["dy"] if what == "alias:dx=dy" else outs["dx"]
        rc = capi.lib.uenc_dwconv7_ln_bwd_data(p(dh), capi.F32, p(y), p(stats), p(g), p(w), p(dout), p(outs["dy"]), p(dx), p(outs.get("dgamma")),
                                               p(outs.get("dbeta")), 0, 0, B, H, W, C, stream)
    else:
        dy, x = zeros(n), zeros(n, "x")
        need = NACC * C * 4 * min(M, WGRAD_MAX_BLOCKS)             # an upper bound of the workspace (tiles <= pixels)
        ws = _buf(need // 4, device)
        outs = {"ws": ws}
        if "dw" not in no:
            outs["dw"] = _buf(49 * C, device)
        if "db" not in no:
            outs["db"] = _buf(C, device)
        nbytes = int(capi.lib.uenc_dwconv7_bwd_weight_workspace_bytes(B, H, W, C))
        nbytes = nbytes - 4 if what == "short_ws" else (nbytes or need)
        rc = capi.lib.uenc_dwconv7_bwd_weight(p(dy), p(x), p(outs.get("dw")), p(outs.get("db")), p(ws), nbytes, B, H, W, C, stream)
    return int(rc), outs


def ls_status_call(row, device, stream=0):
    from uenc import capi
    _, (N, K), what, _ = row
    no = _flags(what, "no")
    n = max(N, 1) * max(K, 1)
    z = lambda k: _buf(k, device).zero_()
    p = lambda t: 0 if t is None else t.data_ptr()
    dw2p, db2p, w2, b2, gamma = z(n), None if "db2p" in no else z(max(N, 1)), z(n), z(max(N, 1)), z(max(N, 1))
    outs = {k: _buf(n if k == "gw2" else max(N, 1), device) for k in ("gw2", "gb2", "ggamma") if k not in no}
    gw2 = dw2p if what == "alias:gw2=dw2p" else outs.get("gw2")
    rc = capi.lib.uenc_layer_scale_grads(p(dw2p), p(db2p), p(w2), p(b2), p(gamma), p(gw2), p(outs.get("gb2")), p(outs.get("ggamma")), N, K, stream)
    return int(rc), outs


def untouched(outs) -> bool:
    return all(bool((t == SENTINEL).all()) for t in outs.values())
