"""Shared by tests/test_attn_tiled_cases_cpu.py and tests/test_attn_tiled_kernels_gpu.py: the case table of the query-tiled attention
kernels of csrc/attn_tiled.hip (`attn_tiled_q_kernel<0|1, DROP>`, `attn_tiled_dkdv_kernel<DROP>`), and the defects its bars must see.

Inputs, the float64 reference `r64` with its absolute companions `A`, the emulation of the rounding points and the bar are those of
tests/mha_cases.py (the kernels keep the rounding points csrc/mha.hip documents: P to bf16 in front of P V, the bf16 out reused for delta,
dS to bf16 in front of both gradient products, bf16 dk / dv, fp32 dq); no case has a mask.  The bar is `mha_cases.bar` with
kappa = 2 RHO_EMU[output], RHO_EMU the emulation's largest rho over THIS table: the emulation sets the scale, never the kernel.
"""
import math

import torch

import mha_cases as MC

TQ, TK = 64, 64                     # queries per workgroup (forward, dQ), keys per LDS block / per dK-dV workgroup (csrc/attn_tiled.hip)
OUTPUTS, BF16_OUTPUTS = MC.OUTPUTS, MC.BF16_OUTPUTS
SCALE = MC.SCALE
DROP_SEED = 0x7A11ED

# Largest rho of the emulation over the whole table, rounded up to two decimals (measured: out 1.429 in q70-s33, dq 0.951 in drop-host,
# dk 0.969 in drop-slot, dv 1.546 in h8-b3); tests/test_attn_tiled_cases_cpu.py asserts it, and that it is no loose cap
RHO_EMU = {"out": 1.43, "dq": 0.96, "dk": 0.97, "dv": 1.55}
KAPPA = {k: 2.0 * v for k, v in RHO_EMU.items()}

# (id, B, H, Lq, S, dropout p, seed by "host" value | device "slot"): what each case reaches
_TABLE = [
    ("one", 1, 1, 1, 1, 0.0, "host"),               # a single query and key: out = v[0] bit for bit, three idle waves
    ("q63-s65", 2, 2, 63, 65, 0.0, "host"),         # one short of the query tile, one over the key block (a 1-key ragged block)
    ("q64-s64", 1, 3, 64, 64, 0.0, "host"),         # exactly one tile and one block; odd H
    ("q65-s63", 3, 1, 65, 63, 0.0, "host"),         # a second query tile of one row (three idle waves), one ragged key block; B = 3
    ("q129-s129", 1, 2, 129, 129, 0.0, "host"),     # two tiles plus one, both ways: the double buffer wraps, the third block holds one row
    ("q129-s64", 2, 1, 129, 64, 0.0, "host"),       # three query tiles against one block (dK / dV: three query blocks, one workgroup per head)
    ("q64-s129", 1, 1, 64, 129, 0.0, "host"),       # one query tile against three blocks (dK / dV: three workgroups, one query block)
    ("q1-s129", 1, 2, 1, 129, 0.0, "host"),         # a single query over three blocks
    ("q128-s1", 1, 2, 128, 1, 0.0, "host"),         # a single key: every row returns v[0] bit for bit
    ("q70-s33", 2, 3, 70, 33, 0.0, "host"),         # Lq != S, neither a multiple of 16
    ("res5-28", 2, 4, 28, 28, 0.0, "host"),         # the pixel-decoder fixture's res5 map (4 x 7 tokens), 4 heads
    ("h8-b3", 3, 8, 17, 40, 0.0, "host"),           # 8 heads, 3 images: 24 workgroups through xcd_remap, a second MFMA tile of one row
    ("q1000", 1, 2, 1000, 1000, 0.0, "host"),       # past the 960-query limit of uenc_mha_bwd: 16 tiles, the last 40 rows
    ("drop-host", 2, 2, 130, 70, 0.1, "host"),      # dropout 0.1, seed by value; ragged tile and block
    ("drop-slot", 1, 3, 65, 129, 0.1, "slot"),      # dropout 0.1, seed read from a device slot (the *_sp entries)
]
CASES = [dict(id=i, B=B, H=H, Lq=Lq, S=S, masked=False, p=p, seed_mode=sm, seed=4000 + n) for n, (i, B, H, Lq, S, p, sm) in enumerate(_TABLE)]
BY_ID = {c["id"]: c for c in CASES}

# defect -> the cases it is aimed at, and the outputs it reaches (lse where the defect moves it)
DEFECT_CASES = {
    "a_last_key_block_dropped": ["q63-s65", "q129-s129", "q64-s129"],
    "b_stale_tile_row": ["q64-s64", "q129-s129", "q1000"],
    "c_missing_inv_keep": ["drop-host", "drop-slot"],
}
DEFECT_REACH = {
    "a_last_key_block_dropped": ("out", "lse", "dq", "dk", "dv"), "b_stale_tile_row": ("out", "lse", "dq", "dk", "dv"),
    "c_missing_inv_keep": ("out", "dq", "dk", "dv"),
}


def inputs(case):
    return MC.inputs(case)


def weights(case):
    """keep / (1 - p) (B, H, Lq, S) float64 of a dropout case (the kernels' hash, restated by uenc.attention.keep_mask_reference), or None."""
    if case["p"] == 0.0:
        return None
    from uenc.attention import keep_mask_reference
    return keep_mask_reference(case["B"], case["H"], case["Lq"], case["S"], case["p"], DROP_SEED).double() / (1.0 - case["p"])


def bar(name, r64, A):
    return MC.bar(name, r64, A, KAPPA[name])


def defective(defect, t, case):
    """The float64 result with one defect applied, in `mha_cases.reference`'s layout (out, lse, dq, dk, dv)."""
    H, S, Lq = case["H"], case["S"], case["Lq"]
    if defect == "c_missing_inv_keep":                  # the keep-mask applied, its 1 / (1 - p) forgotten in all three kernels
        assert case["p"] > 0
        r, _ = MC.reference(t, case, weights(case) * (1.0 - case["p"]))
        return r
    assert case["p"] == 0.0
    s = MC.scores(t, H).clone()
    if defect == "a_last_key_block_dropped":            # the key loop ends one block early
        assert S > TK
        s[..., (-(-S // TK) - 1) * TK:] = -math.inf
    elif defect == "b_stale_tile_row":                  # the last row of the first query tile keeps the row before it
        assert Lq >= TQ
        s[..., TQ - 1, :] = s[..., TQ - 2, :]
    else:
        raise KeyError(defect)
    P, lse = MC.softmax_lse(s)
    out = P @ MC._heads(t["v"], H)
    r, _ = MC.backward(s, lse, out, t, H)
    r.update(out=MC._rows(out), lse=lse)
    return r
