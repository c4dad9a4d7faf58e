"""Shared by tests/test_na2d_cases_cpu.py and tests/test_na2d_kernels_gpu.py: the case table of the neighbourhood-attention kernels of
csrc/na2d_mfma.hip (`na2d_mfma_fwd_kernel<K>`, `na2d_mfma_bwd_q_kernel<K>`, `na2d_mfma_bwd_kv_kernel<K>`, K = 3, 5, 7), of csrc/na2d.hip
(`na2d_fwd_tiled_kernel<K>`, `na2d_bwd_q_tiled_kernel<K>`, `na2d_bwd_kv_kernel<K>`, K = 9, 11, 13) and of their fp32 twins in
csrc/exact.hip (`xna_fwd_kernel`, `xna_bwd_kernel`), their inputs, references, bars, the planner restated, and the defects the bars must see.

Nothing here imports `uenc`.  Inputs come from a seeded CPU generator; qkv and dO are rounded to bf16 once, so a reference sees exactly
the values the kernels see.  q and k have standard deviation 2 (a peaked softmax: one wrong key moves a row), v and dO standard
deviation 1; rpb is fp32 with standard deviation 1 (or None); head_dim is 32 and scale 32^-0.5.

Shapes: out (B, H, W, nH, 32), lse (B, nH, H, W) in natural-log units, dqkv (B, H, W, 3, nH, 32), drpb (nH, 2K-1, 2K-1): the kernels'
own buffers viewed without a copy.  With `heads` given, a function returns only those heads, in the same order of axes.

  r64   `reference`: neighbourhood attention in float64 on the data itself.  Per axis and pixel the window start and the bias start are
        NATTEN 0.14.4's `get_window_start` / `get_pb_start`, restated literally below (scalar, branch by branch; tests/test_dinat_cpu.py
        imports them from here) -- not the kernels' clamp(p - K/2, 0, L - K).  The K x K neighbours are gathered at stride d, scores are
        scale q.k + rpb[...], softmax, @ v; dq, dk, dv, drpb by float64 autograd, so the kernels' inverse-neighbourhood ranges never
        enter it.  NATTEN itself is absent: r64 is a second, independent statement of its published definition, not its output.
  A     `neigh(...)[1]`: per output the same contraction over absolute values, the scale the bf16 rounding points act on:
        A_out = P |v|, A_dv = P^T |dO|, dS_abs = |dS| + P sum_d |o_d dO_d|, A_dq = scale dS_abs |k|, A_dk = scale dS_abs^T |q|,
        A_drpb = the sum of dS_abs over all (query, key) pairs of a bias bin.
  emu   `emulate`: float64 with the rounding points of the kernels, read from the code, and nothing else of them.
        MFMA route (K <= 7).  Forward: the unnormalised exp2(s - m) rounded to bf16 in front of the P V product, the unrounded normaliser
        applied behind it, out rounded to bf16.  Per-query backward: delta from the bf16 saved out times dO; P = exp2(s - lse);
        dS = P (dP - delta) unrounded for drpb, rounded to bf16 in front of the dQ product; dq rounded to bf16 behind the scale.
        Per-key backward: P rounded to bf16 for dV, bf16(P (dP - delta)) feeds dK; dk, dv rounded to bf16.
        VALU route (K >= 9): no intermediate rounding; only delta from the bf16 out and the bf16 rounding of out, dq, dk, dv.
  emu32 `reference(..., dtype=torch.float32)`: the r64 code evaluated in float32, the yardstick of the fp32 twins.

Bars, every element, nothing excused.  out, dqkv (bf16): |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + floor, floor = 8 2^-24 max |r64| +
2^-126.  drpb (fp32, ACCUMULATED into a non-zero prefill by float atomics): |kernel - (prefill + r64)| <= kappa 2^-9 A + floor +
n 2^-24 (|prefill| + A), n = `drpb_adds`: the workgroups that add into one head's bins (MFMA: chunks d^2 B; VALU: tiles d^2 B, from the
restated planner).  lse: max(4 e_ref, 8 2^-24 max |r64|), e_ref the error of emu32's own lse.  fp32 twins: |kernel - r64| <= gamma 2^-24 A
+ floor.  kappa = 2 RHO_EMU[route][output], RHO_EMU the largest rho = (|emu - r64| - 2^-8 |r64|)^+ / (2^-9 A) over the whole table,
measured on the CPU from the emulation, never from a kernel; the factor 2 is for what the kernels do and the emulation does not -- fp32
summation order, the 1-ulp hardware exp2, the diagonal partial sums and atomics of drpb, the fp32 lse the backward reads -- each of
which changes which way a bf16 rounding falls, not its size.  gamma = 8 RHO32[output]: the twins add a window's up to 169 scores and 32
channels strictly one after the other (online softmax in the forward, fmaf chains and one float atomic per (query, key) pair for
dk / dv in the backward) where torch sums in blocks of 8 or more lanes -- random-walk growth of about sqrt(169 / 8) ~ 4.6 at K = 13 and
<= 3.9 at K <= 11 -- times the usual 2: the factor 8 of tests/wattn_cases.py, kept.  (The twins' drpb adds 64 queries per workgroup one
after the other into LDS and then one float atomic per workgroup and bin; the GPU test starts it from zero, as the window-attention
pin does for its table gradient.)

Out of scope: the K <= 7 instantiations of the VALU kernels.  They are reached only when H W 3C >= 2^31, one operand of 4 GiB or more:
no few-second test with a float64 reference can run them, and no switch is added to force the route.

DEFECTS are applied to the emulation; the bars must see each in the cases DEFECT_CASES aims it at.  One is documented as WITHIN the bar,
and nothing is tuned to catch it:
  j_delta_from_unrounded_out   delta = dO . o with o before its bf16 rounding: o moves by at most 2^-9 |o| per channel, so every dS
                               moves by at most 2^-9 P sum_d |o_d dO_d| -- the second term of dS_abs, which kappa 2^-9 A allows by
                               construction in dq, dk and drpb.
"""
import numpy as np
import torch

LOG2E = 1.4426950408889634
SCALE = 32 ** -0.5
U8, U9, U24 = 2.0 ** -8, 2.0 ** -9, 2.0 ** -24
TINY = 2.0 ** -126                   # the smallest normal fp32 number
MAX_SCORES = 32 * 1024 * 1024         # B nH H W K^2 of any case: keeps every GPU test at a few seconds
MAX_QKV = 50 * 1000 * 1000            # elements of qkv
TH, TW = 8, 16                        # NM_TH x NM_TW = NA_TH x NA_TW: the tile of both kernel families, in class positions
OUTPUTS = ("out", "dqkv", "drpb")
BF16_OUTPUTS = ("out", "dqkv")

# Largest rho of the emulation over the whole table, per route, rounded up to two decimals; tests/test_na2d_cases_cpu.py asserts it, and
# that it is no loose cap.  MFMA (measured: out 1.594 and dqkv 1.858 in nt8, drpb 0.784 in min7).  VALU (measured: dqkv 0.866 in
# valu13-halo, drpb 0.529 in valu11): the emulation rounds nothing in front of a product, so out answers to its own bf16 rounding alone
# (rho 0 in every case: that bar is 2^-8 |r64| + floor) and dqkv / drpb to delta from the bf16 out.
RHO_EMU = {"mfma": {"out": 1.60, "dqkv": 1.86, "drpb": 0.79}, "valu": {"out": 0.0, "dqkv": 0.87, "drpb": 0.53}}
KAPPA = {r: {k: 2.0 * v for k, v in t.items()} for r, t in RHO_EMU.items()}
# The same for emu32 in units of 2^-24 A (measured: out 41.50 and dqkv 31.87 in kvmax7, drpb 9.53 in valu11, the same with 2 and with 8
# threads).  An fp32 sum depends on the order the BLAS build adds in, which a float64 emulation is blind to: the figures sit about 4 %
# above the measurement, in the middle of the window tests/test_na2d_cases_cpu.py allows (rho32 <= RHO32 <= 1.1 rho32)
RHO32 = {"out": 43.2, "dqkv": 33.2, "drpb": 9.9}
GAMMA = {k: 8.0 * v for k, v in RHO32.items()}


# ---- NATTEN 0.14.4's neighbourhood, restated literally ------------------------------------------------------------------------------------
def natten_window_start(index, length, K, NS, d):
    """NATTEN 0.14.4 get_window_start, restated literally (scalar)."""
    if d <= 1:
        return max(index - NS, 0) + (index + NS >= length) * (length - index - NS - 1)
    ni = index - NS * d
    if ni < 0:
        return index % d
    if index + NS * d >= length:
        imodd = index % d
        a = (length // d) * d
        b = length - a
        if imodd < b:
            return length - b + imodd - 2 * NS * d
        return a + imodd - K * d
    return ni


def natten_pb_start(index, length, K, NS, d):
    """NATTEN 0.14.4 get_pb_start, restated literally (scalar)."""
    if d <= 1:
        return NS + (index < NS) * (NS - index) + (index + NS >= length) * (length - index - 1 - NS)
    if index - NS * d < 0:
        return K - 1 - (index // d)
    if index + NS * d >= length:
        return (length - index - 1) // d
    return NS


def natten_axis(length, K, d):
    """(nb, pb), both (length, K): the neighbour indices and the bias indices of every index of an axis, from the two functions above."""
    ws = torch.tensor([natten_window_start(i, length, K, K // 2, d) for i in range(length)])
    ps = torch.tensor([natten_pb_start(i, length, K, K // 2, d) for i in range(length)])
    j = torch.arange(K)
    return ws[:, None] + j[None] * d, ps[:, None] + j[None]


def closed_axis(length, K, d, defect=None):
    """The same from the kernels' closed form -- start = clamp(p - K/2, 0, L_r - K) in class positions, bias = start + j - p + K - 1 -- with
    the per-axis defects applied.  A neighbour outside the axis is `length` (read as a zero row)."""
    NS = K // 2
    i = torch.arange(length)
    r, p = i % d, i // d
    L = (length - r + d - 1) // d
    Lc = torch.full_like(L, length // d) if defect == "e_class_length_floor" else L
    hi = (Lc - K - 1).clamp_min(0) if defect == "a_far_clamp_off_by_one" else Lc - K
    start = (p - NS).clamp_min(0)
    if defect != "b_far_border_unclamped":
        start = torch.minimum(start, hi)
    pb0 = torch.full_like(p, NS) if defect == "c_bias_ignores_clamp" else start - p + K - 1
    j = torch.arange(K)
    pos = start[:, None] + j[None]
    nb = torch.where(pos < L[:, None], pos * d + r[:, None], torch.full_like(pos, length))
    return nb, pb0[:, None] + j[None]


# ---- the planner, restated from csrc/na2d_mfma.hip and csrc/na2d.hip ------------------------------------------------------------------------
def dims(case):
    return tuple(case[n] for n in ("B", "H", "W", "nH", "K", "d"))


def mfma_supported(H, W, nH, K):
    """na2d_mfma_supported."""
    return K <= 7 and H * W * 3 * nH * 32 < 2 ** 31


def route(case):
    return "mfma" if mfma_supported(case["H"], case["W"], case["nH"], case["K"]) else "valu"


def plan(B, H, W, nH, d):
    """nm_plan: tiles per residue class, tiles per workgroup (nt), workgroups per class (chunks)."""
    Lx, Ly = -(-W // d), -(-H // d)                                                  # the longest residue class
    tiles_x, tiles_y = -(-Lx // TW), -(-Ly // TH)
    per_class = tiles_x * tiles_y
    total = per_class * d * d * B * nH
    nt = min(max(total // 1536, 1), 8, per_class)
    return dict(tiles_x=tiles_x, tiles_y=tiles_y, per_class=per_class, nt=nt, chunks=-(-per_class // nt))


def tiles_per_group(B, H, W, nH, K, d):
    """What uenc_na2d_tiles_per_group reports: nt on the MFMA route, 0 where the VALU kernels run."""
    return plan(B, H, W, nH, d)["nt"] if mfma_supported(H, W, nH, K) else 0


def class_lengths(length, d):
    return [(length - r + d - 1) // d for r in range(d)]


def _inv_start(pos, K):
    return 0 if pos < K else pos - K // 2


def _inv_end(pos, L, K):
    return L if pos >= L - K else pos + K // 2 + 1


def axis_extent(length, d, K, T):
    """nm_axis_extent: the longest inverse-neighbourhood halo of a tile over all residue classes of an axis."""
    best = 0
    for L in class_lengths(length, d)[:length]:
        for p0 in range(0, L, T):
            pl = min(p0 + T, L) - 1
            best = max(best, _inv_end(pl, L, K) - _inv_start(p0, K))
    return best


def _clamp(v, lo, hi):
    return min(max(v, lo), hi)


def tile_q(t, tiles_x, Ly, Lx, K):
    """nm_tile_q: origin, validity and halo of tile t of a class of Ly x Lx positions."""
    NS = K // 2
    py0, px0 = (t // tiles_x) * TH, (t % tiles_x) * TW
    hsy, hsx = _clamp(py0 - NS, 0, Ly - K), _clamp(px0 - NS, 0, Lx - K)
    return dict(py0=py0, px0=px0, ok=py0 < Ly and px0 < Lx, hsy=hsy, hsx=hsx,
                hh=_clamp(min(py0 + TH, Ly) - 1 - NS, 0, Ly - K) + K - hsy, hw=_clamp(min(px0 + TW, Lx) - 1 - NS, 0, Lx - K) + K - hsx)


def walks(case):
    """The tiles each workgroup of a class walks, in order: [[0, 1], [2]]."""
    B, H, W, nH, K, d = dims(case)
    p = plan(B, H, W, nH, d)
    return [list(range(t0, min(t0 + p["nt"], p["per_class"]))) for t0 in range(0, p["per_class"], p["nt"])]


def drpb_adds(case):
    """Workgroups that add into one head's bins with one float atomic each: chunks d^2 B (MFMA), tiles d^2 B (VALU)."""
    B, H, W, nH, K, d = dims(case)
    p = plan(B, H, W, nH, d)
    return (p["chunks"] if route(case) == "mfma" else p["per_class"]) * d * d * B


def reach(case):
    """What the case makes the kernels do, from the restated planner."""
    B, H, W, nH, K, d = dims(case)
    p = plan(B, H, W, nH, d)
    r = dict(route=route(case), class_len_y=class_lengths(H, d), class_len_x=class_lengths(W, d), tiles_x=p["tiles_x"], tiles_y=p["tiles_y"])
    if r["route"] == "valu":
        r.update(nt=0, walks=[], crosses_row=False, notok_walks=[], notok_prefetched=False, hh_max=0, hw_max=0, ncb=0,
                 grid=(p["tiles_x"] * d, p["tiles_y"] * d, B * nH), halo=(min(TH + K - 1, max(r["class_len_y"])), min(TW + K - 1, max(r["class_len_x"]))))
        return r
    ws = walks(case)
    notok, prefetched, ncb = set(), False, 0
    for Ly in r["class_len_y"]:
        for Lx in r["class_len_x"]:
            for w in ws:
                oks = [tile_q(t, p["tiles_x"], Ly, Lx, K)["ok"] for t in w]
                if not all(oks):
                    notok.add(tuple(w))
                    prefetched = prefetched or not all(oks[1:])
            for t in range(p["per_class"]):
                g = tile_q(t, p["tiles_x"], Ly, Lx, K)
                for wx in (0, 1):                                                    # the per-key kernel's query span per wave, in x
                    if g["ok"] and g["px0"] + 8 * wx < Lx:
                        kx_a, kx_b = min(g["px0"] + 8 * wx, Lx - 1), min(g["px0"] + 8 * wx + 7, Lx - 1)
                        ncb = max(ncb, (_inv_end(kx_b, Lx, K) - _inv_start(kx_a, K) + 15) >> 4)
    r.update(nt=p["nt"], walks=ws, crosses_row=any(len({t // p["tiles_x"] for t in w}) > 1 for w in ws), notok_walks=sorted(list(w) for w in notok),
             notok_prefetched=prefetched, hh_max=axis_extent(H, d, K, TH), hw_max=axis_extent(W, d, K, TW), ncb=ncb,
             grid=(p["chunks"], d * d, B * nH))
    return r


def fdiv(a, b):
    """`(int)(((float)a + 0.5f) * inv_b)`, inv_b = 1.0f / (float)b, in numpy float32 (a: array or int)."""
    inv = np.float32(1.0) / np.float32(b)
    return ((np.asarray(a).astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


# (id, K, d, B, H, W, nH, rpb): what each case reaches
_TABLE = [
    ("min3", 3, 1, 1, 3, 3, 1, True),             # L = K on both axes: all nine queries share one window
    ("min7", 7, 1, 1, 7, 7, 1, True),             # the same at K = 7; one wave active, mostly padded key blocks
    ("min5-d3", 5, 3, 1, 15, 17, 2, True),        # L = K and K + 1 under dilation; ragged classes
    ("short7", 7, 1, 1, 13, 14, 2, True),         # L = 2K - 1 and 2K: both clamps meet in every window
    ("ragged5", 5, 2, 1, 21, 45, 3, True),        # L = 2K and 2K + 1; Lx = 22 / 23; odd head count
    ("kvmax7", 7, 1, 2, 22, 38, 2, True),         # hh_max = 17, hw_max = 25: the largest the per-key LDS image gets; B = 2
    ("ncb2", 7, 1, 1, 9, 22, 1, True),            # per-key query span of 17 (ncb == 2); second tile row with one position
    ("notok3", 3, 4, 1, 16, 130, 1, True),        # Lx = 33 / 33 / 32 / 32: a whole workgroup on a !ok tile
    ("tail65", 3, 1, 1, 8, 65, 1, True),          # a one-column last tile
    ("nt2-tail", 3, 4, 2, 12, 129, 32, True),     # 3072 tiles: nt = 2, chunks [0, 1] and [2]; the clipped last chunk is !ok in three classes of four
    ("nt3-notok", 3, 4, 2, 12, 129, 48, True),    # 4608 tiles: nt = 3, walk [0, 1, 2] with tile 2 !ok as the prefetched tile in classes rx >= 1
    ("nt2-rows", 7, 4, 2, 36, 129, 16, True),     # 3072 tiles, 3 x 2 per class: walk [2, 3] crosses a tile row; drpb carry flushed (wx = 0) and kept (wx = 1)
    ("nt8", 3, 4, 2, 12, 452, 48, True),          # 12288 tiles: nt hits its cap of 8 in one walk of 8
    ("valu9", 9, 2, 1, 19, 37, 1, True),          # VALU route; classes of 9 / 10 x 18 / 19
    ("valu11", 11, 1, 1, 12, 50, 2, True),        # two tile rows, a W tail in the per-key kernel (50 < 64)
    ("valu13-halo", 13, 1, 1, 24, 40, 1, True),   # the full 20 x 28 halo of the <13> tiled kernels; border and interior waves for both drpb paths
    ("valu13-w", 13, 1, 2, 13, 130, 2, True),     # L = K in y; three 64-pixel blocks per row in the per-key kernel, the last a tail
    ("no-rpb", 7, 2, 1, 16, 33, 2, False),        # NULL bias on the MFMA route's tables
    ("no-rpb9", 9, 2, 1, 19, 37, 2, False),       # its K = 9 twin: NULL bias on the VALU route
]
CASES = [dict(id=i, K=K, d=d, B=B, H=H, W=W, nH=nH, rpb=rpb, seed=3000 + n) for n, (i, K, d, B, H, W, nH, rpb) in enumerate(_TABLE)]
BY_ID = {c["id"]: c for c in CASES}
NT_CASES = ("nt2-tail", "nt3-notok", "nt2-rows", "nt8")
# the fp32 twins have no tile walk: every case up to tail65, the VALU-route cases and the NULL bias
F32_CASES = [c for c in CASES if c["id"] not in NT_CASES]
# the cases whose emulation the CPU test evaluates on three heads (first, last, one in between); the GPU test checks every head
EMU_HEADS = {i: (0, BY_ID[i]["nH"] // 2, BY_ID[i]["nH"] - 1) for i in NT_CASES}

# defect -> the cases it is aimed at (tests/test_na2d_cases_cpu.py)
DEFECT_CASES = {
    "a_far_clamp_off_by_one": ["short7", "ragged5", "valu11", "nt2-rows"],
    "b_far_border_unclamped": ["kvmax7", "ragged5", "valu9"],
    "c_bias_ignores_clamp": ["min3", "short7", "valu13-halo", "nt2-rows"],
    "d_bias_transposed": ["min5-d3", "kvmax7", "valu11"],
    "e_class_length_floor": ["min5-d3", "ragged5", "valu9"],
    "f_inverse_band_off_by_one": ["short7", "kvmax7", "valu13-halo"],
    "g_stale_halo": ["nt2-tail", "nt3-notok", "nt2-rows", "nt8"],
    "h_missing_drpb_flush": ["nt2-tail", "nt2-rows", "nt8"],
    "i_lse_in_log2_units": ["min7", "valu9"],
    "j_delta_from_unrounded_out": ["kvmax7", "nt2-rows", "valu13-halo"],
}
_ALL = ("out", "lse", "dqkv", "drpb")
# the outputs a defect must move beyond the bar; () = documented as within the bar (module docstring)
DEFECT_REACH = {
    "a_far_clamp_off_by_one": _ALL, "b_far_border_unclamped": _ALL, "c_bias_ignores_clamp": _ALL, "d_bias_transposed": _ALL,
    "e_class_length_floor": _ALL, "f_inverse_band_off_by_one": ("dk", "dv"), "g_stale_halo": _ALL, "h_missing_drpb_flush": ("drpb",),
    "i_lse_in_log2_units": ("lse",), "j_delta_from_unrounded_out": (),
}
# the outputs a defect must leave bit for bit as they were
DEFECT_UNTOUCHED = {"f_inverse_band_off_by_one": ("out", "lse", "dq", "drpb"), "h_missing_drpb_flush": ("out", "lse", "dqkv"),
                    "i_lse_in_log2_units": ("out", "dqkv", "drpb"), "j_delta_from_unrounded_out": ("out", "lse", "dv")}


def part(r, name):
    """An output by name, "dq" / "dk" / "dv" being the three slices of dqkv."""
    return r["dqkv"][:, :, :, "qkv".index(name[1])] if name in ("dq", "dk", "dv") else r[name]


def n_scores(case):
    B, H, W, nH, K, d = dims(case)
    return B * nH * H * W * K * K


def inputs(case):
    """qkv (B, H, W, 3, nH, 32) and dout (B, H, W, nH, 32) bf16, rpb (nH, 2K-1, 2K-1) fp32 or None, on the CPU."""
    B, H, W, nH, K, d = dims(case)
    g = torch.Generator(device="cpu").manual_seed(case["seed"])
    qkv = torch.randn(B, H, W, 3, nH, 32, generator=g)
    qkv[:, :, :, :2] *= 2.0
    dout = torch.randn(B, H, W, nH, 32, generator=g)
    rpb = torch.randn(nH, 2 * K - 1, 2 * K - 1, generator=g)
    return dict(qkv=qkv.bfloat16(), dout=dout.bfloat16(), rpb=rpb if case["rpb"] else None)


def select(r, heads):
    """The heads `heads` of every output of r (shapes of the module docstring)."""
    h = list(heads)
    return dict(out=r["out"][:, :, :, h], lse=r["lse"][:, h], dqkv=r["dqkv"][:, :, :, :, h], drpb=r["drpb"][h])


# ---- r64 --------------------------------------------------------------------------------------------------------------------------------
def reference(t, case, dtype=torch.float64, heads=None, grads=True):
    """r64 (or, with dtype = float32, emu32): the attention on the data itself and autograd for the gradients, in chunks over heads; runs
    where the inputs live.  grads = False: out and lse only."""
    B, H, W, nH, K, d = dims(case)
    dev = t["qkv"].device
    heads = list(range(nH)) if heads is None else list(heads)
    (ny, py), (nx, px) = (tuple(a.to(dev) for a in natten_axis(n, K, d)) for n in (H, W))
    out, lse, dqkv, drpb = [], [], [], []
    hc = max(1, (24 << 20) // (B * H * W * K * K * 32))
    for c0 in range(0, len(heads), hc):
        hs = heads[c0:c0 + hc]
        x = t["qkv"][:, :, :, :, hs].to(dtype).permute(3, 0, 4, 1, 2, 5).contiguous().requires_grad_(True)           # (3, B, h, H, W, 32)
        # without a bias the kernels still sum dS into the bins they are given: the gradient with respect to an all-zero rpb
        r = torch.zeros(len(hs), 2 * K - 1, 2 * K - 1, dtype=dtype, device=dev) if t["rpb"] is None else t["rpb"][hs].to(dtype).clone()
        r.requires_grad_(True)
        kk = x[1][:, :, ny][:, :, :, :, nx]                                                                      # (B, h, H, K, W, K, 32)
        vv = x[2][:, :, ny][:, :, :, :, nx]
        s = SCALE * torch.einsum("bhyxc,bhyixjc->bhyxij", x[0], kk)
        s = s + r[:, py][:, :, :, px].permute(0, 1, 3, 2, 4)                                                     # (h, H, K, W, K) -> (h, H, W, K, K)
        s = s.reshape(B, len(hs), H, W, K * K)
        o = torch.einsum("bhyxij,bhyixjc->bhyxc", s.softmax(-1).view(B, len(hs), H, W, K, K), vv)
        out.append(o.detach().permute(0, 2, 3, 1, 4))
        lse.append(torch.logsumexp(s.detach(), -1))
        if grads:
            g = torch.autograd.grad(o, [x, r], t["dout"][:, :, :, hs].to(dtype).permute(0, 3, 1, 2, 4))
            dqkv.append(g[0].permute(1, 3, 4, 0, 2, 5))
            drpb.append(g[1])
    if not grads:
        return dict(out=torch.cat(out, 3), lse=torch.cat(lse, 1))
    return dict(out=torch.cat(out, 3), lse=torch.cat(lse, 1), dqkv=torch.cat(dqkv, 4), drpb=torch.cat(drpb, 0))


# ---- per-pixel index maps: the neighbourhood, the defects that move it, the tile walk ----------------------------------------------------
def _class_tiles(case):
    """Every (ry, rx, Ly, Lx) of the case, with the planner."""
    B, H, W, nH, K, d = dims(case)
    p = plan(B, H, W, nH, d)
    return p, [(ry, rx, (H - ry + d - 1) // d, (W - rx + d - 1) // d) for ry in range(min(d, H)) for rx in range(min(d, W))]


def geometry(case, defect=None):
    """key (H W, K K): the pixel every (query, window slot) reads k and v from, H W for a zero row; bias (H W, K K): the flat rpb entry its
    score adds, (2K-1)^2 for none; gbin (H W, K K): the flat drpb bin its dS lands in, (2K-1)^2 for dropped.  Sound maps come from
    NATTEN's formulas; a defect replaces what it names."""
    B, H, W, nH, K, d = dims(case)
    RB, NS, HW = 2 * K - 1, K // 2, H * W
    axis_defect = defect if defect in ("a_far_clamp_off_by_one", "b_far_border_unclamped", "c_bias_ignores_clamp", "e_class_length_floor") else None
    if axis_defect is None:
        (ny, py), (nx, px) = natten_axis(H, K, d), natten_axis(W, K, d)
    else:
        (ny, py), (nx, px) = closed_axis(H, K, d, axis_defect), closed_axis(W, K, d, axis_defect)
    key = ny[:, None, :, None] * W + nx[None, :, None, :]
    key = torch.where((ny[:, None, :, None] < H) & (nx[None, :, None, :] < W), key, torch.full_like(key, HW))       # (H, W, K, K)
    if defect == "d_bias_transposed":
        bias = px[None, :, None, :] * RB + py[:, None, :, None]
    else:
        bias = py[:, None, :, None] * RB + px[None, :, None, :]
    inside = ((py >= 0) & (py < RB))[:, None, :, None] & ((px >= 0) & (px < RB))[None, :, None, :]      # a defect may leave the table: no bias, no bin
    bias = torch.where(inside, bias, torch.full_like(bias, RB * RB)).expand(H, W, K, K).clone()
    gbin = bias.clone()
    if defect == "g_stale_halo":
        # in a walk, tile t + 1 computes on the LDS images of tile t's halo: the same image offsets, the previous tile's pixels
        assert route(case) == "mfma"
        p, classes = _class_tiles(case)
        for ry, rx, Ly, Lx in classes:
            for t in range(p["per_class"]):
                g = tile_q(t, p["tiles_x"], Ly, Lx, K)
                if t % p["nt"] == 0 or not g["ok"]:
                    continue
                gp = tile_q(t - 1, p["tiles_x"], Ly, Lx, K)
                pys, pxs = torch.arange(g["py0"], min(g["py0"] + TH, Ly)), torch.arange(g["px0"], min(g["px0"] + TW, Lx))
                j = torch.arange(K)
                rel_y = (pys - NS).clamp(0, Ly - K)[:, None] - g["hsy"] + j[None]                               # image rows of the window
                rel_x = (pxs - NS).clamp(0, Lx - K)[:, None] - g["hsx"] + j[None]
                oky, okx = (rel_y < gp["hh"]) & gp["ok"], (rel_x < gp["hw"]) & gp["ok"]
                src = ((gp["hsy"] + rel_y) * d + ry)[:, None, :, None] * W + ((gp["hsx"] + rel_x) * d + rx)[None, :, None, :]
                src = torch.where(oky[:, None, :, None] & okx[None, :, None, :], src, torch.full_like(src, HW))
                key[(pys * d + ry)[:, None], (pxs * d + rx)[None, :]] = src
    if defect == "h_missing_drpb_flush":
        # a wave's diagonal sums of a walk all go out with the (by_first, bcol0) of its last active tile
        assert route(case) == "mfma"
        p, classes = _class_tiles(case)
        first = lambda pa, L: _clamp(pa - NS, 0, L - K) - pa + K - 1
        for ry, rx, Ly, Lx in classes:
            for w in walks(case):
                for wy in range(4):
                    for wx in range(2):
                        act = [g for g in (tile_q(t, p["tiles_x"], Ly, Lx, K) for t in w) if g["ok"] and g["py0"] + 2 * wy < Ly and g["px0"] + 8 * wx < Lx]
                        if not act:
                            continue
                        by_l, bc_l = first(act[-1]["py0"] + 2 * wy, Ly), first(act[-1]["px0"] + 8 * wx, Lx)
                        for g in act[:-1]:
                            dy, dx = by_l - first(g["py0"] + 2 * wy, Ly), bc_l - first(g["px0"] + 8 * wx, Lx)
                            pys = torch.arange(g["py0"] + 2 * wy, min(g["py0"] + 2 * wy + 2, Ly))
                            pxs = torch.arange(g["px0"] + 8 * wx, min(g["px0"] + 8 * wx + 8, Lx))
                            Y, X = (pys * d + ry)[:, None], (pxs * d + rx)[None, :]
                            row, col = py[Y][:, :, :, None] + dy, px[X][:, :, None, :] + dx
                            moved = torch.where((row >= 0) & (row < RB) & (col >= 0) & (col < RB), row * RB + col, torch.full_like(row * RB + col, RB * RB))
                            gbin[Y, X] = moved
    return key.reshape(HW, K * K), bias.reshape(HW, K * K), gbin.reshape(HW, K * K)


def _extra_pairs(case):
    """Defect f: the (query pixel, key pixel, flat bias entry or (2K-1)^2) pairs a per-key kernel adds when its inverse neighbourhood
    starts at 0 for pos <= K instead of pos < K.  Per axis the key at class position K gains the queries 0 .. K/2; in two dimensions the
    pairs are (extra in y) x (sound or extra in x) and (sound in y) x (extra in x).  Their bias index lies outside the table: 0."""
    B, H, W, nH, K, d = dims(case)
    RB, NS = 2 * K - 1, K // 2

    def axis(length):
        nb, pb = natten_axis(length, K, d)
        sound = [(q, int(nb[q, i]), int(pb[q, i])) for q in range(length) for i in range(K)]
        extra = []
        for r, L in enumerate(class_lengths(length, d)[:length]):
            if L > K:
                extra += [(qp * d + r, K * d + r, RB) for qp in range(_inv_start(K, K))]         # the sound start of pos == K: K - K/2
        return sound, extra

    (sy, ey), (sx, ex) = axis(H), axis(W)
    pairs = [(a, b) for a in ey for b in sx + ex] + [(a, b) for a in sy for b in ex]
    if not pairs:
        return None
    qp = torch.tensor([a[0] * W + b[0] for a, b in pairs])
    kp = torch.tensor([a[1] * W + b[1] for a, b in pairs])
    bn = torch.tensor([a[2] * RB + b[2] if a[2] < RB and b[2] < RB else RB * RB for a, b in pairs])
    return qp, kp, bn


def _bf(a):
    return a.float().bfloat16().double()


def neigh(t, case, rounded=False, defect=None, heads=None):
    """(result, A).  rounded = False, defect = None: r64's closed forms over explicit (query, slot) maps (tests/test_na2d_cases_cpu.py
    holds them against `reference`) and the absolute contractions A.  rounded = True: the emulation of the case's route, with `defect`
    applied if given; A is None."""
    B, H, W, nH, K, d = dims(case)
    HW, KK, RB2 = H * W, K * K, (2 * K - 1) ** 2
    dev = t["qkv"].device
    heads = list(range(nH)) if heads is None else list(heads)
    nh = len(heads)
    key, bias, gbin = (a.to(dev) for a in geometry(case, defect))
    mfma = rounded and route(case) == "mfma"
    bf = _bf if rounded else (lambda a: a)
    bfm = _bf if mfma else (lambda a: a)
    want_A = not rounded and defect is None
    extra = _extra_pairs(case) if defect == "f_inverse_band_off_by_one" else None
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    R = dict(out=z(B, HW, nh, 32), lse=z(B, nh, HW), dqkv=z(B, HW, 3, nh, 32), drpb=z(nh, RB2))
    A = dict(out=z(B, HW, nh, 32), dqkv=z(B, HW, 3, nh, 32), drpb=z(nh, RB2)) if want_A else None
    qkv, dout = t["qkv"].view(B, HW, 3, nH, 32), t["dout"].view(B, HW, nH, 32)
    hc = max(1, (4 << 20) // (B * HW * KK))
    for c0 in range(0, nh, hc):
        hs = heads[c0:c0 + hc]
        n, sl = len(hs), slice(c0, c0 + len(hs))
        x = qkv[:, :, :, hs].double().permute(2, 0, 3, 1, 4)                         # (3, B, n, HW, 32)
        q, kz, vz = x[0], torch.cat([x[1], z(B, n, 1, 32)], 2), torch.cat([x[2], z(B, n, 1, 32)], 2)
        do = dout[:, :, hs].double().permute(0, 2, 1, 3)                             # (B, n, HW, 32)
        rz = z(n, RB2 + 1)
        if t["rpb"] is not None:
            rz[:, :RB2] = t["rpb"][hs].double().reshape(n, RB2)
        S = torch.empty(B, n, HW, KK, dtype=torch.float64, device=dev)
        for s in range(KK):
            S[..., s] = SCALE * (q * kz[:, :, key[:, s]]).sum(-1) + rz[:, bias[:, s]][None]
        m = S.amax(-1, keepdim=True)
        e = (S - m).exp()
        l = e.sum(-1, keepdim=True)                                                  # the normaliser: unrounded
        lse = (m + l.log()).squeeze(-1)
        P = e / l
        ev = bfm(e)                                                                  # MFMA forward: bf16 in front of the P V product
        acc, dP = z(B, n, HW, 32), torch.empty_like(S)
        for s in range(KK):
            vs = vz[:, :, key[:, s]]
            acc += ev[..., s:s + 1] * vs
            dP[..., s] = (do * vs).sum(-1)
            if want_A:
                A["out"][:, :, sl] += (P[..., s:s + 1] * vs.abs()).permute(0, 2, 1, 3)
        o = bf(acc / l)                                                              # the saved out
        od = (acc / l if defect == "j_delta_from_unrounded_out" else o) * do
        delta = od.sum(-1, keepdim=True)
        dS = P * (dP - delta)                                                        # unrounded for drpb
        dS16, P16 = bfm(dS), bfm(P)                                                  # MFMA: bf16 in front of the dQ, dK and dV products
        dS_abs = dS.abs() + P * od.abs().sum(-1, keepdim=True) if want_A else None
        dq, dk, dv = z(B, n, HW, 32), z(B, n, HW + 1, 32), z(B, n, HW + 1, 32)
        Aq, Ak, Av = (z(B, n, HW, 32), z(B, n, HW + 1, 32), z(B, n, HW + 1, 32)) if want_A else (None, None, None)
        for s in range(KK):
            idx = key[:, s]
            dq += dS16[..., s:s + 1] * kz[:, :, idx]
            dk.index_add_(2, idx, dS16[..., s:s + 1] * q)
            dv.index_add_(2, idx, P16[..., s:s + 1] * do)
            if want_A:
                Aq += dS_abs[..., s:s + 1] * kz[:, :, idx].abs()
                Ak.index_add_(2, idx, dS_abs[..., s:s + 1] * q.abs())
                Av.index_add_(2, idx, P[..., s:s + 1] * do.abs())
        if extra is not None:
            qp, kp, bn = (a.to(dev) for a in extra)
            pe = (SCALE * (q[:, :, qp] * kz[:, :, kp]).sum(-1) + rz[:, bn][None] - lse[:, :, qp]).exp()
            dse = pe * ((do[:, :, qp] * vz[:, :, kp]).sum(-1) - delta[:, :, qp, 0])
            dk.index_add_(2, kp, bfm(dse)[..., None] * q[:, :, qp])
            dv.index_add_(2, kp, bfm(pe)[..., None] * do[:, :, qp])
        g = torch.stack([bf(SCALE * dq), bf(SCALE * dk[:, :, :HW]), bf(dv[:, :, :HW])], 2)              # (B, n, 3, HW, 32)
        R["out"][:, :, sl] = o.permute(0, 2, 1, 3)
        R["lse"][:, sl] = lse * LOG2E if defect == "i_lse_in_log2_units" else lse
        R["dqkv"][:, :, :, sl] = g.permute(0, 3, 2, 1, 4)
        R["drpb"][sl] = z(n, RB2 + 1).index_add_(1, gbin.reshape(-1), dS.sum(0).reshape(n, HW * KK))[:, :RB2]
        if want_A:
            gA = torch.stack([SCALE * Aq, SCALE * Ak[:, :, :HW], Av[:, :, :HW]], 2)
            A["dqkv"][:, :, :, sl] = gA.permute(0, 3, 2, 1, 4)
            A["drpb"][sl] = z(n, RB2 + 1).index_add_(1, gbin.reshape(-1), dS_abs.sum(0).reshape(n, HW * KK))[:, :RB2]
    shape = lambda r: dict(out=r["out"].view(B, H, W, nh, 32), dqkv=r["dqkv"].view(B, H, W, 3, nh, 32), drpb=r["drpb"].view(nh, 2 * K - 1, 2 * K - 1),
                           **({"lse": r["lse"].view(B, nh, H, W)} if "lse" in r else {}))
    return shape(R), (shape(A) if want_A else None)


def emulate(t, case, defect=None, heads=None):
    return neigh(t, case, rounded=True, defect=defect, heads=heads)[0]


# ---- bars ---------------------------------------------------------------------------------------------------------------------------------
def floor(r64):
    """The part of every bar that does not scale with A: 8 ulp of the output's largest element, plus the smallest normal fp32 number."""
    return 8.0 * U24 * float(r64.abs().max()) + TINY


def bar(name, r64, A, kappa):
    """The per-element bar of output `name` of the bf16 kernels (a tensor of r64's shape); kappa = KAPPA[route][name]."""
    b = kappa * U9 * A + floor(r64)
    return b + U8 * r64.abs() if name in BF16_OUTPUTS else b


def bar32(name, r64, A, gamma=None):
    """The per-element bar of output `name` of the fp32 kernels."""
    gamma = GAMMA[name] if gamma is None else gamma
    return gamma * U24 * A + floor(r64)


def rho(name, emu, r64, A, unit=U9, out_rounding=True):
    """max (|emu - r64| - output rounding)^+ / (unit A) of one output, over the elements whose A term is itself a normal fp32 number
    (unit A >= 2^-126); the others must be inside the floor alone."""
    excess = (emu - r64).abs() - (U8 * r64.abs() if out_rounding and name in BF16_OUTPUTS else 0.0)
    ok = unit * A >= TINY
    assert bool((excess[~ok] <= floor(r64)).all()), name
    return float((excess[ok].clamp_min(0) / (unit * A[ok])).max()) if bool(ok.any()) else 0.0


def rho32(name, emu32, r64, A):
    return rho(name, emu32.double(), r64, A, unit=U24, out_rounding=False)


def lse_bar(r64_lse, lse32):
    """(e_ref, bar) of the fp32 output lse: max(4 e_ref, 8 2^-24 max |r64|), e_ref = the error of emu32's log-sum-exp."""
    e_ref = float((lse32.double().to(r64_lse.device) - r64_lse).abs().max())
    return e_ref, max(4.0 * e_ref, 8.0 * U24 * float(r64_lse.abs().max()))
