"""Shared by tests/test_wattn_cases_cpu.py and tests/test_wattn_kernels_gpu.py: the case table of the window-attention kernels of
csrc/window_attn.hip (`wattn_fwd_kernel<NT>`, `wattn_bwd_kernel<NT, LSE>`, `wattn_dtable_kernel<NT>`, `wattn_dtable_grouped_kernel`,
`relpos_expand_kernel`) and of their fp32 twins in csrc/exact.hip (`xwin_fwd_kernel`, `xwin_bwd_kernel`), their inputs, references,
bars and the defects the bars must see.

Nothing here imports `uenc`.  Inputs come from a seeded CPU generator; qkv, the qkv bias and dO are rounded to bf16 once, so a reference
sees exactly the values the kernels see.  q and k have standard deviation 2 (a peaked softmax: one wrong key moves a row), v, dO and the
qkv bias standard deviation 1; the relative-position table is fp32 with standard deviation 1; head_dim is 32.

  r64   `reference`: the Swin block's attention restated step by step in float64 on the data itself -- the qkv bias appended as the
        padded tokens, torch.roll by -shift, window partition, scale q k^T + table[relative_position_index] + the mask built from the
        img_mask slices (0, -ws), (-ws, -shift), (-shift, None) with -100, softmax, @ v, window reverse, roll back, crop -- and every
        gradient by float64 autograd, so nothing of the kernels' closed forms is in it.  Returns out (B, L, C), lse (B, L, nH) in log2
        units, dqkv (B, L, 3C), dtable ((2ws-1)^2, nH) and dpad (3C).
  A     `windowed(...)[1]`: per output the same contraction over absolute values, the scale the bf16 rounding points act on:
        A_out = P |v|, A_dv = P^T |dO|, dS_abs = |dS| + P sum_d |o_d dO_d|, A_dq = scale dS_abs |k|, A_dk = scale dS_abs^T |q|;
        A_dtable sums dS_abs along each diagonal q - key = const; A_dpad sums A_dq, A_dk, A_dv over the padding slots.
  emu   `emulate`: float64 in the window domain with the rounding points of csrc/window_attn.hip and nothing else of it.  Forward: the
        unnormalised exponentials rounded to bf16 in front of the P V product, the unrounded normaliser applied behind it, out rounded to
        bf16.  Backward: delta from the bf16 saved out times dO; phase A keeps dS = P (dP - delta) unrounded for the table gradient and
        rounds it to bf16 in front of the dQ product; the normalised P rounded to bf16 is the P image, dV = P16^T dO, phase B's
        dS = bf16(P16 (dP - delta)) feeds dK; dq, dk, dv rounded to bf16 behind the scale; the padding slots' dk, dv unrounded into dpad.
  emu32 `reference(..., dtype=torch.float32)`: the r64 code evaluated in float32, the yardstick of the fp32 kernels.

Bars, every element, nothing excused.  out, dqkv (bf16): |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + floor, floor = 8 2^-24 max |r64| + 2^-126
(`floor` says what the second term is for); dtable, dpad (fp32): the same without the first term.  kappa = 2 RHO_EMU[output], where
RHO_EMU bounds rho = max over all cases and elements (those whose A term is a normal fp32 number; the rest answer to the floor) of
(|emu - r64| - 2^-8 |r64|)^+ / (2^-9 A): the emulation sets the scale, never a kernel; tests/test_wattn_cases_cpu.py asserts
rho <= RHO_EMU and that RHO_EMU is no loose cap.  The factor 2 is for what the kernels do and the emulation does not -- fp32 summation
order, the 1-ulp hardware exp2, the table gradient's partial sums and atomics, P = exp2(s - lse) against e / sum -- each of which changes
which way a bf16 rounding falls, not its size.  lse: max(4 e_ref, 8 2^-24 max |r64|), e_ref the error of emu32's log-sum-exp.
fp32 kernels: |kernel - r64| <= gamma 2^-24 A + floor, gamma = 8 RHO32[output], RHO32 the worst ratio of emu32 measured the
same way.  The 8: the kernels add a row's up to 144 scores and 32 channels strictly one after the other and rescale online where torch
sums in blocks of 8 or more lanes -- random-walk growth of about sqrt(144 / 8) ~ 4 -- times the usual 2.

DEFECTS are applied to the emulation; the bars must see each in the cases DEFECT_CASES aims it at.  Two are documented as WITHIN the bar,
and nothing is tuned to catch them:
  g_mask_log_base        the mask as -100 in log2 units (-69.3 natural) instead of -100 natural.  Either value leaves a masked key a
                         probability of e^-69 times e^(score gap) or less, some twenty orders of magnitude below the floor of every
                         bar and below float64's resolution of the sums it enters (the defective emulation is bit for bit the sound
                         one); the reference's own -100 is just as arbitrary a stand-in for -inf.
  j_dtable_from_bf16_ds  the table gradient summed from the bf16-rounded dS of phase A: each term moves by at most 2^-9 |dS|, which is
                         what kappa 2^-9 A_dtable allows by construction.
"""
import torch

LOG2E = 1.4426950408889634
SCALE = 32 ** -0.5
U8, U9, U24 = 2.0 ** -8, 2.0 ** -9, 2.0 ** -24
TINY = 2.0 ** -126                  # the smallest normal fp32 number
MAX_SCORES = 32 * 1024 * 1024        # B * windows * nH * N^2 of any case: keeps every GPU test at a few seconds
OUTPUTS = ("out", "dqkv", "dtable", "dpad")
BF16_OUTPUTS = ("out", "dqkv")

# Largest rho of the emulation over the whole table, rounded up to two decimals (measured: out 1.446 in n-g5, dqkv 1.812 and dtable 0.609
# in n-g16, dpad 0.648 in p-ws3); tests/test_wattn_cases_cpu.py asserts it, and that it is no loose cap
RHO_EMU = {"out": 1.45, "dqkv": 1.82, "dtable": 0.61, "dpad": 0.65}
KAPPA = {k: 2.0 * v for k, v in RHO_EMU.items()}
# The same for emu32 in units of 2^-24 A (measured: out 80.85 and dqkv 58.59 in n-g5, dtable 24.4 to 25.1 in k-ws12-s6 depending on the
# thread count, dpad 7.44 in d-ws5).  An fp32 sum depends on the order the BLAS build adds in, which a float64 emulation is blind to: the
# figures sit about 4 % above the measurement, in the middle of the window tests/test_wattn_cases_cpu.py allows (rho32 <= RHO32 <= 1.1 rho32)
RHO32 = {"out": 84.0, "dqkv": 61.0, "dtable": 25.9, "dpad": 7.75}
GAMMA = {k: 8.0 * v for k, v in RHO32.items()}


def ntiles(ws: int) -> int:
    """16-token tiles of a window = the NTILES instantiation, restated from wattn_ntiles."""
    return -(-ws * ws // 16)


def bwd_groups(B: int, H: int, W: int, nH: int, ws: int) -> int:
    """Workgroups per head of the persistent backward, restated from wattn_bwd_groups.  The GPU test asserts it against
    uenc_window_attn_bwd_groups, so a retuned heuristic fails loudly."""
    nwin = B * -(-H // ws) * -(-W // ws)
    nt = ntiles(ws)
    target = 256 if nt >= 5 else (512 if nt >= 3 else 1024)
    return min(max(target // nH, 1), nwin)


def ws_floats(B: int, H: int, W: int, nH: int, ws: int) -> int:
    """Floats of the dense dS partials [nH][G][NP][NP], restated from uenc_window_attn_bwd_ws_floats."""
    return nH * bwd_groups(B, H, W, nH, ws) * (16 * ntiles(ws)) ** 2


def windows_per_group(case):
    """How many windows each of the G workgroups of a head walks: window g, g + G, ..."""
    G = bwd_groups(case["B"], case["H"], case["W"], case["nH"], case["ws"])
    return [len(range(g, n_windows(case), G)) for g in range(G)]


# (id, ws, shift, B, H, W, nH): what each case reaches
_TABLE = [
    ("a-ws1", 1, 0, 1, 3, 5, 2),            # N = 1: out must equal v bit for bit; 15 windows, the forward grid rounds up to 16
    ("b-ws2", 2, 1, 2, 3, 5, 1),            # N = 4 of NP = 16, padding on both axes, two images
    ("c-ws4", 4, 2, 1, 8, 8, 3),            # N == NP = 16: no key >= N at all; odd head count: `npair` with a missing head
    ("d-ws5", 5, 2, 1, 9, 11, 2),           # NT 2, padding on both axes
    ("e-ws6", 6, 3, 1, 13, 7, 2),           # NT 3: an odd tile count (the zero half of the last 32-key block), target = 512
    ("f-ws7", 7, 3, 1, 15, 20, 3),          # NT 4, N = 49 of 64
    ("g-ws8", 8, 4, 1, 16, 16, 1),          # N == NP = 64, no padding
    ("h-ws9", 9, 4, 1, 19, 10, 2),          # NT 6: target = 256
    ("i-ws10", 10, 5, 1, 11, 21, 1),        # NT 7: odd
    ("j-ws11", 11, 5, 1, 12, 23, 2),        # NT 8
    ("k-ws12-s0", 12, 0, 1, 25, 37, 2),     # NT 9 (the loader wave, the LDS bias table), padding; run with and without lse
    ("k-ws12-s6", 12, 6, 1, 25, 37, 2),     # the same, shifted
    ("l-one-token", 12, 0, 1, 1, 1, 1),     # one token, 143 padding slots: out is mostly qkv-bias keys, dpad the main gradient
    ("l-ws7-pad", 7, 3, 1, 2, 3, 1),        # padding-dominated small window, shifted
    ("m-hp-eq-ws", 7, 3, 1, 5, 16, 1),      # Hp == ws with shift > 0: region3 with P == ws, the empty first slice of the reference's mask
    ("m-wp-eq-ws", 12, 6, 1, 30, 9, 1),     # Wp == ws
    ("n-g5", 12, 6, 1, 36, 72, 48),         # G = 5 over 18 windows: 4/4/4/3/3 per workgroup -- three slot tables, both stages; with and without lse
    ("n-g16", 7, 3, 1, 28, 42, 32),         # G = 16 over 24 windows: 2 windows for workgroups 0-7, one for the rest, in the <= 8-wave kernel
    ("o-batch", 7, 0, 3, 14, 21, 2),        # 18 windows, not a multiple of 8; batch independence
    ("p-ws3", 3, 1, 1, 7, 8, 1),            # N = 9 of 16: the one window size the table above leaves out
]
CASES = [dict(id=i, ws=ws, shift=s, B=B, H=H, W=W, nH=nH, seed=2000 + n) for n, (i, ws, s, B, H, W, nH) in enumerate(_TABLE)]
BY_ID = {c["id"]: c for c in CASES}

# defect -> the cases it is aimed at (tests/test_wattn_cases_cpu.py)
DEFECT_CASES = {
    "a_relpos_swapped": ["d-ws5", "e-ws6", "k-ws12-s0"],
    "b_mask_boundary_off_by_one": ["d-ws5", "m-hp-eq-ws", "k-ws12-s6"],
    "c_roll_reversed": ["b-ws2", "f-ws7", "k-ws12-s6"],
    "d_padding_slot_reads_zeros": ["d-ws5", "l-ws7-pad", "k-ws12-s0"],
    "e_padding_keys_masked": ["d-ws5", "l-one-token", "m-wp-eq-ws"],
    "f_tail_keys_admitted": ["b-ws2", "e-ws6", "i-ws10"],
    "g_mask_log_base": ["d-ws5", "k-ws12-s6"],
    "h_lse_without_bias": ["c-ws4", "k-ws12-s0"],
    "i_dpad_without_k": ["d-ws5", "l-ws7-pad", "k-ws12-s0"],
    "j_dtable_from_bf16_ds": ["c-ws4", "h-ws9", "k-ws12-s6"],
}
_ALL = ("out", "lse", "dqkv", "dtable", "dpad")
# the outputs a defect must move beyond the bar; () = documented as within the bar (module docstring)
DEFECT_REACH = {
    "a_relpos_swapped": _ALL, "b_mask_boundary_off_by_one": _ALL, "c_roll_reversed": _ALL, "d_padding_slot_reads_zeros": _ALL,
    "e_padding_keys_masked": _ALL, "f_tail_keys_admitted": ("out", "lse", "dqkv", "dtable"), "g_mask_log_base": (),
    "h_lse_without_bias": ("lse",), "i_dpad_without_k": ("dpad",), "j_dtable_from_bf16_ds": (),
}
# the outputs a defect must leave bit for bit as they were
DEFECT_UNTOUCHED = {"h_lse_without_bias": ("out", "dqkv", "dtable", "dpad"), "i_dpad_without_k": ("out", "lse", "dqkv", "dtable"),
                    "j_dtable_from_bf16_ds": ("out", "lse", "dqkv", "dpad")}


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def padded(case):
    ws = case["ws"]
    return -(-case["H"] // ws) * ws, -(-case["W"] // ws) * ws


def n_windows(case) -> int:
    Hp, Wp = padded(case)
    return case["B"] * (Hp // case["ws"]) * (Wp // case["ws"])


def n_scores(case) -> int:
    return n_windows(case) * case["nH"] * case["ws"] ** 4


def inputs(case):
    """qkv (B, L, 3C), qkv_bias (3C), dout (B, L, C) bf16 and table ((2ws-1)^2, nH) fp32 on the CPU; L = H W, C = 32 nH."""
    B, L, C, ws = case["B"], case["H"] * case["W"], 32 * case["nH"], case["ws"]
    g = _gen(case["seed"])
    qkv = torch.randn(B, L, 3 * C, generator=g)
    qkv[..., :2 * C] *= 2.0
    return dict(qkv=qkv.bfloat16(), qkv_bias=torch.randn(3 * C, generator=g).bfloat16(), dout=torch.randn(B, L, C, generator=g).bfloat16(),
                table=torch.randn((2 * ws - 1) ** 2, case["nH"], generator=g))


# ---- the Swin block's own steps ------------------------------------------------------------------------------------------------------
def _partition(x, ws):
    """(B, Hp, Wp, ...) -> (B * nW, ws * ws, ...)."""
    B, Hp, Wp = x.shape[:3]
    rest = tuple(x.shape[3:])
    x = x.reshape(B, Hp // ws, ws, Wp // ws, ws, *rest)
    return x.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(B * (Hp // ws) * (Wp // ws), ws * ws, *rest)


def _reverse(xw, ws, B, Hp, Wp):
    """(B * nW, ws * ws, ...) -> (B, Hp, Wp, ...)."""
    rest = tuple(xw.shape[2:])
    x = xw.reshape(B, Hp // ws, Wp // ws, ws, ws, *rest)
    return x.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(B, Hp, Wp, *rest)


def relative_position_index(ws: int):
    """(N, N): row of the table the pair (query, key) reads, (qy - ky + ws - 1) (2 ws - 1) + qx - kx + ws - 1."""
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)      # (2, N)
    rel = c[:, :, None] - c[:, None, :] + (ws - 1)
    return rel[0] * (2 * ws - 1) + rel[1]


def region_map(case, shift=None):
    """(Hp, Wp) region number of the shifted map: the three slices per axis, counted row-major."""
    Hp, Wp = padded(case)
    ws, shift = case["ws"], case["shift"] if shift is None else shift
    img = torch.zeros(Hp, Wp)
    if shift > 0:
        cnt = 0
        for hs in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            for wsl in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
                img[hs, wsl] = cnt
                cnt += 1
    return img


def shift_mask(case, dtype=torch.float64, device="cpu", shift=None):
    """(nW, N, N): -100 where query and key sit in different regions, 0 elsewhere; None without a shift."""
    if case["shift"] == 0:
        return None
    r = _partition(region_map(case, shift)[None], case["ws"])                        # (nW, N)
    d = r[:, None, :] - r[:, :, None]
    return torch.zeros_like(d).masked_fill(d != 0, -100.0).to(device=device, dtype=dtype)


def reference(t, case, dtype=torch.float64):
    """r64 (or, with dtype = float32, emu32): the block's attention on the data itself and autograd for the gradients; runs where the
    inputs live."""
    B, H, W, nH, ws, shift = (case[n] for n in ("B", "H", "W", "nH", "ws", "shift"))
    Hp, Wp = padded(case)
    C, N, dev = 32 * nH, ws * ws, t["qkv"].device
    qkv, bias, table = (t[n].to(dtype, copy=True).requires_grad_(True) for n in ("qkv", "qkv_bias", "table"))
    x = qkv.view(B, H, W, 3 * C)
    if Wp > W:                                                                       # the padded tokens: a zero row through the qkv Linear
        x = torch.cat([x, bias.expand(B, H, Wp - W, 3 * C)], 2)
    if Hp > H:
        x = torch.cat([x, bias.expand(B, Hp - H, Wp, 3 * C)], 1)
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    w = _partition(x, ws).reshape(-1, N, 3, nH, 32).permute(2, 0, 3, 1, 4)
    q, k, v = w[0], w[1], w[2]                                                       # (B nW, nH, N, 32)
    attn = (q * SCALE) @ k.transpose(-2, -1)
    attn = attn + table[relative_position_index(ws).reshape(-1).to(dev)].view(N, N, nH).permute(2, 0, 1)[None]
    if shift > 0:
        m = shift_mask(case, dtype, dev)
        attn = (attn.view(B, -1, nH, N, N) + m[None, :, None]).view(-1, nH, N, N)
    lse = torch.logsumexp(attn, -1).transpose(1, 2) * LOG2E                          # (B nW, N, nH)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(-1, N, C)

    def merge(a):
        a = _reverse(a, ws, B, Hp, Wp)
        if shift > 0:
            a = torch.roll(a, shifts=(shift, shift), dims=(1, 2))
        return a[:, :H, :W].reshape(B, H * W, -1)

    out = merge(o)
    dqkv, dpad, dtable = torch.autograd.grad(out, (qkv, bias, table), t["dout"].to(dtype), allow_unused=True)
    dpad = torch.zeros_like(bias) if dpad is None else dpad                          # no padding slot: the bias is not in the graph
    return dict(out=out.detach(), lse=merge(lse).detach(), dqkv=dqkv, dtable=dtable, dpad=dpad)


# ---- the window domain: closed forms, A, the emulation and the defects -----------------------------------------------------------------
def layout(case, roll=-1, mask_shift=None):
    """src (nW, N): token index of every slot of every window of ONE image, H W for a padding slot; rid (nW, N): its region number.
    The same pad / roll / partition as `reference`, on an index map."""
    H, W, ws, shift = case["H"], case["W"], case["ws"], case["shift"]
    Hp, Wp = padded(case)
    idx = torch.full((Hp, Wp), H * W, dtype=torch.int64)
    idx[:H, :W] = torch.arange(H * W).view(H, W)
    if shift > 0:
        idx = torch.roll(idx, shifts=(roll * shift, roll * shift), dims=(0, 1))
    return _partition(idx[None], ws), _partition(region_map(case, mask_shift)[None], ws).long()


def _bf(a):
    return a.float().bfloat16().double()


def windowed(t, case, rounded=False, defect=None):
    """(result, A).  rounded = False, defect = None: r64's closed forms in the window domain (tests/test_wattn_cases_cpu.py holds them
    against `reference`) and the absolute contractions A.  rounded = True: the emulation, with `defect` applied if given; A is None."""
    B, H, W, nH, ws, shift = (case[n] for n in ("B", "H", "W", "nH", "ws", "shift"))
    L, C, N, dev = H * W, 32 * nH, ws * ws, t["qkv"].device
    bf = _bf if rounded else (lambda a: a)
    src, rid = layout(case, roll=1 if defect == "c_roll_reversed" else -1,
                      mask_shift=shift + 1 if defect == "b_mask_boundary_off_by_one" else None)
    assert defect != "b_mask_boundary_off_by_one" or 0 < shift < ws - 1
    src, rid = src.to(dev), rid.to(dev)
    nW = src.shape[0]
    flat = src.reshape(-1)
    pad_row = torch.zeros(3 * C, dtype=torch.float64, device=dev) if defect == "d_padding_slot_reads_zeros" else t["qkv_bias"].double()
    z = torch.cat([t["qkv"].double(), pad_row.expand(B, 1, 3 * C)], 1)
    w = z[:, flat].view(B, nW, N, 3, nH, 32).permute(3, 0, 1, 4, 2, 5)
    q, k, v = w[0], w[1], w[2]                                                       # (B, nW, nH, N, 32)
    do = torch.cat([t["dout"].double(), torch.zeros(B, 1, C, dtype=torch.float64, device=dev)], 1)[:, flat]
    do = do.view(B, nW, N, nH, 32).permute(0, 1, 3, 2, 4)
    real = (src < L).double()                                                        # (nW, N)
    rpi = relative_position_index(ws).to(dev)
    tab = t["table"].double()[rpi.reshape(-1)].view(N, N, nH).permute(2, 0, 1)       # (nH, q, key)
    if defect == "a_relpos_swapped":
        tab = tab.transpose(1, 2)
    qk = SCALE * (q @ k.transpose(-1, -2))
    mask = 0.0
    if shift > 0:
        mask = (rid[:, :, None] != rid[:, None, :]).double() * (-100.0 / LOG2E if defect == "g_mask_log_base" else -100.0)
        mask = mask[None, :, None]
    s = qk + tab[None, None] + mask
    if defect == "e_padding_keys_masked":
        s = s - 1e30 * (1.0 - real)[None, :, None, None, :]
    NK = N
    if defect == "f_tail_keys_admitted":                                             # keys N .. NP - 1: zero rows, score 0, bias 0
        NK = 16 * ntiles(ws)
        assert NK > N
        ext = lambda a, dim: torch.cat([a, torch.zeros(a.shape[:dim] + (NK - N,) + a.shape[dim + 1:], dtype=a.dtype, device=dev)], dim)
        s, k, v = ext(s, 4), ext(k, 3), ext(v, 3)
    m = s.amax(-1, keepdim=True)
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)                                                      # the normaliser: unrounded
    s_lse = s - tab[None, None] if defect == "h_lse_without_bias" else s
    lse = torch.logsumexp(s_lse, -1) * LOG2E                                          # (B, nW, nH, N)
    o = bf((bf(e) @ v) / l) * real[None, :, None, :, None]                           # the saved out; a padding slot's row is read as zeros
    P = e / l
    dP = do @ v.transpose(-1, -2)
    od = o * do
    dd = dP - od.sum(-1, keepdim=True)                                               # dP - delta, delta from the rounded out
    dS = P * dd                                                                      # phase A: unrounded for the table gradient
    P16 = bf(P)
    dSB = bf(P16 * dd)                                                               # phase B
    dq = SCALE * (bf(dS) @ k)
    dk = SCALE * (dSB.transpose(-1, -2) @ q)[..., :N, :]
    dv = (P16.transpose(-1, -2) @ do)[..., :N, :]
    dS_tab = _bf(dS) if defect == "j_dtable_from_bf16_ds" else dS

    def rows(a):                                                                     # (B, nW, nH, N, 32) -> (B, nW N, C)
        return a.permute(0, 1, 3, 2, 4).reshape(B, nW * N, C)

    def scatter(a):                                                                  # -> (B, L + 1, .): row L collects the padding slots
        return torch.zeros(B, L + 1, a.shape[-1], dtype=torch.float64, device=dev).index_add_(1, flat, a)

    def diagonals(a):                                                                # (B, nW, nH, q, key) -> ((2ws-1)^2, nH)
        a = a[..., :N].sum((0, 1)).permute(1, 2, 0).reshape(N * N, nH)
        return torch.zeros((2 * ws - 1) ** 2, nH, dtype=torch.float64, device=dev).index_add_(0, rpi.reshape(-1), a)

    g = scatter(torch.cat([rows(dq), rows(dk), rows(dv)], -1))
    dpad = g[:, L].sum(0)
    if defect == "i_dpad_without_k":
        dpad = dpad.clone()
        dpad[C:2 * C] = 0.0
    r = dict(out=scatter(rows(o))[:, :L], lse=scatter(lse.permute(0, 1, 3, 2).reshape(B, nW * N, nH))[:, :L], dqkv=bf(g[:, :L]),
             dtable=diagonals(dS_tab), dpad=dpad)
    if rounded or defect is not None:
        return r, None
    dS_abs = dS.abs() + P * od.abs().sum(-1, keepdim=True)
    gA = scatter(torch.cat([rows(SCALE * (dS_abs @ k.abs())), rows(SCALE * (dS_abs.transpose(-1, -2) @ q.abs())),
                            rows(P.transpose(-1, -2) @ do.abs())], -1))
    A = dict(out=scatter(rows((P @ v.abs()) * real[None, :, None, :, None]))[:, :L], dqkv=gA[:, :L], dtable=diagonals(dS_abs),
             dpad=gA[:, L].sum(0))
    return r, A


def emulate(t, case, defect=None):
    return windowed(t, case, rounded=True, defect=defect)[0]


def floor(r64):
    """The part of every bar that does not scale with A: 8 ulp of the output's largest element, plus the smallest normal fp32 number.
    The second term matters for elements that only masked pairs reach (a table diagonal whose every pair crosses a region boundary, a
    padding key every real query is masked from): r64 and A are of order e^-100 there, below anything fp32 holds as a normal number."""
    return 8.0 * U24 * float(r64.abs().max()) + TINY


def bar(name, r64, A, kappa=None):
    """The per-element bar of output `name` of the bf16 kernels (a tensor of r64's shape)."""
    kappa = KAPPA[name] if kappa is None else kappa
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
