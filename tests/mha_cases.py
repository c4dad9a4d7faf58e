"""Shared by tests/test_mha_cases_cpu.py and tests/test_mha_kernels_gpu.py: the case table of the decoder attention kernels of csrc/mha.hip
(`mha_q_kernel<0|1, DROP>`, `mha_combine_kernel`, `mha_dkdv_kernel<DROP>`), their inputs, references, bars and the defects the bars must see.

Nothing here imports `uenc`.  Inputs come from a seeded CPU generator and are rounded to bf16 once, so a reference sees exactly the values
the kernels see.  q and k have standard deviation 2 (a peaked softmax: one wrong key moves a row), v and dO standard deviation 1.

  r64   `reference`: plain dense attention in float64, softmax(scale q k^T, blocked -> -inf) v, lse in the log2 domain, and dq / dk / dv by
        the closed forms dP = dO v^T, delta = sum_d o dO, dS = P (dP - delta), dq = scale dS k, dk = scale dS^T q, dv = P^T dO.  Dropout
        multiplies P by w = keep / (1 - p) behind the normaliser (include/uenc.h); the keep mask is handed in by the caller.
  A     per output the same contraction over absolute values, the scale the algorithm's bf16 rounding points act on:
        A_out = P |v|, A_dv = P^T |dO|, dS_abs = |dS| + P sum_d |o_d dO_d|, A_dq = scale dS_abs |k|, A_dk = scale dS_abs^T |q|.
  emu   `emulate`: float64 with the rounding points csrc/mha.hip documents and nothing else of it: the probabilities rounded to bf16 in
        front of the P V product, out rounded to bf16 and reused for delta, dS rounded to bf16 in front of both gradient products, bf16 dk
        and dv, fp32 dq.

Bar, per element of out, dk, dv (bf16):  |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + 8 2^-24 max |r64|;  dq (fp32): the same without the
first term.  kappa = 2 RHO_EMU[output], where RHO_EMU bounds rho = max over all cases and elements of (|emu - r64| - 2^-8 |r64|)^+ /
(2^-9 A) (no 2^-8 term for dq): the emulation sets the scale, never the kernel; tests/test_mha_cases_cpu.py asserts rho <= RHO_EMU.  The
factor 2 is for what the kernel does and the emulation does not -- fp32 summation order, the 1-ulp hardware exp2, rescaling across blocks
and splits, probabilities rounded relative to the running maximum -- each of which changes which way a bf16 rounding falls, not its size.

Rows with every key blocked are outside the contract (include/uenc.h does not define them and the model never passes them): no mask here
has one.  Only the DEFECTS below can leave a row without a visible key; such a row then gives zeros (out, and nothing to any gradient) and
lse = -inf, as a kernel whose normaliser stayed 0 would.
"""
import math

import torch

LOG2E = 1.4426950408889634
SCALE = 32 ** -0.5
MQ, KB = 160, 64                    # queries per launch slice, keys per LDS block (csrc/mha.hip)
U8, U9, U24 = 2.0 ** -8, 2.0 ** -9, 2.0 ** -24
MAX_SCORES = 4 * 1024 * 1024        # B * H * Lq * S of any case: keeps every GPU test at a few seconds
OUTPUTS = ("out", "dq", "dk", "dv")
BF16_OUTPUTS = ("out", "dk", "dv")

# Largest rho of the emulation over the whole table, rounded up to two decimals (measured: out 1.585 and dk 1.504 in drop-bh768, dq 1.230
# in drop-1split, dv 1.946 in bh768-s200); tests/test_mha_cases_cpu.py asserts it, and that it is no loose cap
RHO_EMU = {"out": 1.59, "dq": 1.24, "dk": 1.51, "dv": 1.95}
KAPPA = {k: 2.0 * v for k, v in RHO_EMU.items()}


def splits(B: int, H: int, S: int):
    """(nsplit, keys per split) of the key-range split, restated from mha_splits: about 768 workgroups, at most 64 splits, whole 64-key
    blocks.  The GPU test asserts every case's `nsplit` against uenc_mha_fwd_workspace_floats, so a retuned heuristic fails loudly."""
    nblocks = -(-S // KB)
    ns = max(1, min(-(-768 // (B * H)), nblocks, 64))
    per = -(-nblocks // ns) * KB
    return -(-S // per), per


# (id, B, H, Lq, S, masked, dropout p, nsplit): what each case reaches
_TABLE = [
    # -- heads and grid.  Even H: head-pair block numbering; odd H: plain numbering.  nsplit * B * H % 16 != 0: padded tail blocks return early
    ("h1", 3, 1, 17, 129, True, 0.0, 3),            # odd path, 9 of 16 blocks live, second query tile with one row, 1-key ragged block
    ("h3", 1, 3, 16, 127, False, 0.0, 2),           # odd path, 6 of 16 blocks, exactly one full query tile
    ("h2", 1, 2, 15, 63, True, 0.0, 1),             # one head pair, 2 of 16 blocks, one split in one ragged block, S % 4 = 3
    ("h6", 1, 6, 159, 128, False, 0.0, 2),          # three pairs, 12 of 16 blocks, last tile one row short
    ("h8-tail", 3, 8, 1, 64, False, 0.0, 1),        # 24 of 32 blocks, a single query, one full block
    # -- keys
    ("s1", 2, 2, 5, 1, False, 0.0, 1),              # a single key: every row returns v[0] bit for bit
    ("s3", 2, 3, 17, 3, True, 0.0, 1),              # one mask dword per row, S % 4 = 3
    ("s65-2split", 1, 8, 161, 65, True, 0.0, 2),    # B H = 8: two splits, the second owns ONE key; second launch slice of one row; S % 4 = 1
    ("s4097", 1, 8, 16, 4097, True, 0.0, 33),       # the 64-split cap engages (65 blocks -> 128 keys per split), last split owns one key
    ("s4033-64split", 1, 8, 16, 4033, False, 0.0, 64),   # 64 splits of one block, the last owns one key
    ("bh768-s130", 96, 8, 3, 130, True, 0.0, 1),    # B H = 768: one split over 3 blocks, direct write-out behind the online softmax; S % 4 = 2
    ("bh768-s200", 96, 8, 3, 200, False, 0.0, 1),   # the same over 4 blocks, unmasked
    ("dbuf", 7, 6, 17, 2100, True, 0.0, 17),        # 2 blocks per split and 17 splits: the double buffer inside a split, 714 of 720 blocks;
                                                    # the one-slice mask staging (next tile waits in registers)
    # -- queries: tile ownership qt = wave + 4 i, zero-padded rows, the second slice; S sweeps the block edges
    ("q1-u", 2, 2, 1, 63, False, 0.0, 1), ("q1-m", 2, 2, 1, 63, True, 0.0, 1),
    ("q15-u", 2, 2, 15, 64, False, 0.0, 1), ("q15-m", 2, 2, 15, 64, True, 0.0, 1),
    ("q16-u", 2, 2, 16, 65, False, 0.0, 2), ("q16-m", 2, 2, 16, 65, True, 0.0, 2),
    ("q17-u", 2, 2, 17, 127, False, 0.0, 2), ("q17-m", 2, 2, 17, 127, True, 0.0, 2),
    ("q159-u", 2, 2, 159, 128, False, 0.0, 2), ("q159-m", 2, 2, 159, 128, True, 0.0, 2),
    ("q160-u", 2, 2, 160, 129, False, 0.0, 3), ("q160-m", 2, 2, 160, 129, True, 0.0, 3),
    ("q161-u", 2, 2, 161, 65, False, 0.0, 2), ("q161-m", 2, 2, 161, 65, True, 0.0, 2),
    ("q481-m", 1, 1, 481, 4100, True, 0.0, 33),     # four slices, 2 blocks per split: the nslices > 1 mask staging loop and the LDS opt-in (141 KB)
    ("q640-m", 1, 2, 640, 130, True, 0.0, 3),       # the largest masked Lq the backward accepts
    ("q960-u", 1, 2, 960, 129, False, 0.0, 3),      # the largest unmasked Lq the backward accepts (144 KB)
    # -- dropout: mha_q_kernel<., true>, mha_dkdv_kernel<true>
    ("drop-1split", 2, 2, 161, 63, False, 0.1, 1),
    ("drop-3split-m", 2, 2, 161, 129, True, 0.5, 3),
    ("drop-10split-m", 1, 8, 17, 600, True, 0.1, 10),
    ("drop-bh768", 96, 8, 3, 130, False, 0.5, 1),
]
CASES = [dict(id=i, B=B, H=H, Lq=Lq, S=S, masked=m, p=p, nsplit=ns, seed=1000 + n) for n, (i, B, H, Lq, S, m, p, ns) in enumerate(_TABLE)]
BY_ID = {c["id"]: c for c in CASES}
DROP_SEED = 0x5EED

# argument checks: Lq the backward must refuse (masked?, Lq)
BWD_REJECT_LQ = [(True, 641), (False, 961)]

# defect -> the cases it is aimed at (tests/test_mha_cases_cpu.py)
DEFECT_CASES = {
    "a_last_key_dropped": ["q16-u", "q17-u", "q160-m", "s4033-64split"],
    "b_tile_row_takes_neighbour": ["q16-u", "q17-m", "q160-m"],
    "c_mask_shifted_one_key": ["h1", "s3", "q159-m", "s65-2split"],
    "d_one_mask_byte_flipped": ["q17-m", "bh768-s130", "q481-m"],
    "e_split_left_out": ["s65-2split", "dbuf", "q160-u"],
    "f_split_wrong_maximum": ["s65-2split", "dbuf", "q160-u"],
    "g_head_pair_swapped": ["s65-2split", "h2"],
    "h_delta_zero": ["q17-u", "q161-m", "bh768-s200"],
}
# the outputs a defect reaches (lse is listed where the defect moves it)
DEFECT_REACH = {
    "a_last_key_dropped": ("out", "lse", "dq", "dk", "dv"), "b_tile_row_takes_neighbour": ("out", "lse", "dq", "dk", "dv"),
    "c_mask_shifted_one_key": ("out", "lse", "dq", "dk", "dv"), "d_one_mask_byte_flipped": ("out", "lse", "dq", "dk", "dv"),
    "e_split_left_out": ("out", "lse", "dq", "dk", "dv"), "f_split_wrong_maximum": ("out", "lse", "dq", "dk", "dv"),
    "g_head_pair_swapped": ("out", "lse", "dq", "dk", "dv"), "h_delta_zero": ("dq", "dk"),
}


def _gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def make_mask(case):
    """(B, Lq, S) bool, True = blocked: 60 % blocked at random, every row with at least one visible key.  The first rows of image 0 are
    special (as far as Lq and S allow): row 0 sees only the LAST key (the last key of the ragged block), row 1 only key 0, row 2 nothing
    in the first 64-key block, row 3 nothing in the first split, row 4 nothing in the last split."""
    B, Lq, S = case["B"], case["Lq"], case["S"]
    g = _gen(case["seed"] + 7)
    m = torch.rand(B, Lq, S, generator=g) < 0.6
    nsplit, per = splits(B, case["H"], S)
    if Lq > 2 and S > KB:
        m[0, 2, :KB] = True
    if Lq > 3 and nsplit > 1:
        m[0, 3, :per] = True
    if Lq > 4 and nsplit > 1:
        m[0, 4, (nsplit - 1) * per:] = True
    forced = torch.randint(0, S, (B, Lq), generator=g)
    if Lq > 2 and S > KB:
        forced[0, 2] = KB + forced[0, 2] % (S - KB)
    if Lq > 3 and nsplit > 1:
        forced[0, 3] = per + forced[0, 3] % (S - per)
    if Lq > 4 and nsplit > 1:
        forced[0, 4] = forced[0, 4] % ((nsplit - 1) * per)
    m.scatter_(2, forced[..., None], False)
    m[0, 0, :] = True
    m[0, 0, S - 1] = False
    if Lq > 1:
        m[0, 1, :] = True
        m[0, 1, 0] = False
    return m


def single_key_rows(case):
    """[(b, query, key)] of the rows that see exactly one key: the kernels must return that key's v row bit for bit."""
    if not case["masked"]:
        return [(b, qi, 0) for b in range(case["B"]) for qi in range(case["Lq"])] if case["S"] == 1 else []
    vis = ~make_mask(case)
    rows = (vis.sum(-1) == 1).nonzero().tolist()
    return [(b, qi, int(vis[b, qi].nonzero()[0, 0])) for b, qi in rows]


def inputs(case):
    """q, dout (B, Lq, E) and k, v (B, S, E) bf16 on the CPU, E = 32 H, and `mask` (B, Lq, S) bool or None."""
    B, H, Lq, S = case["B"], case["H"], case["Lq"], case["S"]
    g = _gen(case["seed"])
    E = 32 * H
    t = dict(q=2.0 * torch.randn(B, Lq, E, generator=g), k=2.0 * torch.randn(B, S, E, generator=g),
             v=torch.randn(B, S, E, generator=g), dout=torch.randn(B, Lq, E, generator=g))
    t = {n: a.bfloat16() for n, a in t.items()}
    t["mask"] = make_mask(case) if case["masked"] else None
    return t


def _heads(a, H):
    B, L, _ = a.shape
    return a.double().view(B, L, H, 32).permute(0, 2, 1, 3)


def _rows(a):
    B, H, L, _ = a.shape
    return a.permute(0, 2, 1, 3).reshape(B, L, H * 32)


def scores(t, H, mask="own"):
    """(B, H, Lq, S) float64: scale q k^T, blocked -> -inf."""
    s = SCALE * (_heads(t["q"], H) @ _heads(t["k"], H).transpose(-1, -2))
    mask = t["mask"] if isinstance(mask, str) else mask
    return s if mask is None else s.masked_fill(mask[:, None], -math.inf)


def softmax_lse(s):
    """P and the log2-domain log-sum-exp of scores with -inf entries; a row with nothing visible gives P = 0, lse = -inf."""
    m = s.amax(-1, keepdim=True)
    m = torch.where(m.isfinite(), m, torch.zeros_like(m))
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)
    return e / l.clamp_min(1e-300), ((m + l.log()) * LOG2E).squeeze(-1)


def backward(s, lse, out_h, t, H, w=None, delta_zero=False):
    """dq, dk, dv and their absolute companions from the scores, the SAVED lse and out (B, H, Lq, 32), as the kernels take them."""
    q, k, v, do = (_heads(t[n], H) for n in ("q", "k", "v", "dout"))
    live = lse.isfinite()[..., None]                                # (a row without a visible key: defects only)
    P = torch.where(live, torch.exp2(s * LOG2E - torch.where(live, lse[..., None], torch.zeros_like(lse[..., None]))), torch.zeros_like(s))
    Pd = P if w is None else P * w
    dP = do @ v.transpose(-1, -2)
    dP = dP if w is None else dP * w
    delta = (out_h * do).sum(-1, keepdim=True)
    dS = P * (dP - (0.0 if delta_zero else delta))
    dS_abs = dS.abs() + P * (out_h * do).abs().sum(-1, keepdim=True)
    r = dict(dq=SCALE * (dS @ k), dk=SCALE * (dS.transpose(-1, -2) @ q), dv=Pd.transpose(-1, -2) @ do)
    A = dict(dq=SCALE * (dS_abs @ k.abs()), dk=SCALE * (dS_abs.transpose(-1, -2) @ q.abs()), dv=Pd.transpose(-1, -2) @ do.abs())
    return {n: _rows(a) for n, a in r.items()}, {n: _rows(a) for n, a in A.items()}


def reference(t, case, w=None):
    """r64 and A: dicts of out, dq, dk, dv in the (B, L, E) layout, r64 with lse (B, H, Lq) too.  w = keep / (1 - p) (B, H, Lq, S) or None."""
    H = case["H"]
    s = scores(t, H)
    P, lse = softmax_lse(s)
    Pd = P if w is None else P * w
    v = _heads(t["v"], H)
    out = Pd @ v
    r, A = backward(s, lse, out, t, H, w)
    r.update(out=_rows(out), lse=lse)
    A["out"] = _rows(Pd @ v.abs())
    return r, A


def _bf(a):
    return a.float().bfloat16().double()


def emulate(t, case, w=None):
    """The float64 reference with the rounding points of csrc/mha.hip (see the module docstring); same layout as `reference`."""
    H = case["H"]
    q, k, v, do = (_heads(t[n], H) for n in ("q", "k", "v", "dout"))
    s = scores(t, H)
    m = s.amax(-1, keepdim=True)
    e = (s - m).exp()
    l = e.sum(-1, keepdim=True)                                     # the normaliser: unrounded, before dropout
    lse = ((m + l.log()) * LOG2E).squeeze(-1)
    out = _bf((_bf(e if w is None else e * w) @ v) / l)             # probabilities rounded in front of P V; out rounded
    P = torch.exp2(s * LOG2E - lse[..., None])
    dP = do @ v.transpose(-1, -2)
    dP = dP if w is None else dP * w
    dSb = _bf(P * (dP - (out * do).sum(-1, keepdim=True)))          # delta from the rounded out; dS rounded
    Pb = _bf(P if w is None else P * w)
    return dict(out=_rows(out), lse=lse, dq=_rows(SCALE * (dSb @ k)).float().double(), dk=_rows(_bf(SCALE * (dSb.transpose(-1, -2) @ q))),
                dv=_rows(_bf(Pb.transpose(-1, -2) @ do)))


def bar(name, r64, A, kappa=None):
    """The per-element bar of output `name` (a tensor of r64's shape)."""
    kappa = KAPPA[name] if kappa is None else kappa
    b = kappa * U9 * A + 8.0 * U24 * float(r64.abs().max())
    return b + U8 * r64.abs() if name in BF16_OUTPUTS else b


def rho(name, emu, r64, A):
    """max (|emu - r64| - output rounding)^+ / (2^-9 A) of one output."""
    excess = (emu - r64).abs() - (U8 * r64.abs() if name in BF16_OUTPUTS else 0.0)
    ok = A > 0
    assert bool((excess[~ok] <= 0).all())
    return float((excess[ok].clamp_min(0) / (U9 * A[ok])).max()) if bool(ok.any()) else 0.0


def lse_fp32(t, case, device="cpu"):
    """The log2-domain log-sum-exp composed in fp32 torch on `device`: its distance from r64 is `e_ref` of the lse bar."""
    H = case["H"]
    q, k = (_heads(t[n].to(device), H).float() for n in ("q", "k"))
    s = SCALE * (q @ k.transpose(-1, -2))
    if t["mask"] is not None:
        s = s.masked_fill(t["mask"].to(device)[:, None], -math.inf)
    return torch.logsumexp(s, -1) * LOG2E


def lse_bar(r64_lse, t32_lse):
    """(e_ref, bar) of the fp32 output lse: max(4 e_ref, 8 2^-24 max |r64|), as tests/test_fpn_kernels_gpu.py judges fp32 outputs."""
    e_ref = float((t32_lse.double().cpu() - r64_lse.cpu()).abs().max())
    return e_ref, max(4.0 * e_ref, 8.0 * U24 * float(r64_lse.abs().max()))


# ---- defects ------------------------------------------------------------------------------------------------------------------------
def _split_forward(s, v, per, skip=None, wrong=None):
    """Forward through per-split partials (m, l, O) and the combine; `skip` = a split left out, `wrong` = (j, j2): split j is weighted with
    the maximum of split j2."""
    S = s.shape[-1]
    ns = -(-S // per)
    ms, ls, Os = [], [], []
    for j in range(ns):
        sj = s[..., j * per:(j + 1) * per]
        mj = sj.amax(-1, keepdim=True)
        mj = torch.where(mj.isfinite(), mj, torch.full_like(mj, -1e300))
        ej = (sj - mj).exp()
        ms.append(mj); ls.append(ej.sum(-1, keepdim=True)); Os.append(ej @ v[..., j * per:(j + 1) * per, :])
    M = torch.stack(ms).amax(0)
    L, O = torch.zeros_like(M), torch.zeros_like(Os[0])
    for j in range(ns):
        if j == skip:
            continue
        wj = (ms[wrong[1] if wrong is not None and j == wrong[0] else j] - M).exp()
        L, O = L + wj * ls[j], O + wj * Os[j]
    return torch.where(L > 0, O / L.clamp_min(1e-300), torch.zeros_like(O)), ((M + L.log()) * LOG2E).squeeze(-1)


def defective(defect: str, t, case):
    """The float64 result with one defect applied, in `reference`'s layout (out, lse, dq, dk, dv).  Forward defects reach the backward the
    way they would in the kernels: through the saved out and lse (combine defects) or through the scores both passes see."""
    H, S, Lq = case["H"], case["S"], case["Lq"]
    assert case["p"] == 0.0
    s = scores(t, H)
    v = _heads(t["v"], H)
    nsplit, per = splits(case["B"], H, S)
    sb = s                                                          # the scores the backward sees
    kw = {}
    if defect == "a_last_key_dropped":
        assert S % KB != 0 and S > 1
        s = s.clone(); s[..., S - 1] = -math.inf; sb = s
    elif defect == "b_tile_row_takes_neighbour":
        assert Lq >= 16
        s = s.clone(); s[..., 15, :] = s[..., 14, :]; sb = s
    elif defect == "c_mask_shifted_one_key":
        s = scores(t, H, torch.roll(t["mask"], 1, dims=-1)); sb = s
    elif defect == "d_one_mask_byte_flipped":
        # one byte: in the last row of the last image, the blocked key that head 0 scores highest becomes visible
        raw = scores(t, H, None)[-1, 0, -1]
        key = int(torch.where(t["mask"][-1, -1], raw, torch.full_like(raw, -math.inf)).argmax())
        m2 = t["mask"].clone(); m2[-1, -1, key] = False
        s = scores(t, H, m2); sb = s
    elif defect in ("e_split_left_out", "f_split_wrong_maximum", "g_head_pair_swapped", "h_delta_zero"):
        pass
    else:
        raise KeyError(defect)
    if defect == "e_split_left_out":
        assert nsplit > 1
        out, lse = _split_forward(s, v, per, skip=nsplit - 1)
    elif defect == "f_split_wrong_maximum":
        assert nsplit > 1
        out, lse = _split_forward(s, v, per, wrong=(0, 1))
    else:
        P, lse = softmax_lse(s)
        out = P @ v
    if defect == "h_delta_zero":
        kw["delta_zero"] = True
    r, _ = backward(sb, lse, out, t, H, **kw)
    r.update(out=_rows(out), lse=lse)
    if defect == "g_head_pair_swapped":
        assert H % 2 == 0
        perm = torch.arange(H).view(-1, 2).flip(1).reshape(-1)
        for n in OUTPUTS:
            B, L, _ = r[n].shape
            r[n] = r[n].view(B, L, H, 32)[:, :, perm].reshape(B, L, H * 32)
        r["lse"] = r["lse"][:, perm]
    return r
