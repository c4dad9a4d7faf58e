"""The query-tiled attention kernels of csrc/attn_tiled.hip (`attn_tiled_q_kernel<0|1, DROP>`, `attn_tiled_dkdv_kernel<DROP>`) through
`uenc_attn_tiled_fwd` / `_bwd` (and their seed-slot twins) themselves, element by element against the float64 reference of tests/mha_cases.py.

Bars (tests/attn_tiled_cases.py; kappa = 2 RHO_EMU comes from the CPU emulation over that table, never from a kernel):
  out, dk, dv (bf16): every element |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + 8 2^-24 max |r64|
  dq (fp32)         : every element |kernel - r64| <= kappa 2^-9 A + 8 2^-24 max |r64|
  lse (fp32)        : max |kernel - r64| <= max(4 e_ref, 8 2^-24 max |r64|), e_ref the error of the same log-sum-exp composed in fp32 torch on the GPU
  exact             : every output (dq included: nothing is accumulated atomically) between two calls and between operand layouts; a row
                      that sees a single key returns that key's v row; every sentinel in the gaps of the wider buffers.
Layouts: "packed" = q | k as neighbouring column slices of ONE buffer where Lq = S (the self-attention in-projection's output, read in
place), k | v packed otherwise, outputs as slices of wider buffers; "wide" = every operand a slice of its own wider buffer; "contig".
Each case prints and records its figures (`record_parity("attn_tiled/...")`) before anything is asserted.
"""
import pytest
import torch

import attn_tiled_cases as AC
import mha_cases as MC
from conftest import record_parity

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -7.0                      # exact in bf16 and fp32
PAD_L, PAD_R = 8, 16
EINVAL = -1
SLOT = 3


@pytest.fixture(scope="module")
def capi():
    from uenc import capi
    return capi


@pytest.fixture(autouse=True)
def _product_mode(monkeypatch):
    from uenc import kernels
    monkeypatch.setattr(kernels, "EXACT", False)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _CASE.clear()


_CASE = {}


def _case(case):
    """Inputs (CPU and GPU), r64 / A (float64, on the GPU) of one case: built once per module and left unchanged."""
    if case["id"] not in _CASE:
        t = AC.inputs(case)
        r64, A = MC.reference(t, case, AC.weights(case))
        _CASE[case["id"]] = dict(t=t, g={n: a.cuda() for n, a in t.items() if a is not None}, r64={n: a.cuda() for n, a in r64.items()},
                                 A={n: a.cuda() for n, a in A.items()}, runs={})
    return _CASE[case["id"]]


def _slices(parts, mode):
    """`parts` [(B, L, E) ...] as column slices: mode "packed" = neighbours in one wider buffer, "wide" = each in its own, "contig".
    Returns (views, buffers)."""
    if mode == "contig":
        return [p.contiguous() for p in parts], []
    groups = [parts] if mode == "packed" else [[p] for p in parts]
    views, bufs = [], []
    for grp in groups:
        E = grp[0].shape[2]
        buf = torch.full(grp[0].shape[:2] + (PAD_L + len(grp) * E + PAD_R,), SENTINEL, dtype=grp[0].dtype, device="cuda")
        for i, p in enumerate(grp):
            buf[..., PAD_L + i * E:PAD_L + (i + 1) * E] = p
            views.append(buf[..., PAD_L + i * E:PAD_L + (i + 1) * E])
        bufs.append((buf, len(grp) * E))
    return views, bufs


def _out(shape, dtype, mode):
    if mode == "contig":
        o = torch.full(shape, SENTINEL, dtype=dtype, device="cuda")
        return o, (o, None)
    buf = torch.full(shape[:2] + (PAD_L + shape[2] + PAD_R,), SENTINEL, dtype=dtype, device="cuda")
    return buf[..., PAD_L:PAD_L + shape[2]], (buf, shape[2])


def _gaps_intact(buf, width):
    return width is None or (bool((buf[..., :PAD_L] == SENTINEL).all()) and bool((buf[..., PAD_L + width:] == SENTINEL).all()))


def _sdp(x):
    return (x.data_ptr(), x.stride(0), x.stride(1))


def _run(capi, case, g, mode):
    """One forward and one backward; returns the outputs (views) and whether every sentinel around them survived."""
    lib, B, H, Lq, S = capi.lib, case["B"], case["H"], case["Lq"], case["S"]
    E = 32 * H
    if mode == "packed" and Lq == S:
        (q, k), _ = _slices([g["q"], g["k"]], "packed")
        (v,), _ = _slices([g["v"]], "wide")
    else:
        (q,), _ = _slices([g["q"]], "wide" if mode != "contig" else "contig")
        (k, v), _ = _slices([g["k"], g["v"]], mode)
    (do,), _ = _slices([g["dout"]], "wide" if mode != "contig" else "contig")
    out, ob = _out((B, Lq, E), BF16, mode)
    lse = torch.full((B, H, Lq), SENTINEL, device="cuda")
    seeds = torch.full((8,), 12345, dtype=torch.int32, device="cuda")
    seeds[SLOT] = AC.DROP_SEED
    slot = case["seed_mode"] == "slot"
    tail = (seeds.data_ptr(), SLOT, capi.stream_ptr()) if slot else (AC.DROP_SEED, capi.stream_ptr())
    fwd, bwd = (lib.uenc_attn_tiled_fwd_sp, lib.uenc_attn_tiled_bwd_sp) if slot else (lib.uenc_attn_tiled_fwd, lib.uenc_attn_tiled_bwd)
    capi.check(fwd(*_sdp(q), *_sdp(k), *_sdp(v), *_sdp(out), lse.data_ptr(), B, H, Lq, S, AC.SCALE, case["p"], *tail), "attn_tiled_fwd")
    dq, qb = _out((B, Lq, E), F32, mode)
    dk, kb = _out((B, S, E), BF16, mode)
    dv, vb = _out((B, S, E), BF16, mode)
    capi.check(bwd(*_sdp(q), *_sdp(k), *_sdp(v), *_sdp(out), lse.data_ptr(), *_sdp(do), *_sdp(dq), *_sdp(dk), *_sdp(dv), B, H, Lq, S,
                   AC.SCALE, case["p"], *tail), "attn_tiled_bwd")
    torch.cuda.synchronize()
    intact = all(_gaps_intact(*b) for b in (ob, qb, kb, vb))
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, intact=intact)


def _bits(a):
    return a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(tag, name, got, c):
    r64, A = c["r64"][name], c["A"][name]
    assert got.shape == r64.shape and got.dtype == (BF16 if name in AC.BF16_OUTPUTS else F32), (tag, name)
    err = (got.double() - r64).abs()
    share = err / AC.bar(name, r64, A)
    figs = dict(e_kernel=float(err.max()), worst_share_of_bar=float(share.max()), kappa=AC.KAPPA[name], r64_abs_max=float(r64.abs().max()))
    print(f"{tag}/{name}", figs)
    record_parity(f"{tag}/{name}", **figs)
    return figs


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c["id"])
def test_kernels_against_float64(capi, case):
    c = _case(case)
    tag = f"attn_tiled/{case['id']}"
    r1 = _run(capi, case, c["g"], "packed")
    r2 = _run(capi, case, c["g"], "packed")
    c["runs"]["main"] = r1
    figs = {n: _check(tag, n, r1[n], c) for n in AC.OUTPUTS}
    e_ref, lbar = MC.lse_bar(c["r64"]["lse"], MC.lse_fp32(c["t"], case, "cuda"))
    lfig = dict(e_kernel=float((r1["lse"].double() - c["r64"]["lse"]).abs().max()), e_ref=e_ref, bar=lbar)
    print(f"{tag}/lse", lfig)
    record_parity(f"{tag}/lse", **lfig)
    for n in AC.OUTPUTS:
        assert figs[n]["worst_share_of_bar"] <= 1.0, (case["id"], n, figs[n])
    assert lfig["e_kernel"] <= lbar, (case["id"], lfig)
    for n in ("out", "lse", "dq", "dk", "dv"):                               # two calls: the same bits, dq included (no atomics)
        assert _same_bits(r1[n], r2[n]), (case["id"], n)
    assert r1["intact"] and r2["intact"], case["id"]                         # nothing written outside the column slices
    if case["S"] == 1:                                                       # a row that sees one key: that key's v row, bit for bit
        for b in range(case["B"]):
            for qi in range(case["Lq"]):
                assert _same_bits(r1["out"][b, qi], c["g"]["v"][b, 0]), (case["id"], b, qi)


@pytest.mark.parametrize("case", AC.CASES, ids=lambda c: c["id"])
def test_layout_does_not_matter(capi, case):
    """Contiguous operands and one wider buffer per operand against the packed run: every output bit for bit, every gap untouched."""
    c = _case(case)
    main = c["runs"].get("main") or _run(capi, case, c["g"], "packed")
    for mode in ("contig", "wide"):
        r = _run(capi, case, c["g"], mode)
        assert r["intact"], (case["id"], mode)
        for n in ("out", "lse", "dq", "dk", "dv"):
            assert _same_bits(r[n], main[n]), (case["id"], mode, n)


def test_dq_is_written_not_accumulated(capi):
    """dq needs no zeroing: a prefilled buffer gives the same bits (`_run` prefills every output with the sentinel) -- and the forward's
    out and lse do not depend on what the buffers held."""
    case = AC.BY_ID["q70-s33"]
    c = _case(case)
    r = _run(capi, case, c["g"], "contig")
    assert not bool((r["dq"] == SENTINEL).any()) and not bool((r["lse"] == SENTINEL).any())
    share = float(((r["dq"].double() - c["r64"]["dq"]).abs() / AC.bar("dq", c["r64"]["dq"], c["A"]["dq"])).max())
    assert share <= 1.0


def test_wrapper_and_autograd(capi):
    """ops.attention_tiled on the slices of a packed in-projection output (consumed in place) with autograd: the same reference; the
    wrapper rounds dq to bf16."""
    from uenc import ops
    case = AC.BY_ID["q129-s129"]
    c = _case(case)
    g, H, E = c["g"], case["H"], 32 * case["H"]
    qkv = torch.cat([g["q"], g["k"], g["v"]], -1).requires_grad_(True)
    q, k, v = qkv[..., :E], qkv[..., E:2 * E], qkv[..., 2 * E:]
    out = ops.attention_tiled(q, k, v, H)
    (dqkv,) = torch.autograd.grad(out, (qkv,), g["dout"])
    got = dict(out=out.detach(), dq=dqkv[..., :E], dk=dqkv[..., E:2 * E], dv=dqkv[..., 2 * E:])
    for n in AC.OUTPUTS:
        assert got[n].dtype == BF16
        r64, A = c["r64"][n], c["A"][n]
        bar = AC.bar(n, r64, A) + (MC.U8 * r64.abs() if n == "dq" else 0.0)          # dq: the wrapper's own rounding to bf16
        share = float(((got[n].double() - r64).abs() / bar).max())
        print(f"attn_tiled/wrapper/{n}", share)
        record_parity(f"attn_tiled/wrapper/{n}", worst_share_of_bar=share)
        assert share <= 1.0, (n, share)


# ---- argument checks: UENC_EINVAL, and nothing launched -----------------------------------------------------------------------------
def _call(capi, B=1, H=2, Lq=5, S=6, p=0.0, **bad):
    """A small valid call with the operands, strides and sizes in `bad` replaced; returns the return codes of the forward and the backward
    and whether out, dq, dk, dv still hold their sentinels."""
    lib, E = capi.lib, 32 * H
    z = lambda L, dtype=BF16, fill=SENTINEL: torch.full((B, L, E + 8), fill, dtype=dtype, device="cuda")
    q, k, v, do = z(Lq, fill=1.0), z(S, fill=1.0), z(S, fill=1.0), z(Lq, fill=1.0)
    out, dk, dv, dq = z(Lq), z(S), z(S), z(Lq, F32)
    lse = torch.zeros(B, H, Lq, device="cuda")
    a = dict(q=q.data_ptr(), q_bs=q.stride(0), q_rs=q.stride(1), k=k.data_ptr(), k_bs=k.stride(0), k_rs=k.stride(1),
             v=v.data_ptr(), v_bs=v.stride(0), v_rs=v.stride(1), out=out.data_ptr(), o_rs=out.stride(1), dq=dq.data_ptr(), dq_rs=dq.stride(1),
             dk=dk.data_ptr(), dk_rs=dk.stride(1), p=p, B=B, H=H, Lq=Lq, S=S)
    for name, val in bad.items():
        a[name] = a[name] + val[1] if isinstance(val, tuple) else val                       # ("add", n): relative to the valid value
    head = (a["q"], a["q_bs"], a["q_rs"], a["k"], a["k_bs"], a["k_rs"], a["v"], a["v_bs"], a["v_rs"])
    sizes = (a["B"], a["H"], a["Lq"], a["S"], AC.SCALE, a["p"], 1, capi.stream_ptr())
    rc_f = lib.uenc_attn_tiled_fwd(*head, a["out"], out.stride(0), a["o_rs"], lse.data_ptr(), *sizes)
    rc_b = lib.uenc_attn_tiled_bwd(*head, a["out"], out.stride(0), a["o_rs"], lse.data_ptr(), *_sdp(do), a["dq"], dq.stride(0), a["dq_rs"],
                                   a["dk"], dk.stride(0), a["dk_rs"], *_sdp(dv), *sizes)
    torch.cuda.synchronize()
    return rc_f, rc_b, all(bool((x == SENTINEL).all()) for x in (out, dq, dk, dv))


# (why, bad, the forward refuses too)
REJECTS = [
    ("q row stride not a multiple of 8", dict(q_rs=("add", 4)), True),
    ("k batch stride not a multiple of 8", dict(k_bs=("add", 2)), True),
    ("v row stride not a multiple of 8", dict(v_rs=("add", 1)), True),
    ("q not 16-byte aligned", dict(q=("add", 8)), True),
    ("v not 16-byte aligned", dict(v=("add", 2)), True),
    ("out row stride not a multiple of 4", dict(o_rs=("add", 2)), True),
    ("out not 8-byte aligned", dict(out=("add", 2)), True),
    ("q NULL", dict(q=0), True),
    ("Lq = 0", dict(Lq=0), True),
    ("S = 0", dict(S=0), True),
    ("H = 0", dict(H=0), True),
    ("dropout_p = 1", dict(p=1.0), True),
    ("dropout_p < 0", dict(p=-0.25), True),
    ("dq row stride not a multiple of 4", dict(dq_rs=("add", 2)), False),
    ("dq not 16-byte aligned", dict(dq=("add", 8)), False),
    ("dk row stride not a multiple of 4", dict(dk_rs=("add", 1)), False),
    ("dk not 8-byte aligned", dict(dk=("add", 4)), False),
]


@pytest.mark.parametrize("why,bad,fwd_too", REJECTS, ids=[w for w, _, _ in REJECTS])
def test_arguments_are_refused(capi, why, bad, fwd_too):
    assert _call(capi) == (0, 0, False)                                      # the call itself is valid ...
    rc_f, rc_b, untouched = _call(capi, **bad)                               # ... and refused for the one thing changed
    assert rc_b == EINVAL, why
    if fwd_too:
        assert rc_f == EINVAL and untouched, why                             # nothing written at all
    else:
        assert rc_f == 0, why                                                # (the forward does not take that operand)


def test_seed_slot_arguments_are_refused(capi):
    lib = capi.lib
    x = torch.ones(1, 4, 32, dtype=BF16, device="cuda")
    o = torch.full((1, 4, 32), SENTINEL, dtype=BF16, device="cuda")
    lse = torch.zeros(1, 1, 4, device="cuda")
    seeds = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = (*_sdp(x), *_sdp(x), *_sdp(x), *_sdp(o), lse.data_ptr(), 1, 1, 4, 4, AC.SCALE, 0.1)
    assert lib.uenc_attn_tiled_fwd_sp(*args, 0, 0, capi.stream_ptr()) == EINVAL
    assert lib.uenc_attn_tiled_fwd_sp(*args, seeds.data_ptr(), -1, capi.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert bool((o == SENTINEL).all())
