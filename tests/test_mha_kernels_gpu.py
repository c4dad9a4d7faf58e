"""The decoder attention kernels of csrc/mha.hip (`mha_q_kernel<0|1, DROP>`, `mha_combine_kernel`, `mha_dkdv_kernel<DROP>`) through
`uenc_mha_fwd` / `uenc_mha_bwd` themselves, element by element against the float64 references of tests/mha_cases.py.

The C entry points are called directly, so lse, the fp32 dq, every operand's strides and the mask's row stride are the test's own;
`uenc.attention.mha` (which rounds dq to bf16 and keeps lse to itself) is run once, for `_strided` and `_mask_bytes`.

Bars (tests/mha_cases.py has the derivation; kappa = 2 RHO_EMU comes from the CPU emulation, never from a kernel):
  out, dk, dv (bf16): every element |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + 8 2^-24 max |r64|
  dq (fp32)         : every element |kernel - r64| <= kappa 2^-9 A + 8 2^-24 max |r64|
  lse (fp32)        : max |kernel - r64| <= max(4 e_ref, 8 2^-24 max |r64|), e_ref the error of the same log-sum-exp composed in fp32 torch on the GPU
  exact             : out, lse, dk, dv between two calls, between operand layouts and between mask row strides / pad bytes; dq likewise when the
                      case has one split (several splits add their partials with float atomics: the bar alone); a row that sees a single key
                      returns that key's v row; every sentinel outside an output's column slice.
No element is excused anywhere.  Rows with every key blocked are outside the contract (include/uenc.h does not define them, the model never
passes them) and no case has one.  Each case prints and records e_kernel, the worst share of the bar and kappa per output
(`record_parity("mha/...")`, written where UENC_PARITY_OUT points) before anything is asserted.
"""
import pytest
import torch

import mha_cases as MC
from conftest import record_parity

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -7.0                      # exact in bf16 and fp32
PAD_L, PAD_R = 8, 16                 # columns around the slices of a wider buffer (16-byte aligned slices, row strides a multiple of 8)
EINVAL = -1


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module")
def capi():
    from uenc import capi
    return capi


@pytest.fixture(autouse=True)
def _product_mode(K, monkeypatch):
    monkeypatch.setattr(K, "EXACT", False)


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _CASE.clear()


_CASE = {}


def _case(case):
    """Inputs (CPU and GPU), dropout weights, r64 / A (float64, on the GPU) of one case: built once per module and left unchanged."""
    if case["id"] not in _CASE:
        t = MC.inputs(case)
        w = None
        if case["p"] > 0:
            from uenc.attention import keep_mask_reference
            w = keep_mask_reference(case["B"], case["H"], case["Lq"], case["S"], case["p"], MC.DROP_SEED).double() / (1.0 - case["p"])
        r64, A = MC.reference(t, case, w)
        _CASE[case["id"]] = dict(t=t, g={n: (a.cuda() if a is not None else None) for n, a in t.items()},
                                 r64={n: a.cuda() for n, a in r64.items()}, A={n: a.cuda() for n, a in A.items()}, runs={})
    return _CASE[case["id"]]


def _wide(a=None, shape=None, dtype=None, strided=True, fill=SENTINEL):
    """(buffer, view): `a` (or a `fill`ed tensor of `shape`) as the column slice [PAD_L, PAD_L + E) of a wider buffer, or contiguous."""
    shape = tuple(a.shape) if a is not None else shape
    dtype = a.dtype if a is not None else dtype
    if strided:
        buf = torch.full(shape[:2] + (PAD_L + shape[2] + PAD_R,), fill, dtype=dtype, device="cuda")
        view = buf[..., PAD_L:PAD_L + shape[2]]
    else:
        buf = torch.full(shape, fill, dtype=dtype, device="cuda")
        view = buf
    if a is not None:
        view.copy_(a)
    return buf, view


def _packed(a, b, strided):
    """`a` and `b` (B, L, E) as the neighbouring column slices of one wider packed buffer (the way the in-projection hands over k | v), or
    each contiguous."""
    if not strided:
        return a.contiguous(), b.contiguous()
    E = a.shape[2]
    buf = torch.full(a.shape[:2] + (PAD_L + 2 * E + PAD_R,), SENTINEL, dtype=a.dtype, device="cuda")
    buf[..., PAD_L:PAD_L + E] = a
    buf[..., PAD_L + E:PAD_L + 2 * E] = b
    return buf[..., PAD_L:PAD_L + E], buf[..., PAD_L + E:PAD_L + 2 * E]


def _untouched(buf, view):
    """Every element of `buf` outside the column slice `view` still holds the sentinel."""
    if buf is view:
        return True
    E = view.shape[2]
    return bool((buf[..., :PAD_L] == SENTINEL).all()) and bool((buf[..., PAD_L + E:] == SENTINEL).all())


def _mask_bytes(mask, extra, pad):
    """(B, Lq, rs) uint8 with rs = S rounded up to 4, plus `extra`; pad bytes = `pad`."""
    if mask is None:
        return None
    B, Lq, S = mask.shape
    m8 = torch.full((B, Lq, -(-S // 4) * 4 + extra), pad, dtype=torch.uint8, device="cuda")
    m8[..., :S] = mask
    return m8


def _sdp(x):
    return (x.data_ptr(), x.stride(0), x.stride(1))


def _nsplit(capi, case):
    nws = capi.lib.uenc_mha_fwd_workspace_floats(case["B"], case["H"], case["Lq"], case["S"])
    slices = -(-case["Lq"] // MC.MQ)
    assert nws % (case["B"] * case["H"] * slices * MC.MQ * 34) == 0
    return (nws // (case["B"] * case["H"] * slices * MC.MQ * 34) or 1), nws


def _run(capi, case, g, strided, mask_extra=0, mask_pad=0, dq_prefill=None):
    """One forward and one backward; returns the outputs (views) and whether every sentinel around them survived."""
    lib, B, H, Lq, S = capi.lib, case["B"], case["H"], case["Lq"], case["S"]
    E = 32 * H
    q, do = _packed(g["q"], g["dout"], strided)
    k, v = _packed(g["k"], g["v"], strided)
    m8 = _mask_bytes(g["mask"], mask_extra, mask_pad)
    mptr, mrs = (m8.data_ptr(), m8.shape[2]) if m8 is not None else (0, 0)
    _, nws = _nsplit(capi, case)
    ws = torch.empty(max(nws, 1), device="cuda")
    obuf, out = _wide(shape=(B, Lq, E), dtype=BF16, strided=strided)
    lse = torch.full((B, H, Lq), SENTINEL, device="cuda")
    capi.check(lib.uenc_mha_fwd(*_sdp(q), *_sdp(k), *_sdp(v), mptr, mrs, *_sdp(out), lse.data_ptr(), ws.data_ptr() if nws else 0,
                                B, H, Lq, S, MC.SCALE, case["p"], MC.DROP_SEED, capi.stream_ptr()), "mha_fwd")
    qbuf, dq = _wide(shape=(B, Lq, E), dtype=F32, strided=strided)
    dq.copy_(dq_prefill) if dq_prefill is not None else dq.zero_()
    kbuf, dk = _wide(shape=(B, S, E), dtype=BF16, strided=strided)
    vbuf, dv = _wide(shape=(B, S, E), dtype=BF16, strided=strided)
    capi.check(lib.uenc_mha_bwd(*_sdp(q), *_sdp(k), *_sdp(v), mptr, mrs, *_sdp(out), lse.data_ptr(), *_sdp(do), *_sdp(dq), *_sdp(dk), *_sdp(dv),
                                B, H, Lq, S, MC.SCALE, case["p"], MC.DROP_SEED, capi.stream_ptr()), "mha_bwd")
    torch.cuda.synchronize()
    intact = all(_untouched(b, x) for b, x in ((obuf, out), (qbuf, dq), (kbuf, dk), (vbuf, dv)))
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, intact=intact)


def _bits(a):
    return a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check(tag, name, got, c):
    """One output against its bar, every element; figures printed and recorded first."""
    r64, A = c["r64"][name], c["A"][name]
    assert got.shape == r64.shape and got.dtype == (BF16 if name in MC.BF16_OUTPUTS else F32), (tag, name)
    err = (got.double() - r64).abs()
    share = err / MC.bar(name, r64, A)
    figs = dict(e_kernel=float(err.max()), worst_share_of_bar=float(share.max()), kappa=MC.KAPPA[name], r64_abs_max=float(r64.abs().max()))
    print(f"{tag}/{name}", figs)
    record_parity(f"{tag}/{name}", **figs)
    return figs


# the layout of a case's main run: strided operands, a mask row 68 bytes (more than a key block) longer than it must be, pad bytes 0xFF
MAIN = dict(strided=True, mask_extra=68, mask_pad=0xFF)


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c["id"])
def test_kernels_against_float64(capi, case):
    c = _case(case)
    tag = f"mha/{case['id']}"
    nsplit, _ = _nsplit(capi, case)
    assert nsplit == case["nsplit"], (case["id"], nsplit)                   # the case still reaches the split count it was written for
    r1 = _run(capi, case, c["g"], **MAIN)
    r2 = _run(capi, case, c["g"], **MAIN)
    c["runs"]["main"] = r1
    figs = {n: _check(tag, n, r1[n], c) for n in MC.OUTPUTS}
    e_ref, lbar = MC.lse_bar(c["r64"]["lse"], MC.lse_fp32(c["t"], case, "cuda"))
    lfig = dict(e_kernel=float((r1["lse"].double() - c["r64"]["lse"]).abs().max()), e_ref=e_ref, bar=lbar)
    print(f"{tag}/lse", lfig)
    record_parity(f"{tag}/lse", **lfig)
    for n in MC.OUTPUTS:
        assert figs[n]["worst_share_of_bar"] <= 1.0, (case["id"], n, figs[n])
    assert lfig["e_kernel"] <= lbar, (case["id"], lfig)
    # two calls: the same bits wherever nothing is accumulated atomically
    for n in ("out", "lse", "dk", "dv") + (("dq",) if nsplit == 1 else ()):
        assert _same_bits(r1[n], r2[n]), (case["id"], n)
    assert r1["intact"] and r2["intact"], case["id"]                         # nothing written outside the column slices
    # a row that sees one key: probability 1, one split with weight 1 -> that key's v row, bit for bit
    if case["p"] == 0.0:
        for b, qi, key in MC.single_key_rows(case):
            assert _same_bits(r1["out"][b, qi], c["g"]["v"][b, key]), (case["id"], b, qi, key)


@pytest.mark.parametrize("case", MC.CASES, ids=lambda c: c["id"])
def test_layout_and_mask_padding_do_not_matter(capi, case):
    """Contiguous operands, the shortest mask row (S rounded up to 4) and pad bytes of 0 against the strided run with a longer mask row and
    pad bytes of 0xFF: out, lse, dk, dv bit for bit, dq too with one split and inside its bar otherwise."""
    c = _case(case)
    main = c["runs"].get("main") or _run(capi, case, c["g"], **MAIN)
    variants = [dict(strided=False, mask_extra=0, mask_pad=0)]
    if case["masked"]:
        variants += [dict(strided=False, mask_extra=0, mask_pad=0xFF), dict(strided=True, mask_extra=68, mask_pad=0)]
    for var in variants:
        r = _run(capi, case, c["g"], **var)
        assert r["intact"], (case["id"], var)
        for n in ("out", "lse", "dk", "dv") + (("dq",) if case["nsplit"] == 1 else ()):
            assert _same_bits(r[n], main[n]), (case["id"], var, n)
        share = float(((r["dq"].double() - c["r64"]["dq"]).abs() / MC.bar("dq", c["r64"]["dq"], c["A"]["dq"])).max())
        assert share <= 1.0, (case["id"], var, share)


@pytest.mark.parametrize("cid", ["q15-m", "q160-u"])
def test_dq_is_accumulated(capi, cid):
    """dq = prefill + gradient.  Every split adds its partial to the element with one fp32 atomic: nsplit roundings of a running sum that
    stays below |prefill| + A_dq (the absolute contraction bounds the partials' magnitudes), on top of the gradient's own bar."""
    case = MC.BY_ID[cid]
    c = _case(case)
    pre = torch.randn(case["B"], case["Lq"], 32 * case["H"], generator=torch.Generator().manual_seed(3)).cuda()
    r = _run(capi, case, c["g"], strided=True, mask_extra=0, mask_pad=0, dq_prefill=pre)
    want = pre.double() + c["r64"]["dq"]
    bar = MC.bar("dq", c["r64"]["dq"], c["A"]["dq"]) + case["nsplit"] * MC.U24 * (pre.double().abs() + c["A"]["dq"])
    share = float(((r["dq"].double() - want).abs() / bar).max())
    print(f"mha/dq_prefill/{cid}", share)
    record_parity(f"mha/dq_prefill/{cid}", worst_share_of_bar=share)
    assert share <= 1.0 and r["intact"]


def test_wrapper_strides_and_bool_mask(K):
    """uenc.attention.mha on q with a 16-byte misaligned column slice, k as an aligned slice (consumed in place), v and dout with a non-unit
    inner stride, and a bool mask with S % 4 = 3: `_strided` and `_mask_bytes` against the same reference.  The wrapper rounds dq to bf16."""
    from uenc.attention import mha
    case = MC.BY_ID["q17-m"]
    assert case["S"] % 4 == 3
    c = _case(case)
    g, H, E = c["g"], case["H"], 32 * case["H"]
    qw = torch.zeros(case["B"], case["Lq"], E + 12, dtype=BF16, device="cuda")
    qw[..., 4:4 + E] = g["q"]
    kw = torch.zeros(case["B"], case["S"], E + 24, dtype=BF16, device="cuda")
    kw[..., 8:8 + E] = g["k"]
    vt = g["v"].transpose(1, 2).contiguous()
    for a in (qw, kw, vt):
        a.requires_grad_(True)
    q, k, v = qw[..., 4:4 + E], kw[..., 8:8 + E], vt.transpose(1, 2)
    assert q.data_ptr() % 16 != 0 and k.data_ptr() % 16 == 0 and not k.is_contiguous() and v.stride(2) != 1
    out = mha(q, k, v, H, g["mask"])
    dout = g["dout"].transpose(1, 2).contiguous().transpose(1, 2)
    assert dout.stride(2) != 1
    dqw, dkw, dvt = torch.autograd.grad(out, (qw, kw, vt), dout)
    got = dict(out=out.detach(), dq=dqw[..., 4:4 + E], dk=dkw[..., 8:8 + E], dv=dvt.transpose(1, 2))
    for n in MC.OUTPUTS:
        assert got[n].dtype == BF16
        r64, A = c["r64"][n], c["A"][n]
        bar = MC.bar(n, r64, A) + (MC.U8 * r64.abs() if n == "dq" else 0.0)          # dq: the wrapper's own rounding to bf16
        share = float(((got[n].double() - r64).abs() / bar).max())
        print(f"mha/wrapper/{n}", share)
        record_parity(f"mha/wrapper/{n}", worst_share_of_bar=share)
        assert share <= 1.0, (n, share)
    assert not bool(dqw[..., :4].any()) and not bool(dqw[..., 4 + E:].any()) and not bool(dkw[..., :8].any())


# ---- argument checks: UENC_EINVAL, and nothing launched -----------------------------------------------------------------------------
def _call(capi, B=1, H=2, Lq=5, S=6, masked=True, p=0.0, backward=True, **bad):
    """A small valid call with the operands, strides and sizes in `bad` replaced; returns the return codes of the forward and (if asked for)
    the backward and whether out, dq, dk, dv still hold their sentinels."""
    lib, E = capi.lib, 32 * H
    z = lambda L, dtype=BF16, fill=SENTINEL: torch.full((B, L, E + 8), fill, dtype=dtype, device="cuda")
    q, k, v, do = z(Lq, fill=1.0), z(S, fill=1.0), z(S, fill=1.0), z(Lq, fill=1.0)
    out, dk, dv, dq = z(Lq), z(S), z(S), z(Lq, F32)
    lse = torch.zeros(B, H, Lq, device="cuda")
    mrs = -(-S // 4) * 4
    m8 = torch.zeros(B * Lq * mrs + 8, dtype=torch.uint8, device="cuda")
    nws = lib.uenc_mha_fwd_workspace_floats(B, H, Lq, S)
    ws = torch.empty(max(nws, 1), device="cuda")
    a = dict(q=q.data_ptr(), q_bs=q.stride(0), q_rs=q.stride(1), k=k.data_ptr(), k_bs=k.stride(0), k_rs=k.stride(1),
             v=v.data_ptr(), v_bs=v.stride(0), v_rs=v.stride(1), mask=m8.data_ptr() if masked else 0, mask_rs=mrs if masked else 0,
             ws=ws.data_ptr() if nws else 0, p=p)
    for name, val in bad.items():
        a[name] = a[name] + val[1] if isinstance(val, tuple) else val                       # ("add", n): relative to the valid value
    head = (a["q"], a["q_bs"], a["q_rs"], a["k"], a["k_bs"], a["k_rs"], a["v"], a["v_bs"], a["v_rs"], a["mask"], a["mask_rs"])
    rc_f = lib.uenc_mha_fwd(*head, *_sdp(out), lse.data_ptr(), a["ws"], B, H, Lq, S, MC.SCALE, a["p"], 1, capi.stream_ptr())
    rc_b = None
    if backward:
        rc_b = lib.uenc_mha_bwd(*head, *_sdp(out), lse.data_ptr(), *_sdp(do), *_sdp(dq), *_sdp(dk), *_sdp(dv), B, H, Lq, S, MC.SCALE, a["p"], 1,
                                capi.stream_ptr())
    torch.cuda.synchronize()
    return rc_f, rc_b, all(bool((x == SENTINEL).all()) for x in (out, dq, dk, dv))


REJECTS = [
    ("q row stride not a multiple of 8", dict(q_rs=("add", 4))),
    ("k batch stride not a multiple of 8", dict(k_bs=("add", 2))),
    ("v row stride not a multiple of 8", dict(v_rs=("add", 1))),
    ("q not 16-byte aligned", dict(q=("add", 8))),
    ("v not 16-byte aligned", dict(v=("add", 2))),
    ("mask not 4-byte aligned", dict(mask=("add", 1))),
    ("mask_rs not a multiple of 4", dict(mask_rs=("add", 2))),
    ("mask_rs below S", dict(mask_rs=4)),
    ("dropout_p = 1", dict(p=1.0)),
    ("dropout_p < 0", dict(p=-0.25)),
]


@pytest.mark.parametrize("why,bad", REJECTS, ids=[w for w, _ in REJECTS])
def test_arguments_are_refused(capi, why, bad):
    assert _call(capi) == (0, 0, False)                                      # the call itself is valid ...
    assert _call(capi, **bad) == (EINVAL, EINVAL, True), why                 # ... and refused for the one thing changed, nothing written


def test_null_workspace_is_refused(capi):
    B, H, Lq, S = 1, 2, 5, 129
    assert capi.lib.uenc_mha_fwd_workspace_floats(B, H, Lq, S) > 0
    assert _call(capi, B, H, Lq, S, backward=False) == (0, None, False)
    assert _call(capi, B, H, Lq, S, backward=False, ws=0) == (EINVAL, None, True)


@pytest.mark.parametrize("masked,Lq", MC.BWD_REJECT_LQ)
def test_backward_refuses_too_many_queries_before_it_launches(capi, masked, Lq):
    """One query more than the dK / dV kernel can hold in LDS: the forward accepts it, the backward returns UENC_EINVAL and has not
    touched dq either (the refusal used to come after the dQ launch)."""
    lib, B, H, S = capi.lib, 1, 2, 8
    E = 32 * H
    g = torch.Generator().manual_seed(11)
    q, k, v, do = (torch.randn(B, n, E, generator=g).cuda().to(BF16) for n in (Lq, S, S, Lq))
    out = torch.empty(B, Lq, E, dtype=BF16, device="cuda")
    lse = torch.empty(B, H, Lq, device="cuda")
    m8 = torch.zeros(B, Lq, S, dtype=torch.uint8, device="cuda")
    m8[:, :, 1::2] = 1
    head = (*_sdp(q), *_sdp(k), *_sdp(v), m8.data_ptr() if masked else 0, S if masked else 0)
    assert lib.uenc_mha_fwd_workspace_floats(B, H, Lq, S) == 0
    assert lib.uenc_mha_fwd(*head, *_sdp(out), lse.data_ptr(), 0, B, H, Lq, S, MC.SCALE, 0.0, 0, capi.stream_ptr()) == 0
    dq = torch.full((B, Lq, E), SENTINEL, device="cuda")
    dk, dv = (torch.full((B, S, E), SENTINEL, dtype=BF16, device="cuda") for _ in range(2))
    rc = lib.uenc_mha_bwd(*head, *_sdp(out), lse.data_ptr(), *_sdp(do), *_sdp(dq), *_sdp(dk), *_sdp(dv), B, H, Lq, S, MC.SCALE, 0.0, 0,
                          capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == EINVAL
    assert all(bool((x == SENTINEL).all()) for x in (dq, dk, dv))
