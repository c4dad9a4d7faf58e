"""The window-attention kernels of csrc/window_attn.hip through `uenc_window_attn_fwd` / `uenc_window_attn_bwd` /
`uenc_window_attn_dtable_grouped` / `uenc_relpos_expand(_grouped)` themselves, and their fp32 twins of csrc/exact.hip through
`uenc_window_attn_f32_{fwd,bwd}`, element by element against the float64 references of tests/wattn_cases.py.

The C entry points are called directly, so lse, the dS scratch, the deferred table gradient and every buffer's size are the test's own.

Bars (tests/wattn_cases.py has the derivation; kappa = 2 RHO_EMU and gamma = 8 RHO32 come from CPU emulations, never from a kernel):
  out, dqkv (bf16)   : every element |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + floor,  floor = 8 2^-24 max |r64| + 2^-126
  dtable, dpad (fp32): every element |kernel - (prefill + r64)| <= kappa 2^-9 A + floor + n 2^-24 (|prefill| + A): both are ACCUMULATED into
                       non-zero caller buffers, with n float atomics per element (dtable: one per query tile; dpad: one per workgroup of the head)
  lse (fp32)         : max |kernel - r64| <= max(4 e_ref, 8 2^-24 max |r64|), e_ref the error of the same log-sum-exp composed in fp32 torch
  fp32 kernels       : every element |kernel - r64| <= gamma 2^-24 A + floor
  exact              : out and lse between two calls and between lse == NULL and lse given; out per image between a batch and its images
                       alone; dqkv between two calls and between defer_dtable 0 and 1 (no atomics touch it), and between lse given and lse
                       NULL wherever the kernel ignores lse (every window size but 12; at 12 the two runs compute P differently and each
                       is held to the bar alone); N = 1: out == v; the deferred table gradient equals the immediate one where a single
                       block adds per entry (NT == 1); 64 sentinel floats behind dS_ws, dtable, dpad, lse, bias_q, bias_k, out and dqkv.
No element is excused anywhere.  Each case prints and records e_kernel, the worst share of the bar and kappa (gamma) per output
(`record_parity("wattn/...")`, `record_parity("wattn_f32/...")`, written where UENC_PARITY_OUT points) before anything is asserted.
"""
import numpy as np
import pytest
import torch

import wattn_cases as WC
from conftest import record_parity

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -7.0                      # exact in bf16 and fp32
GUARD = 64                           # sentinel elements behind every buffer a kernel writes
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
    """Inputs (CPU and GPU), r64 / A (float64, on the GPU), emu32's lse and the accumulation prefills of one case: built once per module
    and left unchanged."""
    if case["id"] not in _CASE:
        t = WC.inputs(case)
        r64 = WC.reference(t, case)
        _, A = WC.windowed(t, case)
        gen = torch.Generator().manual_seed(case["seed"] + 5)
        pre = dict(dtable=torch.randn(r64["dtable"].shape, generator=gen).cuda(), dpad=torch.randn(r64["dpad"].shape, generator=gen).cuda())
        _CASE[case["id"]] = dict(t=t, g={n: a.cuda() for n, a in t.items()}, r64={n: a.cuda() for n, a in r64.items()},
                                 A={n: a.cuda() for n, a in A.items()}, lse32=WC.reference(t, case, F32)["lse"].cuda(), pre=pre, runs={})
    return _CASE[case["id"]]


def _guarded(n, dtype, fill=SENTINEL):
    """(buffer, view): n elements followed by GUARD sentinels."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    buf[:n] = fill
    return buf, buf[:n]


def _intact(bufs):
    return all(bool((b[-GUARD:] == SENTINEL).all()) for b in bufs)


def _geom(case):
    return case["B"], case["H"], case["W"], 32 * case["nH"], case["nH"], case["ws"], case["shift"]


def _expand(capi, table, nH, ws):
    """bias_q, bias_k (nH, NP, NP) of uenc_relpos_expand, and whether the sentinels behind them survived."""
    NP = capi.lib.uenc_window_attn_np(ws)
    assert NP == 16 * WC.ntiles(ws)
    qb, bq = _guarded(nH * NP * NP, F32)
    kb, bk = _guarded(nH * NP * NP, F32)
    capi.check(capi.lib.uenc_relpos_expand(table.data_ptr(), bq.data_ptr(), bk.data_ptr(), nH, ws, capi.stream_ptr()), "relpos_expand")
    torch.cuda.synchronize()
    return bq.view(nH, NP, NP), bk.view(nH, NP, NP), _intact((qb, kb))


def _run(capi, case, c, with_lse=True, defer=0, g=None, B=None):
    """One forward and one backward.  with_lse: the forward writes the row statistics and the backward gets them; otherwise both get NULL.
    Returns the outputs (views), the dS scratch and whether every sentinel survived."""
    lib = capi.lib
    g = c["g"] if g is None else g
    _, H, W, C, nH, ws, shift = _geom(case)
    B = case["B"] if B is None else B
    L = H * W
    bq, bk, ok = _expand(capi, g["table"], nH, ws)
    obuf, out = _guarded(B * L * C, BF16)
    lbuf, lse = _guarded(B * L * nH, F32)
    capi.check(lib.uenc_window_attn_fwd(g["qkv"].data_ptr(), g["qkv_bias"].data_ptr(), bq.data_ptr(), out.data_ptr(),
                                        lse.data_ptr() if with_lse else 0, B, H, W, C, nH, ws, shift, WC.SCALE, capi.stream_ptr()), "window_attn_fwd")
    nws = lib.uenc_window_attn_bwd_ws_floats(B, H, W, nH, ws)
    wbuf, dS = _guarded(nws, F32)
    gbuf, dqkv = _guarded(B * L * 3 * C, BF16)
    tbuf, dtable = _guarded(c["pre"]["dtable"].numel(), F32)
    pbuf, dpad = _guarded(3 * C, F32)
    dtable.copy_(c["pre"]["dtable"].reshape(-1))
    dpad.copy_(c["pre"]["dpad"])
    capi.check(lib.uenc_window_attn_bwd(g["qkv"].data_ptr(), g["qkv_bias"].data_ptr(), bq.data_ptr(), bk.data_ptr(), out.data_ptr(),
                                        lse.data_ptr() if with_lse else 0, g["dout"].data_ptr(), dqkv.data_ptr(), dS.data_ptr(), dtable.data_ptr(),
                                        dpad.data_ptr(), B, H, W, C, nH, ws, shift, WC.SCALE, defer, capi.stream_ptr()), "window_attn_bwd")
    torch.cuda.synchronize()
    intact = ok and _intact((obuf, lbuf, wbuf, gbuf, tbuf, pbuf))
    if not with_lse:
        intact = intact and bool((lse == SENTINEL).all())
    return dict(out=out.view(B, L, C), lse=lse.view(B, L, nH), dqkv=dqkv.view(B, L, 3 * C), dtable=dtable.view(c["pre"]["dtable"].shape),
                dpad=dpad, dS=dS, intact=intact)


def _bits(a):
    return a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _adds(case, name):
    """Float atomics per element of an accumulated output: dtable one per query tile, dpad one per workgroup of the head."""
    return WC.ntiles(case["ws"]) if name == "dtable" else WC.bwd_groups(case["B"], case["H"], case["W"], case["nH"], case["ws"])


def _check(tag, name, got, case, c):
    """One output against its bar, every element; figures printed and recorded first."""
    r64, A = c["r64"][name], c["A"][name]
    assert got.shape == r64.shape and got.dtype == (BF16 if name in WC.BF16_OUTPUTS else F32), (tag, name)
    bar, want = WC.bar(name, r64, A), r64
    if name in c["pre"]:
        pre = c["pre"][name].double()
        want, bar = pre + r64, bar + _adds(case, name) * WC.U24 * (pre.abs() + A)
    err = (got.double() - want).abs()
    figs = dict(e_kernel=float(err.max()), worst_share_of_bar=float((err / bar).max()), kappa=WC.KAPPA[name], r64_abs_max=float(r64.abs().max()))
    print(f"{tag}/{name}", figs)
    record_parity(f"{tag}/{name}", **figs)
    return figs


def _check_lse(tag, got, c):
    e_ref, lbar = WC.lse_bar(c["r64"]["lse"], c["lse32"])
    figs = dict(e_kernel=float((got.double() - c["r64"]["lse"]).abs().max()), e_ref=e_ref, bar=lbar)
    print(f"{tag}/lse", figs)
    record_parity(f"{tag}/lse", **figs)
    return figs


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c["id"])
def test_kernels_against_float64(capi, case):
    c = _case(case)
    tag = f"wattn/{case['id']}"
    B, H, W, C, nH, ws, shift = _geom(case)
    # the case still reaches the group count and the scratch size it was written for
    assert capi.lib.uenc_window_attn_bwd_groups(B, H, W, nH, ws) == WC.bwd_groups(B, H, W, nH, ws), case["id"]
    assert capi.lib.uenc_window_attn_bwd_ws_floats(B, H, W, nH, ws) == WC.ws_floats(B, H, W, nH, ws), case["id"]
    r1 = _run(capi, case, c)
    r2 = _run(capi, case, c)
    r0 = _run(capi, case, c, with_lse=False)
    rd = _run(capi, case, c, defer=1)
    c["runs"]["main"] = r1
    figs = {n: _check(tag, n, r1[n], case, c) for n in WC.OUTPUTS}
    figs0 = {n: _check(tag + "/no-lse", n, r0[n], case, c) for n in WC.OUTPUTS}
    lfig = _check_lse(tag, r1["lse"], c)
    for n in WC.OUTPUTS:
        assert figs[n]["worst_share_of_bar"] <= 1.0, (case["id"], n, figs[n])
        assert figs0[n]["worst_share_of_bar"] <= 1.0, (case["id"], "no lse", n, figs0[n])
    assert lfig["e_kernel"] <= lfig["bar"], (case["id"], lfig)
    # two calls: the same bits wherever nothing is accumulated atomically; the statistics do not change the forward
    for n in ("out", "lse", "dqkv"):
        assert _same_bits(r1[n], r2[n]), (case["id"], n)
    assert _same_bits(r1["out"], r0["out"]), case["id"]
    if ws != 12:                                                             # only the 12 x 12 backward reads lse
        assert _same_bits(r1["dqkv"], r0["dqkv"]), case["id"]
    # the deferred path: the same dqkv, nothing added to the table gradient, dpad inside its bar
    assert _same_bits(r1["dqkv"], rd["dqkv"]), case["id"]
    assert torch.equal(rd["dtable"], c["pre"]["dtable"]), case["id"]
    assert _check(tag + "/deferred", "dpad", rd["dpad"], case, c)["worst_share_of_bar"] <= 1.0
    assert r1["intact"] and r2["intact"] and r0["intact"] and rd["intact"], case["id"]       # nothing written behind any buffer
    if ws == 1:                                                              # one key: probability 1 -> v, bit for bit
        assert _same_bits(r1["out"], c["g"]["qkv"][..., 2 * C:]), case["id"]


def test_images_of_a_batch_do_not_see_each_other(capi):
    """Case o batched against its three images run alone: out and lse per image bit for bit."""
    case = WC.BY_ID["o-batch"]
    c = _case(case)
    main = c["runs"].get("main") or _run(capi, case, c)
    for b in range(case["B"]):
        g = dict(c["g"], qkv=c["g"]["qkv"][b:b + 1].contiguous(), dout=c["g"]["dout"][b:b + 1].contiguous())
        r = _run(capi, case, c, g=g, B=1)
        assert r["intact"], b
        for n in ("out", "lse", "dqkv"):
            assert _same_bits(r[n][0], main[n][b]), (b, n)


def _dtable_descriptors(items):
    """The 40-byte descriptors of uenc_window_attn_dtable_grouped in device memory, and the block count."""
    desc = np.zeros(len(items), dtype=[("wsd", "<u8"), ("dtab", "<u8"), ("G", "<i4"), ("nH", "<i4"), ("ws", "<i4"), ("ntiles", "<i4"),
                                       ("blk_begin", "<i4"), ("pad", "<i4")])
    assert desc.dtype.itemsize == 40
    blocks = 0
    for i, (wsd, dtab, G, nH, ws) in enumerate(items):
        desc[i] = (wsd.data_ptr(), dtab.data_ptr(), G, nH, ws, WC.ntiles(ws), blocks, 0)
        blocks += nH * WC.ntiles(ws)
    return torch.from_numpy(desc.view(np.uint8)).cuda(), blocks


def test_deferred_table_gradients_in_one_grouped_launch(capi):
    """defer_dtable = 1 leaves the dense dS partials; ONE uenc_window_attn_dtable_grouped launch over descriptors of different ws, ntiles
    and nH (1, 6, 9 and 9 tiles; 3, 2, 2 and 2 heads) reduces them: every table gradient inside its bar, and the NT == 1 one bit for bit
    what the immediate path gives (there a single block adds once per entry, from the same sums in the same order)."""
    ids = ["c-ws4", "h-ws9", "k-ws12-s6", "k-ws12-s0"]
    runs, items, bufs = [], [], []
    for cid in ids:
        case = WC.BY_ID[cid]
        c = _case(case)
        r = _run(capi, case, c, defer=1)
        B, H, W, _, nH, ws, _ = _geom(case)
        tbuf, dtab = _guarded(c["pre"]["dtable"].numel(), F32)
        dtab.copy_(c["pre"]["dtable"].reshape(-1))
        runs.append((case, c, r, dtab.view(c["pre"]["dtable"].shape)))
        bufs.append(tbuf)
        items.append((r["dS"], dtab, WC.bwd_groups(B, H, W, nH, ws), nH, ws))
    table, blocks = _dtable_descriptors(items)
    assert table.data_ptr() % 8 == 0
    capi.check(capi.lib.uenc_window_attn_dtable_grouped(table.data_ptr(), len(items), blocks, capi.stream_ptr()), "dtable_grouped")
    torch.cuda.synchronize()
    assert _intact(bufs)
    figs = [_check(f"wattn/grouped/{case['id']}", "dtable", dtab, case, c) for case, c, _, dtab in runs]
    for (case, _, _, _), f in zip(runs, figs):
        assert f["worst_share_of_bar"] <= 1.0, (case["id"], f)
    case, c, _, dtab = runs[0]
    assert WC.ntiles(case["ws"]) == 1
    assert _same_bits(dtab, (c["runs"].get("main") or _run(capi, case, c))["dtable"])


# ---- uenc_relpos_expand ---------------------------------------------------------------------------------------------------------------
def _expanded_on_the_host(table, ws):
    """bias_q (nH, NP, NP): float32(log2 e) * table gathered for q, key < N; -30000 in every column key >= N; 0 for q >= N, key < N."""
    nH, N, NP = table.shape[1], ws * ws, 16 * WC.ntiles(ws)
    want = torch.zeros(nH, NP, NP, device="cuda")
    rpi = WC.relative_position_index(ws).reshape(-1).cuda()
    want[:, :N, :N] = (torch.tensor(WC.LOG2E, dtype=F32, device="cuda") * table)[rpi].view(N, N, nH).permute(2, 0, 1)
    want[:, :, N:] = -30000.0
    return want


RELPOS = [(1, 2), (2, 1), (4, 3), (5, 2), (7, 3), (10, 1), (12, 2)]


@pytest.mark.parametrize("ws,nH", RELPOS)
def test_relpos_expand_values(capi, ws, nH):
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=torch.Generator().manual_seed(40 + ws)).cuda()
    bq, bk, intact = _expand(capi, table, nH, ws)
    want = _expanded_on_the_host(table, ws)
    N = ws * ws
    assert intact
    assert _same_bits(bq, want)
    assert bool((bq[:, :, N:] == -30000.0).all()) and bool((bq[:, N:, :N] == 0).all())
    assert _same_bits(bk, bq.transpose(1, 2))


def test_relpos_expand_grouped_equals_single(capi):
    """One grouped launch over descriptors of different ws, NP and nH, one of them with a NULL bias_k: bias_q and bias_k bit for bit what
    the single form writes, nothing behind the buffers, the NULL one not written."""
    specs = [(12, 2), (5, 3), (2, 1), (7, 2)]
    desc = np.zeros(len(specs), dtype=[("table", "<u8"), ("bias_q", "<u8"), ("bias_k", "<u8"), ("nH", "<i4"), ("ws", "<i4"), ("NP", "<i4"),
                                       ("blk_begin", "<i4")])
    assert desc.dtype.itemsize == 40
    keep, blocks = [], 0
    for i, (ws, nH) in enumerate(specs):
        NP = 16 * WC.ntiles(ws)
        table = torch.randn((2 * ws - 1) ** 2, nH, generator=torch.Generator().manual_seed(60 + ws)).cuda()
        qb, bq = _guarded(nH * NP * NP, F32)
        kb, bk = _guarded(nH * NP * NP, F32)
        null_k = i == 1
        desc[i] = (table.data_ptr(), bq.data_ptr(), 0 if null_k else bk.data_ptr(), nH, ws, NP, blocks)
        blocks += -(-(nH * NP * NP) // 2048)
        keep.append((table, ws, nH, NP, qb, bq, kb, bk, null_k))
    dev = torch.from_numpy(desc.view(np.uint8)).cuda()
    capi.check(capi.lib.uenc_relpos_expand_grouped(dev.data_ptr(), len(specs), blocks, capi.stream_ptr()), "relpos_expand_grouped")
    torch.cuda.synchronize()
    for table, ws, nH, NP, qb, bq, kb, bk, null_k in keep:
        sq, sk, intact = _expand(capi, table, nH, ws)
        assert intact and _intact((qb, kb)), ws
        assert _same_bits(bq.view(nH, NP, NP), sq), ws
        assert bool((bk == SENTINEL).all()) if null_k else _same_bits(bk.view(nH, NP, NP), sk), ws


# ---- the fp32 verification kernels ----------------------------------------------------------------------------------------------------
def _run32(capi, case, c, twice=False):
    lib = capi.lib
    B, H, W, C, nH, ws, shift = _geom(case)
    L = H * W
    qkv, bias, dout = c["g"]["qkv"].float(), c["g"]["qkv_bias"].float(), c["g"]["dout"].float()
    obuf, out = _guarded(B * L * C, F32)
    capi.check(lib.uenc_window_attn_f32_fwd(qkv.data_ptr(), bias.data_ptr(), c["g"]["table"].data_ptr(), out.data_ptr(), B, H, W, C, nH, ws, shift,
                                            WC.SCALE, capi.stream_ptr()), "window_attn_f32_fwd")
    gbuf, dqkv = _guarded(B * L * 3 * C, F32)
    tbuf, dtable = _guarded(c["pre"]["dtable"].numel(), F32, 0.0)
    pbuf, dpad = _guarded(3 * C, F32, 0.0)
    for _ in range(2 if twice else 1):
        capi.check(lib.uenc_window_attn_f32_bwd(qkv.data_ptr(), bias.data_ptr(), c["g"]["table"].data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                                                dtable.data_ptr(), dpad.data_ptr(), B, H, W, C, nH, ws, shift, WC.SCALE, capi.stream_ptr()),
                   "window_attn_f32_bwd")
    torch.cuda.synchronize()
    return dict(out=out.view(B, L, C), dqkv=dqkv.view(B, L, 3 * C), dtable=dtable.view(c["pre"]["dtable"].shape), dpad=dpad,
                intact=_intact((obuf, gbuf, tbuf, pbuf)))


@pytest.mark.parametrize("case", WC.CASES, ids=lambda c: c["id"])
def test_fp32_kernels_against_float64(capi, case):
    """uenc_window_attn_f32_{fwd,bwd} on the same (bf16-valued) inputs as fp32 tensors: one r64 serves both.  dtable and dpad start from
    zero here: these kernels add every (query, key) pair to the table gradient with an atomic of its own, thousands per entry."""
    c = _case(case)
    r = _run32(capi, case, c)
    figs = {}
    for n in WC.OUTPUTS:
        r64, A = c["r64"][n], c["A"][n]
        assert r[n].shape == r64.shape and r[n].dtype == F32
        err = (r[n].double() - r64).abs()
        figs[n] = dict(e_kernel=float(err.max()), worst_share_of_bar=float((err / WC.bar32(n, r64, A)).max()), gamma=WC.GAMMA[n],
                       r64_abs_max=float(r64.abs().max()))
        print(f"wattn_f32/{case['id']}/{n}", figs[n])
        record_parity(f"wattn_f32/{case['id']}/{n}", **figs[n])
    for n in WC.OUTPUTS:
        assert figs[n]["worst_share_of_bar"] <= 1.0, (case["id"], n, figs[n])
    assert r["intact"], case["id"]
    if case["ws"] == 1:
        assert _same_bits(r["out"], c["g"]["qkv"][..., 2 * 32 * case["nH"]:].float()), case["id"]


def test_fp32_backward_accumulates(capi):
    """Two backward calls into the same dtable / dpad: twice the gradient, inside twice the bar."""
    case = WC.BY_ID["d-ws5"]
    c = _case(case)
    r = _run32(capi, case, c, twice=True)
    for n in ("dtable", "dpad"):
        r64, A = c["r64"][n], c["A"][n]
        assert float(((r[n].double() - 2.0 * r64).abs() / (2.0 * WC.bar32(n, r64, A))).max()) <= 1.0, n
        assert float(r64.abs().max()) > 0.1
    assert r["intact"]


# ---- argument checks: UENC_EINVAL, and nothing launched --------------------------------------------------------------------------------
def _call(capi, B=1, H=5, W=6, nH=2, ws=4, shift=1, C=None, qkv_off=0, null_dtable=False, alloc_ws=None, which=(1, 1, 1, 1)):
    """A small valid call with the named arguments replaced, made to the entry points selected by `which` (fwd, bwd, f32 fwd, f32 bwd);
    returns their return codes (None: not called) and whether every output still holds its sentinel.  Buffers are sized for `alloc_ws`
    (a window size inside the domain) when ws itself is outside it."""
    lib = capi.lib
    C = 32 * nH if C is None else C
    Cb = max(C, 32 * nH)
    aws = ws if alloc_ws is None else alloc_ws
    L, NP, TT = H * W, 16 * WC.ntiles(aws), (2 * max(aws, ws) - 1) ** 2
    qkv = torch.ones(B * L * 3 * Cb + 64, dtype=BF16, device="cuda")
    qkv32 = torch.ones(B * L * 3 * Cb + 64, dtype=F32, device="cuda")
    bias, bias32 = torch.ones(3 * Cb, dtype=BF16, device="cuda"), torch.ones(3 * Cb, device="cuda")
    table = torch.zeros(TT, nH, device="cuda")
    bq = torch.zeros(nH, NP, NP, device="cuda")
    z = lambda n, dtype: torch.full((n,), SENTINEL, dtype=dtype, device="cuda")
    out, dqkv, lse = z(B * L * Cb, BF16), z(B * L * 3 * Cb, BF16), z(B * L * nH, F32)
    out32, dqkv32 = z(B * L * Cb, F32), z(B * L * 3 * Cb, F32)
    dtab, dpad, dtab32, dpad32 = z(TT * nH, F32), z(3 * Cb, F32), z(TT * nH, F32), z(3 * Cb, F32)
    do, do32 = torch.ones(B * L * Cb, dtype=BF16, device="cuda"), torch.ones(B * L * Cb, device="cuda")
    osave = torch.zeros(B * L * Cb, dtype=BF16, device="cuda")
    dS = z(max(int(lib.uenc_window_attn_bwd_ws_floats(B, H, W, nH, aws)), 1), F32)
    qp = qkv.data_ptr() + qkv_off
    s = capi.stream_ptr()
    calls = (
        lambda: lib.uenc_window_attn_fwd(qp, bias.data_ptr(), bq.data_ptr(), out.data_ptr(), lse.data_ptr(), B, H, W, C, nH, ws, shift, WC.SCALE, s),
        lambda: lib.uenc_window_attn_bwd(qp, bias.data_ptr(), bq.data_ptr(), bq.data_ptr(), osave.data_ptr(), 0, do.data_ptr(), dqkv.data_ptr(),
                                         dS.data_ptr(), 0 if null_dtable else dtab.data_ptr(), dpad.data_ptr(), B, H, W, C, nH, ws, shift,
                                         WC.SCALE, 0, s),
        lambda: lib.uenc_window_attn_f32_fwd(qkv32.data_ptr(), bias32.data_ptr(), table.data_ptr(), out32.data_ptr(), B, H, W, C, nH, ws, shift,
                                             WC.SCALE, s),
        lambda: lib.uenc_window_attn_f32_bwd(qkv32.data_ptr(), bias32.data_ptr(), table.data_ptr(), do32.data_ptr(), dqkv32.data_ptr(),
                                             dtab32.data_ptr(), dpad32.data_ptr(), B, H, W, C, nH, ws, shift, WC.SCALE, s))
    rc = tuple(f() if on else None for f, on in zip(calls, which))
    torch.cuda.synchronize()
    return rc, all(bool((x == SENTINEL).all()) for x in (out, dqkv, lse, dS, dtab, dpad, out32, dqkv32, dtab32, dpad32))


# (why, arguments, the entry points the argument concerns and that must refuse it: fwd, bwd, f32 fwd, f32 bwd)
REJECTS = [
    ("ws 0", dict(ws=0, shift=0, alloc_ws=4), (1, 1, 1, 1)),
    ("ws 13", dict(ws=13, shift=6, alloc_ws=12), (1, 1, 1, 1)),
    ("shift == ws", dict(shift=4), (1, 1, 1, 1)),
    ("C != 32 nH", dict(C=96), (1, 1, 1, 1)),
    ("qkv off 16-byte alignment", dict(qkv_off=8), (1, 1, 0, 0)),
    ("NULL dtable", dict(null_dtable=True), (0, 1, 0, 0)),
]


@pytest.mark.parametrize("why,bad,which", REJECTS, ids=[w for w, _, _ in REJECTS])
def test_arguments_are_refused(capi, why, bad, which):
    """The call itself is valid; with the one thing changed every entry point it concerns returns UENC_EINVAL before any launch: all
    outputs keep the sentinel."""
    rc, untouched = _call(capi, which=which)
    assert rc == tuple(0 if on else None for on in which) and not untouched
    rc, untouched = _call(capi, which=which, **bad)
    assert rc == tuple(EINVAL if on else None for on in which) and untouched, why
