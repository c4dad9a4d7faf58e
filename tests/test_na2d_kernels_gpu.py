"""The neighbourhood-attention kernels of csrc/na2d_mfma.hip (K <= 7) and csrc/na2d.hip (K >= 9) through `uenc_na2d_fwd` / `uenc_na2d_bwd`
themselves, and their fp32 twins of csrc/exact.hip through `uenc_na2d_f32_{fwd,bwd}`, element by element against the float64 references
of tests/na2d_cases.py -- at the shapes where the planner gives a workgroup several tiles (nt = 2, 3, 8: the register prefetch, a !ok
tile inside a walk, the clipped last chunk, the drpb carry and its flush), at the largest per-key LDS image, the full 20 x 28 VALU
halo, NULL rpb / drpb / lse.  NATTEN itself is absent: r64 restates its published definition (tests/na2d_cases.py).

The C entry points are called directly, so out, lse, delta_ws and every buffer's size are the test's own.

Bars (tests/na2d_cases.py has the derivation; kappa = 2 RHO_EMU[route] and gamma = 8 RHO32 come from CPU emulations, never from a kernel):
  out, dqkv (bf16): every element |kernel - r64| <= 2^-8 |r64| + kappa 2^-9 A + floor,  floor = 8 2^-24 max |r64| + 2^-126
  drpb (fp32)     : every element |kernel - (prefill + r64)| <= kappa 2^-9 A + floor + n 2^-24 (|prefill| + A): ACCUMULATED into a random
                    non-zero prefill, one float atomic per workgroup and bin (n = chunks d^2 B on the MFMA route, tiles d^2 B on the VALU one)
  lse (fp32)      : max |kernel - r64| <= max(4 e_ref, 8 2^-24 max |r64|), e_ref the error of the same log-sum-exp composed in fp32 torch
  fp32 twins      : every element |kernel - r64| <= gamma 2^-24 A + floor (their drpb starts from zero: one LDS atomic per pair)
  exact           : out, lse, dqkv between two calls (no atomics touch them); out between lse == NULL and lse given; dqkv between
                    drpb == NULL and drpb given; out, lse, dqkv between rpb == NULL and an all-zero rpb; every image of a B = 2 case
                    against the image run alone at B = 1 (in the nt* cases B = 1 halves the tile count: another nt, another chunking),
                    with drpb of the batch equal to the sum of the single runs within the atomic-sum term of its bar; kvmax7 before and
                    after smaller launches (the per-key kernel's dynamic-LDS attribute grows between launches of one instantiation);
                    64 sentinel elements behind out, lse, dqkv, drpb and delta_ws (exactly B nH H W floats).
The backward consumes the kernel's own out and lse, as production does.  No element is excused anywhere.  Each case prints and records
the worst share of the bar and kappa (gamma) per output (`record_parity("na2d/<id>")`, `record_parity("na2d_f32/<id>")`, written where
UENC_PARITY_OUT points) before anything is asserted.  The restated planner is held against `uenc_na2d_tiles_per_group` in every case.

Not run: the K <= 7 instantiations of the VALU kernels, reached only when H W 3C >= 2^31 (tests/na2d_cases.py).
"""
import pytest
import torch

import na2d_cases as NC
from conftest import record_parity

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = -7.0                      # exact in bf16 and fp32
GUARD = 64                           # sentinel elements behind every buffer a kernel writes


@pytest.fixture(scope="module")
def capi():
    from uenc import capi
    return capi


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _CASE.clear()


_CASE = {}


def _case(case):
    """Inputs on the GPU, r64 / A (float64, computed on the GPU), emu32's lse (fp32 torch on the CPU) and the drpb prefill of one case:
    built once per module and left unchanged."""
    if case["id"] not in _CASE:
        t = NC.inputs(case)
        g = {n: (None if a is None else a.cuda()) for n, a in t.items()}
        r64 = NC.reference(g, case)
        _, A = NC.neigh(g, case)
        gen = torch.Generator().manual_seed(case["seed"] + 5)
        _CASE[case["id"]] = dict(g=g, r64=r64, A=A, lse32=NC.reference(t, case, F32, grads=False)["lse"].cuda(),
                                 pre=torch.randn(r64["drpb"].shape, generator=gen).cuda(), runs={})
    return _CASE[case["id"]]


def _guarded(n, dtype, fill=SENTINEL):
    """(buffer, view): n elements followed by GUARD sentinels."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    buf[:n] = fill
    return buf, buf[:n]


def _intact(bufs):
    return all(bool((b[-GUARD:] == SENTINEL).all()) for b in bufs)


def _ptr(a):
    return 0 if a is None else a.data_ptr()


def _run(capi, case, c, with_lse=True, with_drpb=True, rpb="own", image=None, backward=True):
    """One forward and (backward = True) one backward on the case's inputs, or on image `image` of them alone at B = 1.  rpb: "own" (the
    case's, NULL where it has none) or "zero" (an all-zero table).  Returns the outputs (views) and whether every sentinel survived."""
    lib = capi.lib
    _, H, W, nH, K, d = NC.dims(case)
    B = case["B"] if image is None else 1
    qkv, dout = (c["g"][n] if image is None else c["g"][n][image:image + 1].contiguous() for n in ("qkv", "dout"))
    rp = torch.zeros(nH, 2 * K - 1, 2 * K - 1, device="cuda") if rpb == "zero" else c["g"]["rpb"]
    obuf, out = _guarded(B * H * W * nH * 32, BF16)
    lbuf, lse = _guarded(B * nH * H * W, F32)
    capi.check(lib.uenc_na2d_fwd(qkv.data_ptr(), _ptr(rp), out.data_ptr(), lse.data_ptr() if with_lse else 0, B, H, W, nH, K, d, NC.SCALE,
                                 capi.stream_ptr()), "na2d_fwd")
    r = dict(out=out.view(B, H, W, nH, 32), lse=lse.view(B, nH, H, W))
    bufs = [obuf, lbuf]
    if backward:
        assert with_lse
        gbuf, dqkv = _guarded(B * H * W * 3 * nH * 32, BF16)
        tbuf, drpb = _guarded(c["pre"].numel(), F32)
        wbuf, delta = _guarded(B * nH * H * W, F32)                     # delta_ws: exactly B nH H W floats
        drpb.copy_(c["pre"].reshape(-1))
        capi.check(lib.uenc_na2d_bwd(qkv.data_ptr(), _ptr(rp), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(),
                                     drpb.data_ptr() if with_drpb else 0, delta.data_ptr(), B, H, W, nH, K, d, NC.SCALE, capi.stream_ptr()), "na2d_bwd")
        r.update(dqkv=dqkv.view(B, H, W, 3, nH, 32), drpb=drpb.view(c["pre"].shape))
        bufs += [gbuf, tbuf, wbuf]
    torch.cuda.synchronize()
    r["intact"] = _intact(bufs) and (with_lse or bool((lse == SENTINEL).all())) and (not backward or with_drpb or torch.equal(r["drpb"], c["pre"]))
    return r


def _bits(a):
    return a.contiguous().view(torch.int16 if a.dtype == BF16 else torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _shares(case, c, r):
    """Worst share of the bar and kappa per output, and the lse figures, of one run."""
    rt, figs = NC.route(case), {}
    for n in NC.OUTPUTS:
        r64, A, kappa = c["r64"][n], c["A"][n], NC.KAPPA[NC.route(case)][n]
        assert r[n].shape == r64.shape and r[n].dtype == (BF16 if n in NC.BF16_OUTPUTS else F32), (case["id"], n)
        bar, want = NC.bar(n, r64, A, kappa), r64
        if n == "drpb":
            pre = c["pre"].double()
            want, bar = pre + r64, bar + NC.drpb_adds(case) * NC.U24 * (pre.abs() + A)
        err = (r[n].double() - want).abs()
        figs[n + "_e_kernel"], figs[n + "_worst_share_of_bar"], figs[n + "_kappa"] = float(err.max()), float((err / bar).max()), kappa
    e_ref, lbar = NC.lse_bar(c["r64"]["lse"], c["lse32"])
    figs.update(lse_e_kernel=float((r["lse"].double() - c["r64"]["lse"]).abs().max()), lse_e_ref=e_ref, lse_bar=lbar, route=rt)
    return figs


def _plan_agrees(capi, case):
    _, H, W, nH, K, d = NC.dims(case)
    return all(capi.lib.uenc_na2d_tiles_per_group(B, H, W, nH, K, d) == NC.tiles_per_group(B, H, W, nH, K, d) for B in (case["B"], 1))


def test_per_key_lds_grows_between_launches(capi):
    """The per-key kernel's dynamic LDS is raised by a function attribute kept in a static per instantiation: kvmax7 (the largest image,
    17 x 25 positions) after the smaller min7 and min3 launches and again before them -- the same bits both ways, for all three.  First in
    the module: run alone, the K = 7 attribute really grows between min7 and kvmax7 here."""
    small = [NC.BY_ID["min3"], NC.BY_ID["min7"]]
    big = NC.BY_ID["kvmax7"]
    first = [_run(capi, s, _case(s)) for s in small]
    b1 = _run(capi, big, _case(big))
    b2 = _run(capi, big, _case(big))
    second = [_run(capi, s, _case(s)) for s in small]
    for a, b in zip(first + [b1], second + [b2]):
        assert a["intact"] and b["intact"]
        for n in ("out", "lse", "dqkv"):
            assert _same_bits(a[n], b[n]), n
    assert _shares(big, _case(big), b1)["dqkv_worst_share_of_bar"] <= 1.0


@pytest.mark.parametrize("case", NC.CASES, ids=lambda c: c["id"])
def test_kernels_against_float64(capi, case):
    c = _case(case)
    tag = f"na2d/{case['id']}"
    assert _plan_agrees(capi, case), case["id"]                       # the case still reaches the walk it was written for
    r1 = _run(capi, case, c)
    r2 = _run(capi, case, c)
    r_nolse = _run(capi, case, c, with_lse=False, backward=False)
    r_nodrpb = _run(capi, case, c, with_drpb=False)
    c["runs"]["main"] = r1
    figs = _shares(case, c, r1)
    print(tag, figs)
    record_parity(tag, **figs)
    for n in NC.OUTPUTS:
        assert figs[n + "_worst_share_of_bar"] <= 1.0, (case["id"], n, figs)
    assert figs["lse_e_kernel"] <= figs["lse_bar"], (case["id"], figs)
    # two calls: the same bits wherever nothing is accumulated atomically; NULL lse / NULL drpb change nothing else
    for n in ("out", "lse", "dqkv"):
        assert _same_bits(r1[n], r2[n]), (case["id"], n)
    assert _same_bits(r1["out"], r_nolse["out"]), case["id"]
    assert _same_bits(r1["dqkv"], r_nodrpb["dqkv"]), case["id"]
    if not case["rpb"]:                                               # NULL rpb against an all-zero table
        rz = _run(capi, case, c, rpb="zero")
        assert rz["intact"]
        for n in ("out", "lse", "dqkv"):
            assert _same_bits(r1[n], rz[n]), (case["id"], n)
    assert r1["intact"] and r2["intact"] and r_nolse["intact"] and r_nodrpb["intact"], case["id"]      # nothing written behind any buffer


@pytest.mark.parametrize("cid", [c["id"] for c in NC.CASES if c["B"] == 2])
def test_images_of_a_batch_alone(capi, cid):
    """Each image of a B = 2 case at B = 1: out, lse, dqkv bit for bit per image -- in the nt* cases under another nt and chunking, the
    sharpest check of the tile walk, with no reference in it -- and drpb of the batch = the sum of the single runs within the
    atomic-sum term of its bar."""
    case = NC.BY_ID[cid]
    c = _case(case)
    _, H, W, nH, K, d = NC.dims(case)
    if cid in NC.NT_CASES:
        assert NC.tiles_per_group(1, H, W, nH, K, d) != NC.tiles_per_group(2, H, W, nH, K, d)
    main = c["runs"].get("main") or _run(capi, case, c)
    pre = c["pre"].double()
    total = torch.zeros_like(pre)
    for b in range(2):
        r = _run(capi, case, c, image=b)
        assert r["intact"], (cid, b)
        for n in ("out", "lse", "dqkv"):
            assert _same_bits(r[n][0], main[n][b]), (cid, b, n)
        total += r["drpb"].double() - pre
    err = (main["drpb"].double() - pre - total).abs()
    share = float((err / (NC.drpb_adds(case) * NC.U24 * (pre.abs() + c["A"]["drpb"]) + NC.floor(c["r64"]["drpb"]))).max())
    print(f"na2d/{cid}/batch", dict(drpb_batch_vs_singles_share=share))
    record_parity(f"na2d/{cid}", drpb_batch_vs_singles_share=share)
    assert share <= 1.0, (cid, share)


# ---- the fp32 verification kernels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.F32_CASES, ids=lambda c: c["id"])
def test_fp32_kernels_against_float64(capi, case):
    """uenc_na2d_f32_{fwd,bwd} on the same (bf16-valued) inputs as fp32 tensors: one r64 serves both.  drpb starts from zero here: these
    kernels add every (query, key) pair to an LDS bin with an atomic of its own."""
    lib, c = capi.lib, _case(case)
    B, H, W, nH, K, d = NC.dims(case)
    qkv, dout, rpb = c["g"]["qkv"].float(), c["g"]["dout"].float(), c["g"]["rpb"]
    obuf, out = _guarded(B * H * W * nH * 32, F32)
    lbuf, lse = _guarded(B * nH * H * W, F32)
    capi.check(lib.uenc_na2d_f32_fwd(qkv.data_ptr(), _ptr(rpb), out.data_ptr(), lse.data_ptr(), B, H, W, nH, K, d, NC.SCALE, capi.stream_ptr()),
               "na2d_f32_fwd")
    gbuf, dqkv = _guarded(B * H * W * 3 * nH * 32, F32)
    tbuf, drpb = _guarded(c["pre"].numel(), F32, 0.0)
    capi.check(lib.uenc_na2d_f32_bwd(qkv.data_ptr(), _ptr(rpb), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), dqkv.data_ptr(), drpb.data_ptr(),
                                     B, H, W, nH, K, d, NC.SCALE, capi.stream_ptr()), "na2d_f32_bwd")
    torch.cuda.synchronize()
    r = dict(out=out.view(B, H, W, nH, 32), lse=lse.view(B, nH, H, W), dqkv=dqkv.view(B, H, W, 3, nH, 32), drpb=drpb.view(c["pre"].shape))
    figs = {}
    for n in NC.OUTPUTS:
        r64, A = c["r64"][n], c["A"][n]
        assert r[n].shape == r64.shape and r[n].dtype == F32
        err = (r[n].double() - r64).abs()
        figs[n + "_e_kernel"], figs[n + "_worst_share_of_bar"], figs[n + "_gamma"] = float(err.max()), float((err / NC.bar32(n, r64, A)).max()), NC.GAMMA[n]
    e_ref, lbar = NC.lse_bar(c["r64"]["lse"], c["lse32"])
    figs.update(lse_e_kernel=float((r["lse"].double() - c["r64"]["lse"]).abs().max()), lse_e_ref=e_ref, lse_bar=lbar)
    print(f"na2d_f32/{case['id']}", figs)
    record_parity(f"na2d_f32/{case['id']}", **figs)
    for n in NC.OUTPUTS:
        assert figs[n + "_worst_share_of_bar"] <= 1.0, (case["id"], n, figs)
    assert figs["lse_e_kernel"] <= figs["lse_bar"], (case["id"], figs)
    assert _intact((obuf, lbuf, gbuf, tbuf)), case["id"]
