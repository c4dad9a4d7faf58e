"""The ConvNeXt kernels (csrc/dwconv.hip, the LayerNorm backward they call, `uenc_layer_scale_grads`) and `ops.conv2x2_s2` through their
`uenc.kernels` / `uenc.ops` entry points, element by element against the float64 references of tests/convnext_cases.py, at the shapes
where the kernels' tiling branches (tests/test_convnext_cases_cpu.py computes which branch each case reaches).

Bars.  u = 2^-24; `r64` is the float64 reference, `comp` its absolute-value companion (the same sum over magnitudes).
  closed  : |kernel - r64| <= k * u * comp, element by element, where the operation count gives k:
              y        k = 50            49 fused multiply-adds on top of the bias, (1 + u)^49 - 1 < 50 u
              mean     k = 50 + ceil(C / 32) + 7     y's error, the slab additions, 5 butterfly levels, 1 / C and the product with it
              dw, db   k = 8 + T + 3 + NB + 1        8-pixel chain, T tiles per workgroup, pair + 4 waves, NB partials, the +=  (A, B: 270)
              gw2, gb2 k = 2             one product, one addition;   ggamma  k = ceil(K / 256) + 11
              conv2x2_s2 (fp32 GEMM bound: a sum of n terms in any order)   out k = 4 Cin + 1, dx k = Cout, dw and db k = B Ho Wo + 1
  exact   : dbeta.  dh and the prefill are multiples of 1/64 whose magnitudes sum to less than 2^18, so every partial sum in any order is
            an fp32 number (asserted on the host): the kernels' dbeta equals the reference bit for bit.
  ATen    : rstd, h, dy, dx, dgamma have no closed bound (they pass through 1 / sqrt(var) and the LayerNorm backward).  The same torch
            composition is run in fp32 on the CPU; with e_aten = max |fp32 ATen - r64| over the output the bar is 4 * e_aten for every
            element.  The factor 4 covers the half-wave butterfly and wave sums where ATen sums sequentially.
            dgamma is the one output here that is not reproducible: ln_bwd_kernel and ln_bwd_param_kernel add their block sums with float
            atomics, so its rounding error depends on the order the blocks arrive in.  The longest such sum is case A's (17408 rows into
            8 channels): over eight runs on the same inputs its error lay between 1.3e-4 and 3.2e-4 against the bar of 4.26e-4
            (e_aten 1.07e-4), a share of up to 0.74, the thinnest margin of an order-dependent sum in this file; the dgamma of every
            other case stayed below 0.55 of its bar.  (test_backward_data runs each case four times on the same dh, y and stats: the four
            recorded dgamma figures of a case are that spread.)
  bf16    : h in product mode, and conv2x2_s2's dx where it passes through a bf16 GEMM result: the stored value is the rounding to
            nearest of an fp32 value v that meets the fp32 bar, |kernel - r64| <= halfulp(|r64| + bar) + bar per element, where
            halfulp(a) = 2^(floor(log2 a) - 8) is half a unit in the last place of bf16 at a (8-bit significand), at least that of v.
            A store that truncated would miss this by up to a factor 2 (tests/test_convnext_cases_cpu.py shows it on the reference).
No bar is taken from the kernels' output.  Every figure is printed and recorded (`record_parity("convnext_kernels/...")`) before it is
asserted; profiles/convnext_kernels_parity.json is the copy of one MI355X run.
"""
import pytest
import torch

import convnext_cases as CC
from conftest import record_parity

pytestmark = pytest.mark.gpu

U24 = CC.U24
F32, BF16 = torch.float32, torch.bfloat16
ids = CC.sid


@pytest.fixture(scope="module")
def K():
    import model  # noqa: F401
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _DEV.clear()
    _FWD.clear()


@pytest.fixture()
def mode(K, request, monkeypatch):
    """"f32": the fp32 verification mode; "bf16": product mode (h and the GEMM operands in bf16)."""
    monkeypatch.setattr(K, "EXACT", request.param == "f32")
    return request.param


MODES = pytest.mark.parametrize("mode", ["f32", "bf16"], indirect=True)
_DEV, _FWD = {}, {}


def _dev(shape):
    if shape not in _DEV:
        _DEV[shape] = {k: v.cuda() for k, v in CC.dw_inputs(shape).items()}
    return _DEV[shape]


def _fwd(K, shape):
    """y and stats of the forward kernel, the saved tensors of the backward tests (the same in both modes): computed once per shape."""
    if shape not in _FWD:
        c = _dev(shape)
        y, _, st = K.dwconv7_ln_fwd(c["x"], c["w"], c["b"], c["g"], c["be"], CC.EPS)
        _FWD[shape] = (y, st)
    return _FWD[shape]


def _host(t):
    return t.detach().double().cpu()


def _closed(tag, got, r64, k, comp):
    assert got.dtype == F32 and got.shape == r64.shape, (tag, got.dtype, got.shape, r64.shape)
    err = (_host(got) - r64).abs()
    bar = k * U24 * comp
    figs = dict(kind="closed", k=k, e_kernel=float(err.max()), worst_share_of_bar=float((err / bar.clamp_min(1e-300)).max()))
    print(tag, figs)
    record_parity(tag, **figs)
    assert bool((err <= bar).all()), (tag, figs)


def _aten_bar(r64, a32):
    e_ref = float((a32.double() - r64).abs().max())
    return e_ref, 4.0 * e_ref


def _aten(tag, got, r64, a32):
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    err = (_host(got) - r64).abs()
    e_ref, bar = _aten_bar(r64, a32)
    figs = dict(kind="aten", e_kernel=float(err.max()), e_aten_fp32=e_ref, bar=bar)
    if got.dtype == BF16:
        figs["worst_share_of_bf16_allowance"] = float((err / CC.bf16_allowance(r64, bar)).max())
    print(tag, figs)
    record_parity(tag, **figs)
    if got.dtype == BF16:
        assert figs["worst_share_of_bf16_allowance"] <= 1.0, (tag, figs)
    else:
        assert got.dtype == F32 and figs["e_kernel"] <= bar, (tag, figs)


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("shape", CC.DW_CASES, ids=ids)
def test_forward(K, shape, mode):
    B, H, W, C = shape
    c, r64, a32 = _dev(shape), CC.dw_reference(shape), CC.dw_reference(shape, F32)
    tag = f"convnext_kernels/fwd/{ids(shape)}/{mode}"
    y, h, st = K.dwconv7_ln_fwd(c["x"], c["w"], c["b"], c["g"], c["be"], CC.EPS)
    y2, h2, st2 = K.dwconv7_ln_fwd(c["x"], c["w"], c["b"], c["g"], c["be"], CC.EPS)
    assert h.dtype == (F32 if mode == "f32" else BF16) and st.shape == (B * H * W, 2) and st.dtype == F32
    assert torch.equal(y, y2) and torch.equal(h, h2) and torch.equal(st, st2)                 # no atomics: the same bits
    _closed(tag + "/y", y, r64["y"], CC.k_y(), r64["abs_y"])
    _closed(tag + "/mean", st[:, 0].view(B, H, W), r64["mean"], CC.k_mean(C), r64["abs_y"].mean(-1))
    _aten(tag + "/rstd", st[:, 1].view(B, H, W), r64["rstd"], a32["rstd"])
    _aten(tag + "/h", h, r64["h"], a32["h"])


# ---- backward data ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_dout", [True, False], ids=["dout", "nodout"])
@pytest.mark.parametrize("dh_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", CC.DW_CASES, ids=ids)
def test_backward_data(K, shape, dh_dtype, with_dout):
    c, r64, a32 = _dev(shape), CC.dw_reference(shape), CC.dw_reference(shape, F32)
    tag = f"convnext_kernels/bwd_data/{ids(shape)}/dh_{dh_dtype}/{'dout' if with_dout else 'nodout'}"
    y, st = _fwd(K, shape)
    dh = c["dh"] if dh_dtype == "f32" else c["dh"].bfloat16()
    assert torch.equal(dh.float(), c["dh"])                                                    # the reference's dh is the kernel's
    dgamma, dbeta = c["pre_dgamma"].clone(), c["pre_dbeta"].clone()
    dx, dy = K.dwconv7_ln_bwd_data(dh, y, st, c["g"], c["w"], dout=c["dout"] if with_dout else None, dgamma=dgamma, dbeta=dbeta)
    torch.cuda.synchronize()
    key = "dx" if with_dout else "dx0"
    _aten(tag + "/dy", dy, r64["dy"], a32["dy"])
    _aten(tag + "/dx", dx, r64[key], a32[key])
    _aten(tag + "/dgamma", dgamma, r64["dgamma"], a32["dgamma"])
    assert torch.equal(_host(dbeta), r64["dbeta"]), (tag, float((_host(dbeta) - r64["dbeta"]).abs().max()))


def test_backward_data_three_ways_with_stored_partials(K):
    """Case F: the LayerNorm backward stores its 400 block partials.  Immediate (ln_bwd_param_kernel sums them), deferred
    (SmallReductions -> uenc_ln_param_grouped at the flush) and without parameter gradients."""
    shape = CC.CASE_F
    c, r64, a32 = _dev(shape), CC.dw_reference(shape), CC.dw_reference(shape, F32)
    tag = "convnext_kernels/bwd_data_three_ways/" + ids(shape)
    assert int(K.lib.uenc_layernorm_bwd_blocks(shape[0] * shape[1] * shape[2], shape[3])) == 400
    y, st = _fwd(K, shape)
    dh = c["dh"].bfloat16()
    run = lambda **kw: K.dwconv7_ln_bwd_data(dh, y, st, c["g"], c["w"], dout=c["dout"], **kw)
    dg_i, db_i = c["pre_dgamma"].clone(), c["pre_dbeta"].clone()
    dx_i, dy_i = run(dgamma=dg_i, dbeta=db_i)
    q = K.SmallReductions()
    dg_d, db_d = c["pre_dgamma"].clone(), c["pre_dbeta"].clone()
    dx_d, dy_d = run(dgamma=dg_d, dbeta=db_d, defer=q)
    torch.cuda.synchronize()
    assert bool(q) and len(q.ln) == 1 and q.ln[0][3] == 400
    assert torch.equal(dg_d, c["pre_dgamma"]) and torch.equal(db_d, c["pre_dbeta"])           # parked: untouched before the flush
    q.flush()
    torch.cuda.synchronize()
    assert not q
    dx_n, dy_n = run(dgamma=None, dbeta=None)
    for dx, dy in ((dx_d, dy_d), (dx_n, dy_n)):                                                # dx, dy do not depend on how dgamma is summed
        assert torch.equal(dx, dx_i) and torch.equal(dy, dy_i)
    _aten(tag + "/dx", dx_i, r64["dx"], a32["dx"])
    _aten(tag + "/immediate/dgamma", dg_i, r64["dgamma"], a32["dgamma"])
    _aten(tag + "/deferred/dgamma", dg_d, r64["dgamma"], a32["dgamma"])
    bar = _aten_bar(r64["dgamma"], a32["dgamma"])[1]
    gap = float((dg_i.double() - dg_d.double()).abs().max())
    record_parity(tag + "/immediate_vs_deferred", gap=gap, bar=bar)
    assert gap <= bar
    assert torch.equal(_host(db_i), r64["dbeta"]) and torch.equal(_host(db_d), r64["dbeta"])


# ---- backward weight ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CC.DW_CASES, ids=ids)
def test_backward_weight(K, shape):
    c, ref = _dev(shape), CC.wgrad_reference(shape)
    tag = "convnext_kernels/bwd_weight/" + ids(shape)
    dy = CC.wgrad_operand(shape).cuda()
    x0, dy0 = c["x"].clone(), dy.clone()
    dw, db = c["pre_dw"].clone(), c["pre_db"].clone()
    K.dwconv7_bwd_weight(dy, c["x"], dw, db)
    dw2, db2 = c["pre_dw"].clone(), c["pre_db"].clone()
    K.dwconv7_bwd_weight(dy, c["x"], dw2, db2)
    dw3 = c["pre_dw"].clone()
    K.dwconv7_bwd_weight(dy, c["x"], dw3, None)
    torch.cuda.synchronize()
    assert torch.equal(dw, dw2) and torch.equal(db, db2)                                       # fixed summation order: the same bits
    assert torch.equal(dw, dw3)                                                                # db = None: dw as before ...
    assert torch.equal(c["x"], x0) and torch.equal(dy, dy0)                                    # ... and the operands as they were
    k = CC.k_wgrad(shape)
    _closed(tag + "/dw", dw, ref["dw"], k, ref["abs_dw"])
    _closed(tag + "/db", db, ref["db"], k, ref["abs_db"])


# ---- layer scale --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(CC.LS_PATTERNS), ids=str)
@pytest.mark.parametrize("NK", CC.LS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layer_scale_grads(K, NK, pattern):
    N, Kd = NK
    pat = CC.LS_PATTERNS[pattern]
    t = CC.ls_inputs(N, Kd)
    ref = CC.ls_reference(t, pat)
    c = {k: v.cuda() for k, v in t.items()}
    arg = lambda k: c[k] if pat[k] else None
    K.layer_scale_grads(c["dw2p"], arg("db2p"), c["w2"], arg("b2"), c["gamma"], arg("gw2"), arg("gb2"), arg("ggamma"))
    torch.cuda.synchronize()
    tag = f"convnext_kernels/layer_scale/{N}x{Kd}/{pattern}"
    for k, kk in (("gw2", 2), ("gb2", 2), ("ggamma", CC.k_layer_scale(Kd))):
        if pat[k]:
            _closed(tag + "/" + k, c[k], ref[k], kk, ref["abs_" + k])
    for k in ("dw2p", "db2p", "w2", "b2", "gamma"):
        assert torch.equal(c[k].cpu(), t[k])


# ---- conv2x2_s2 ---------------------------------------------------------------------------------------------------------------------------
def _bounded(tag, got, r64, k, comp, through_bf16):
    """Closed GEMM bound; through_bf16: the value was stored as bf16 on its way (its half-ulp of bf16 on top, element by element)."""
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    err = (_host(got) - r64).abs()
    bar = k * U24 * comp
    if through_bf16:
        bar = CC.bf16_allowance(r64, bar)
    figs = dict(kind="closed", k=k, through_bf16=through_bf16, e_kernel=float(err.max()),
                worst_share_of_bar=float((err / bar.clamp_min(1e-300)).max()))
    print(tag, figs)
    record_parity(tag, **figs)
    assert bool((err <= bar).all()), (tag, figs)


@pytest.mark.parametrize("arith", ["f32", "bf16"])
@pytest.mark.parametrize("case", CC.C2_CASES, ids=lambda c: ids(c[:5]) + c[5])
def test_conv2x2_s2(K, case, arith):
    from uenc import ops
    B, H, W, Ci, Co, in_dtype = case
    Ho, Wo = H // 2, W // 2
    t = CC.c2_inputs(case)
    ref = CC.c2_reference(t, round_weight=(arith == "bf16"))
    tag = f"convnext_kernels/conv2x2_s2/{ids(case[:5])}{in_dtype}/{arith}"
    ops.set_exact(arith == "f32")
    try:
        x = t["x"].cuda().requires_grad_(True)
        w, b = torch.nn.Parameter(t["w"].cuda()), torch.nn.Parameter(t["b"].cuda())
        out = ops.conv2x2_s2(x, w, b)
        out.backward(t["dy"].cuda())
        ops.flush_wgrads()
        torch.cuda.synchronize()
    finally:
        ops.set_exact(False)
    assert out.dtype == F32 and out.shape == (B, Ho, Wo, Co) and x.grad.dtype == x.dtype and x.grad.shape == x.shape
    if H % 2:
        assert float(x.grad[:, H - 1].float().abs().max()) == 0.0                              # the dropped row: exactly zero
    if W % 2:
        assert float(x.grad[:, :, W - 1].float().abs().max()) == 0.0
    M = B * Ho * Wo
    _bounded(tag + "/out", out, ref["out"], 4 * Ci + 1, ref["abs_out"], False)
    _bounded(tag + "/dx", x.grad, ref["dx"], Co, ref["abs_dx"], arith == "bf16" or in_dtype == "bf16")
    _bounded(tag + "/dw", w.grad, ref["dw"], M + 1, ref["abs_dw"], False)
    _bounded(tag + "/db", b.grad, ref["db"], M + 1, ref["abs_db"], False)


# ---- accept / reject ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", CC.DW_STATUS, ids=lambda r: r[0])
def test_depthwise_entry_point_status(K, row):
    from uenc import capi
    rc, outs = CC.dw_status_call(row, "cuda", capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == row[4]
    if rc == CC.EINVAL:
        assert CC.untouched(outs)
    elif row[1] != "bwd_weight":
        assert all(bool((t != CC.SENTINEL).all()) for k, t in outs.items() if k in ("y", "stats", "dy", "dx"))


@pytest.mark.parametrize("row", CC.LS_STATUS, ids=lambda r: r[0])
def test_layer_scale_entry_point_status(K, row):
    from uenc import capi
    rc, outs = CC.ls_status_call(row, "cuda", capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == row[3]
    if rc == CC.EINVAL:
        assert CC.untouched(outs)


def test_wrappers_raise_on_a_refusal(K):
    from uenc import capi
    x = torch.zeros(1, 1, 1, 6152, device="cuda")
    w, v = torch.zeros(6152, 1, 7, 7, device="cuda"), torch.zeros(6152, device="cuda")
    with pytest.raises(capi.UencError, match="nothing was launched"):
        K.dwconv7_ln_fwd(x, w, v, v, v)
    with pytest.raises(capi.UencError, match="nothing was launched"):
        K.dwconv7_bwd_weight(x, x, w, v)
    with pytest.raises(ValueError):
        K.dwconv7_ln_fwd(torch.zeros(1, 2, 2, 12, device="cuda"), torch.zeros(12, 1, 7, 7, device="cuda"), None, v[:12], v[:12])
