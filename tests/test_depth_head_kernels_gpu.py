"""The three kernel pairs of csrc/depth_head.hip through their direct `uenc.kernels` entry points, element by element against the float64
references of tests/depth_head_cases.py.

Bars (those of tests/test_fpn_kernels_gpu.py).  `r64` is the float64 CPU reference, `t32` the same torch composition in fp32 on the GPU,
`e_ref = max |t32 - r64|`.
  fp32 output : max |kernel - r64| <= max(4 * e_ref, 8 * 2^-24 * max |r64|).
  bf16 output : every element within 2^-8 * |r64| plus the fp32 bar above.
No element is excused.  Every backward runs twice and must give the same bits (gathers in a fixed order, no float atomics).  Each case
prints and records e_kernel, e_ref and their ratio (`record_parity("depth_head/...")`)."""
import pytest
import torch

import depth_head_cases as DC
from conftest import record_parity

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(autouse=True)
def _product_mode(K, monkeypatch):
    monkeypatch.setattr(K, "EXACT", False)


def _check(tag, got, r64, t32):
    """One output against the bar of its dtype; the figures are printed and recorded before anything is asserted."""
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    r64 = r64.cuda()
    err = (got.double() - r64).abs()
    e_ref = float((t32.double() - r64).abs().max())
    bar = max(4.0 * e_ref, 8.0 * U24 * float(r64.abs().max()))
    e_k = float(err.max())
    figs = dict(e_kernel=e_k, e_ref=e_ref, ratio=(e_k / e_ref if e_ref > 0 else None), bar=bar)
    if got.dtype == BF16:
        figs["worst_share_of_allowance"] = float((err / (2.0 ** -8 * r64.abs() + bar)).max())
    print(tag, figs)
    record_parity(tag, **figs)
    assert bool(torch.isfinite(got.float()).all()), tag
    if got.dtype == BF16:
        assert figs["worst_share_of_allowance"] <= 1.0, (tag, figs)
    else:
        assert got.dtype == F32 and e_k <= bar, (tag, figs)


def _dev(t, variant, keep_f32=()):
    dt = F32 if variant == "f32" else BF16
    return {k: (v.cuda() if k in keep_f32 else v.to(dt).cuda()) for k, v in t.items()}


@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("shape", DC.UPSAMPLE_SHAPES, ids=DC.shape_id)
def test_upsample2x_ac(K, shape, variant):
    t = DC.upsample_inputs(shape, variant)
    r64, t32 = DC.upsample_reference(t), DC.upsample_reference(t, F32, "cuda")
    c = _dev(t, variant)
    tag = f"depth_head/upsample/{DC.shape_id(shape)}/{variant}"
    y, dx = K.upsample2x_ac_fwd(c["x"]), K.upsample2x_ac_bwd(c["dy"])
    assert y.dtype == c["x"].dtype and dx.dtype == c["dy"].dtype
    assert torch.equal(y, K.upsample2x_ac_fwd(c["x"])) and torch.equal(dx, K.upsample2x_ac_bwd(c["dy"]))
    _check(tag + "/y", y, r64["y"], t32["y"])
    _check(tag + "/dx", dx, r64["dx"], t32["dx"])
    if variant == "bf16":                                   # bf16 operands, fp32 results: the fp32 bar alone
        _check(tag + "/y_f32out", K.upsample2x_ac_fwd(c["x"], out_dtype=F32), r64["y"], t32["y"])
        _check(tag + "/dx_f32out", K.upsample2x_ac_bwd(c["dy"], out_dtype=F32), r64["dx"], t32["dx"])


@pytest.mark.parametrize("second", (False, True), ids=("one_grad", "two_grads"))
@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("case", DC.gate_cases(), ids=lambda c: c["id"])
def test_softmax_gate(K, case, variant, second):
    t = DC.gate_inputs(case, variant)
    r64, t32 = DC.gate_reference(t, second), DC.gate_reference(t, second, F32, "cuda")
    c = _dev(t, variant)
    dt = F32 if variant == "f32" else BF16
    tag = f"depth_head/gate/{case['id']}/{variant}/{'two' if second else 'one'}"
    res, g = K.softmax_gate_fwd(c["a"], c["b"], c["z"], out_dtype=dt)
    res32, _ = K.softmax_gate_fwd(c["a"], c["b"], c["z"], out_dtype=F32)
    args = (c["dg"], c["dres"] if second else None, c["z"], res32)
    d_res, d_z = K.softmax_gate_bwd(*args, out_dtype=dt)
    d_res2, d_z2 = K.softmax_gate_bwd(*args, out_dtype=dt)
    assert torch.equal(d_res, d_res2) and torch.equal(d_z, d_z2)
    _check(tag + "/res", res, r64["res"], t32["res"])
    _check(tag + "/g", g, r64["g"], t32["g"])
    _check(tag + "/d_res", d_res, r64["d_res"], t32["d_res"])
    _check(tag + "/d_z", d_z, r64["d_z"], t32["d_z"])


@pytest.mark.parametrize("second", (False, True), ids=("one_grad", "two_grads"))
@pytest.mark.parametrize("case", DC.gate_cases(), ids=lambda c: c["id"])
def test_softmax_gate_backward_reads_a_bf16_res(K, case, second):
    """The backward with the forward's own bf16 `res` (the operand path res_dtype = bf16), against the float64 reference on the exact sum.

    Bound.  The stored res_k is the exact a_k + b_k rounded to nearest bf16 (8 significant bits): res_k (1 + e_k), |e_k| <= 2^-8, the
    same unit roundoff the bf16-output allowance of `_check` uses.  d_res does not read res.  In d_z_k = att_k (q_k - sum_j q_j att_j),
    q = dg * res, the rounding moves q_j by at most 2^-8 |q_j|, hence d_z_k by at most x_k = 2^-8 att_k (|q_k| + sum_j |q_j| att_j).  The
    output rounding then acts on the moved value, 2^-8 (|d_z_k| + x_k).  So x_k (1 + 2^-8), evaluated in float64, is added to the
    allowance of `_check`."""
    t = DC.gate_inputs(case, "bf16")
    r64, t32 = DC.gate_reference(t, second), DC.gate_reference(t, second, F32, "cuda")
    c = _dev(t, "bf16")
    tag = f"depth_head/gate_bf16_res/{case['id']}/{'two' if second else 'one'}"
    res16, _ = K.softmax_gate_fwd(c["a"], c["b"], c["z"], out_dtype=BF16)
    assert res16.dtype == BF16
    args = (c["dg"], c["dres"] if second else None, c["z"], res16)
    d_res, d_z = K.softmax_gate_bwd(*args, out_dtype=BF16)
    d_res2, d_z2 = K.softmax_gate_bwd(*args, out_dtype=BF16)
    assert torch.equal(d_res, d_res2) and torch.equal(d_z, d_z2)
    _check(tag + "/d_res", d_res, r64["d_res"], t32["d_res"])
    att = torch.softmax(t["z"].double(), -1)
    q = (t["dg"].double() * r64["res"]).abs()
    extra = ((1.0 + 2.0 ** -8) * 2.0 ** -8 * att * (q + (q * att).sum(-1, keepdim=True))).cuda()
    want = r64["d_z"].cuda()
    err = (d_z.double() - want).abs()
    e_ref = float((t32["d_z"].double() - want).abs().max())
    bar = max(4.0 * e_ref, 8.0 * U24 * float(want.abs().max()))
    share = float((err / (2.0 ** -8 * want.abs() + bar + extra)).max())
    figs = dict(e_kernel=float(err.max()), e_ref=e_ref, bar=bar, worst_share_of_allowance=share)
    print(tag + "/d_z", figs)
    record_parity(tag + "/d_z", **figs)
    assert bool(torch.isfinite(d_z.float()).all()) and share <= 1.0, (tag, figs)


@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("case", DC.head_cases(), ids=lambda c: c["id"])
def test_soft_att_depth(K, case, variant):
    t = DC.head_inputs(case, variant)
    r64, t32 = DC.head_reference(t), DC.head_reference(t, F32, "cuda")
    c = _dev(t, variant, keep_f32=("grid", "ddisp"))
    dt = F32 if variant == "f32" else BF16
    tag = f"depth_head/head/{case['id']}/{variant}"
    disp = K.soft_att_depth_fwd(c["z"], c["grid"])
    dz = K.soft_att_depth_bwd(c["ddisp"], c["z"], c["grid"], out_dtype=dt)
    assert disp.dtype == F32 and torch.equal(dz, K.soft_att_depth_bwd(c["ddisp"], c["z"], c["grid"], out_dtype=dt))
    _check(tag + "/disp", disp, r64["disp"], t32["disp"])
    _check(tag + "/dz", dz, r64["dz"], t32["dz"])


def test_wrappers_refuse_what_the_library_refuses(K):
    from uenc import capi
    refused = lambda: pytest.raises(capi.UencError, match="nothing was launched")
    with refused():
        K.upsample2x_ac_fwd(torch.zeros(1, 2, 2, 12, device="cuda"))
    with refused():
        K.softmax_gate_fwd(*(torch.zeros(4, 12, device="cuda") for _ in range(3)))
    with refused():
        K.soft_att_depth_fwd(torch.zeros(4, 72, device="cuda"), torch.zeros(72, device="cuda"))
