"""The seven kernels of csrc/fpn.hip through their direct `uenc.kernels` entry points, element by element against the float64 references
of tests/fpn_cases.py.

Bars.  `r64` is the float64 CPU reference, `t32` the same torch composition in fp32 on the GPU, `e_ref = max |t32 - r64|`.
  fp32 output : max |kernel - r64| <= max(4 * e_ref, 8 * 2^-24 * max |r64|).  The bar is the reference composition's own fp32 error (kernel
                and composition differ only in summation order and operation grouping, hence a small factor), with a floor of eight
                fp32 roundings of the largest value for outputs the composition happens to hit exactly.
  bf16 output : every element within 2^-8 * |r64| (round to nearest of an 8-bit significand) plus the fp32 bar above.
  exact       : im2col, col2im (against the sum in the kernel's own order), the identity-size adjoint, and y / dx between two calls.
No element is excused anywhere: the ReLU cases keep |pre-activation| >= 1e-4 (tests/test_fpn_cases_cpu.py), far above fp32 rounding.
Each case prints and records e_kernel, e_ref and their ratio (`record_parity("fpn/...")`, written where UENC_PARITY_OUT points).
"""
import math

import pytest
import torch

import fpn_cases as FC
from conftest import record_parity

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def K():
    from uenc import kernels
    return kernels


@pytest.fixture(scope="module", autouse=True)
def _drop_cached_cases():
    yield
    _GN.clear()


@pytest.fixture(autouse=True)
def _product_mode(K, monkeypatch):
    monkeypatch.setattr(K, "EXACT", False)          # the bf16 outputs asked for below stay bf16


def _bar32(r64, t32):
    e_ref = float((t32.double() - r64).abs().max())
    return e_ref, max(4.0 * e_ref, 8.0 * U24 * float(r64.abs().max()))


def _check(tag, got, r64, t32):
    """One output against the bar of its dtype; the figures are printed and recorded before anything is asserted."""
    assert got.shape == r64.shape, (tag, got.shape, r64.shape)
    err = (got.double() - r64).abs()
    e_ref, bar = _bar32(r64, t32)
    e_k = float(err.max())
    figs = dict(e_kernel=e_k, e_ref=e_ref, ratio=(e_k / e_ref if e_ref > 0 else None), bar=bar)
    if got.dtype == BF16:
        figs["worst_share_of_allowance"] = float((err / (2.0 ** -8 * r64.abs() + bar)).max())
    print(tag, figs)
    record_parity(tag, **figs)
    if got.dtype == BF16:
        assert figs["worst_share_of_allowance"] <= 1.0, (tag, figs)
    else:
        assert got.dtype == F32 and e_k <= bar, (tag, figs)


# ---- 3.1 GroupNorm forward and backward -------------------------------------------------------------------------------------------
GN_CASES = FC.gn_cases()
_GN = {}


def _gn(case, variant):
    """Inputs on the GPU, r64 (computed on the CPU, kept on the GPU as float64) and t32 of one case: built once per module."""
    key = (case["id"], variant)
    if key not in _GN:
        t = FC.gn_inputs(case, variant)
        r64 = {k: v.cuda() for k, v in FC.gn_reference(t, case).items()}
        t32 = {k: v.detach() for k, v in FC.gn_reference(t, case, torch.float32, "cuda").items()}
        _GN[key] = ({k: v.cuda() for k, v in t.items()}, r64, t32)
    return _GN[key]


def _gn_fwd(K, case, variant, c):
    return K.groupnorm_tokens_fwd(c["x"], c["gamma"], c["beta"], case["G"], FC.EPS, relu=case["relu"], add_src=c.get("src"),
                                  add_hw=case["merge"][1] if case["merge"] is not None else None,
                                  out_dtype=F32 if variant == "f32" else BF16)


@pytest.mark.parametrize("variant", FC.VARIANTS)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c["id"])
def test_groupnorm_forward(K, case, variant):
    c, r64, t32 = _gn(case, variant)
    tag = f"fpn/gn_fwd/{case['id']}/{variant}"
    y, stats = _gn_fwd(K, case, variant, c)
    y2, stats2 = _gn_fwd(K, case, variant, c)
    assert y.dtype == (F32 if variant == "f32" else BF16) and stats.dtype == F32 and stats.shape == (case["B"], case["G"], 2)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)                       # two calls: the same bits
    _check(tag + "/y", y, r64["y"], t32["y"])
    _check(tag + "/mean", stats[..., 0], r64["mean"], t32["mean"])
    _check(tag + "/rstd", stats[..., 1], r64["rstd"], t32["rstd"])


@pytest.mark.parametrize("variant", FC.VARIANTS)
@pytest.mark.parametrize("case", GN_CASES, ids=lambda c: c["id"])
def test_groupnorm_backward(K, case, variant):
    c, r64, t32 = _gn(case, variant)
    tag = f"fpn/gn_bwd/{case['id']}/{variant}"
    dt = F32 if variant == "f32" else BF16
    _, stats = _gn_fwd(K, case, variant, c)
    dgamma, dbeta = c["pre_dgamma"].clone(), c["pre_dbeta"].clone()
    args = (c["dy"], c["x"], c["gamma"], c["beta"], stats, case["G"])
    dx = K.groupnorm_tokens_bwd(*args, relu=case["relu"], dgamma=dgamma, dbeta=dbeta, dx_dtype=dt)
    dx2 = K.groupnorm_tokens_bwd(*args, relu=case["relu"], dgamma=None, dbeta=None, dx_dtype=dt)
    assert dx.dtype == dt
    assert torch.equal(dx, dx2)            # the same bits without the parameter gradients (dgamma itself goes through float atomics over images)
    _check(tag + "/dx", dx, r64["dx"], t32["dx"])
    _check(tag + "/dgamma", dgamma, r64["dgamma"], t32["dgamma"])                  # prefill + gradient
    _check(tag + "/dbeta", dbeta, r64["dbeta"], t32["dbeta"])
    if case["merge"] is not None:
        (Hs, Ws), (H, W) = case["merge"]
        dsrc = K.upsample_bilinear_tokens_bwd(c["dy"].view(case["B"], H, W, case["C"]), Hs, Ws)
        _check(tag + "/dsrc", dsrc, r64["dsrc"], t32["dsrc"])


# ---- 3.2 adjoint of the bilinear merge --------------------------------------------------------------------------------------------
def _sizes_id(s):
    return f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}"


@pytest.mark.parametrize("dtype", FC.ADJOINT_DTYPES)
@pytest.mark.parametrize("C", FC.ADJOINT_C)
@pytest.mark.parametrize("sizes", FC.ADJOINT_SIZES, ids=_sizes_id)
def test_merge_adjoint_elementwise(K, sizes, C, dtype):
    (Hs, Ws), (H, W) = sizes
    t = FC.adjoint_inputs(Hs, Ws, H, W, C, dtype)
    d = t["d"].cuda()
    got = K.upsample_bilinear_tokens_bwd(d, Hs, Ws)
    assert torch.equal(got, K.upsample_bilinear_tokens_bwd(d, Hs, Ws))            # a gather: no atomics, the same bits
    r64 = FC.upsample_adjoint(t["d"].double(), Hs, Ws).cuda()
    t32 = FC.upsample_adjoint(d.float(), Hs, Ws)
    _check(f"fpn/merge_adjoint/{_sizes_id(sizes)}/c{C}/{dtype}", got, r64, t32)


@pytest.mark.parametrize("dtype", FC.ADJOINT_DTYPES)
@pytest.mark.parametrize("C", FC.ADJOINT_C)
@pytest.mark.parametrize("sizes", FC.ADJOINT_SIZES, ids=_sizes_id)
def test_merge_adjoint_inner_product(K, sizes, C, dtype):
    """<up(src), d> == <src, up^T d> for the kernels' own forward and adjoint.  gamma = beta = 0 turns the forward into the bare resize.

    Bound.  The adjoint recomputes the forward's axis weights bit for bit, so both sides are fp32 evaluations of the same sum
    sum_{o, i} wy wx src_i d_o and differ by rounding only.  A term passes through at most 4 roundings in the forward
    (hy * (hx * a + lx * b) + ...) and, in the adjoint, through wy * wx, w * d and one addition per tap gathered after it; a source
    pixel gathers at most n = (ceil(2 H / Hs) + 1) * (ceil(2 W / Ws) + 1) taps (outputs whose source coordinate lies within one pixel
    of it, one more per axis for the rounding of the coordinate).  Hence |lhs - rhs| <= (6 + n) * 2^-24 * sum |w| |src| |d|; the inner
    products themselves are accumulated in float64."""
    (Hs, Ws), (H, W) = sizes
    t = {k: v.cuda() for k, v in FC.adjoint_inputs(Hs, Ws, H, W, C, dtype).items()}
    zero = torch.zeros(C, device="cuda")
    y, _ = K.groupnorm_tokens_fwd(t["x"], zero, zero, C // 4 if C <= 8 else 32, FC.EPS, add_src=t["src"], add_hw=(H, W))
    adj = K.upsample_bilinear_tokens_bwd(t["d"], Hs, Ws)
    d64, s64 = t["d"].double(), t["src"].double()
    lhs = float((y.view(-1, H, W, C).double() * d64).sum())
    rhs = float((s64 * adj.double()).sum())
    scale = float((FC.upsample(s64.abs(), (H, W)) * d64.abs()).sum())
    n = (math.ceil(2 * H / Hs) + 1) * (math.ceil(2 * W / Ws) + 1)
    bound = (6 + n) * U24 * scale
    figs = dict(lhs=lhs, rhs=rhs, difference=abs(lhs - rhs), bound=bound, share_of_bound=abs(lhs - rhs) / bound)
    print(sizes, C, dtype, figs)
    record_parity(f"fpn/merge_inner_product/{_sizes_id(sizes)}/c{C}/{dtype}", **figs)
    assert abs(lhs - rhs) <= bound, figs


def test_merge_adjoint_identity_size_past_the_grid_cap(K):
    """(Hs, Ws) == (H, W): every weight is exactly 1 or 0, so the adjoint returns dy itself; 4.3 M channel quads run the
    16384-workgroup stride loop."""
    B, H, W, C = FC.ADJOINT_IDENTITY_CAP
    d = torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(5)).cuda()
    assert B * H * W * (C // 4) > 16384 * 256
    assert torch.equal(K.upsample_bilinear_tokens_bwd(d, H, W), d)


# ---- 3.3 / 3.4 im2col and col2im ---------------------------------------------------------------------------------------------------
def _shape_id(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("shape", FC.gather_cases(1), ids=_shape_id)
def test_im2col3x3(K, shape):
    x = FC.gather_input(*shape)
    assert torch.equal(K.im2col3x3(x.cuda()).cpu(), FC.im2col_ref(x, 1))


@pytest.mark.parametrize("shape", FC.gather_cases(2), ids=_shape_id)
def test_im2col3x3_s2(K, shape):
    x = FC.gather_input(*shape)
    assert torch.equal(K.im2col3x3_s2(x.cuda()).cpu(), FC.im2col_ref(x, 2))


def test_im2col3x3_past_the_grid_cap(K):
    B, H, W, C = FC.IM2COL_CAP
    assert B * H * W * 9 * (C // 8) > 65536 * 256
    x = FC.gather_input(B, H, W, C).cuda()
    assert torch.equal(K.im2col3x3(x), FC.im2col_ref(x, 1))               # pad, slice and cat on the GPU


@pytest.mark.parametrize("shape", FC.gather_cases(1), ids=_shape_id)
def test_col2im3x3(K, shape):
    dcol = FC.gather_dcol(*shape, 1)
    got = K.col2im3x3(dcol.cuda(), *shape)
    assert got.dtype == BF16 and torch.equal(got.cpu(), FC.col2im_expected(dcol, *shape, 1))


@pytest.mark.parametrize("shape", FC.gather_cases(2), ids=_shape_id)
def test_col2im3x3_s2(K, shape):
    dcol = FC.gather_dcol(*shape, 2)
    got = K.col2im3x3_s2(dcol.cuda(), *shape)
    assert got.dtype == F32 and torch.equal(got.cpu(), FC.col2im_expected(dcol, *shape, 2))


# ---- 3.5 argument checks: the library refuses (-1) before anything is launched -----------------------------------------------------
@pytest.fixture(scope="module")
def refused():
    from uenc import capi
    return lambda: pytest.raises(capi.UencError, match="nothing was launched")


@pytest.mark.parametrize("C,G,why", FC.GN_REJECT)
def test_groupnorm_rejects(K, refused, C, G, why):
    x = torch.zeros(1, 16, C, device="cuda")
    w, stats = torch.ones(C, device="cuda"), torch.zeros(1, G, 2, device="cuda")
    with refused():
        K.groupnorm_tokens_fwd(x, w, w, G, FC.EPS)
    with refused():
        K.groupnorm_tokens_bwd(x, x, w, w, stats, G, dx_dtype=F32)


def test_groupnorm_forward_rejects_relu_with_a_merge(K, refused):
    """The backward recomputes the ReLU mask from xhat * gamma + beta alone: a ReLU behind the merged term could not be differentiated."""
    x, src = torch.randn(1, 12, 8, device="cuda"), torch.randn(1, 2, 2, 8, device="cuda")
    w = torch.ones(8, device="cuda")
    with refused():
        K.groupnorm_tokens_fwd(x, w, w, 2, FC.EPS, relu=True, add_src=src, add_hw=(3, 4))
    K.groupnorm_tokens_fwd(x, w, w, 2, FC.EPS, relu=False, add_src=src, add_hw=(3, 4))        # each flag alone is accepted
    K.groupnorm_tokens_fwd(x, w, w, 2, FC.EPS, relu=True)


@pytest.mark.parametrize("src_hw,hw,C,why", FC.ADJOINT_REJECT)
def test_merge_adjoint_rejects(K, refused, src_hw, hw, C, why):
    with refused():
        K.upsample_bilinear_tokens_bwd(torch.zeros(1, hw[0], hw[1], C, device="cuda"), src_hw[0], src_hw[1])


@pytest.mark.parametrize("C", FC.GATHER_REJECT_C)
def test_gathers_reject(K, refused, C):
    from uenc import capi
    B, H, W = 1, 4, 4
    x = torch.zeros(B, H, W, C, dtype=BF16, device="cuda")
    with refused():
        K.im2col3x3(x)
    with refused():
        K.col2im3x3(torch.zeros(B * H * W, 9 * C, dtype=BF16, device="cuda"), B, H, W, C)
    col = torch.zeros(B * 2 * 2, 9 * C, dtype=BF16, device="cuda")
    with refused():           # past the wrapper's own assert, straight to the library
        capi.check(capi.lib.uenc_im2col3x3_s2(x.data_ptr(), col.data_ptr(), B, H, W, C, capi.stream_ptr()), "im2col3x3_s2")
    with refused():
        K.col2im3x3_s2(col, B, H, W, C)
