"""The cases of tests/depth_head_cases.py checked on the CPU: the float64 references (autograd of `F.interpolate(align_corners=True)` /
`F.softmax` compositions) equal the closed forms the kernels of csrc/depth_head.hip implement, written out here in float64, and the
upsample reference satisfies the adjoint identity.  No GPU, no library call."""
import pytest
import torch

import depth_head_cases as DC

F64 = torch.float64


def _taps(n_in):
    """(i0, i1, l0, l1) of every output index of the x2 align-corners resize, in float64: source = o * (n_in - 1) / (2 n_in - 1)."""
    n_out = 2 * n_in
    o = torch.arange(n_out, dtype=F64)
    src = o * ((n_in - 1) / (n_out - 1))
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    l1 = src - i0
    return i0, i1, 1.0 - l1, l1


def _matrix(n_in):
    """The (2 n_in, n_in) matrix of the 1-D resize."""
    i0, i1, l0, l1 = _taps(n_in)
    U = torch.zeros(2 * n_in, n_in, dtype=F64)
    U.scatter_add_(1, i0[:, None], l0[:, None])
    U.scatter_add_(1, i1[:, None], l1[:, None])
    return U


@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("shape", DC.UPSAMPLE_SHAPES, ids=DC.shape_id)
def test_upsample_reference_is_the_separable_tap_form(shape, variant):
    t = DC.upsample_inputs(shape, variant)
    r = DC.upsample_reference(t)
    B, H, W, C = shape
    Uy, Ux = _matrix(H), _matrix(W)
    y = torch.einsum("oh,bhwc,pw->bopc", Uy, t["x"].double(), Ux)
    dx = torch.einsum("oh,bopc,pw->bhwc", Uy, t["dy"].double(), Ux)
    assert r["y"].shape == (B, 2 * H, 2 * W, C) and r["dx"].shape == shape
    assert float((r["y"] - y).abs().max()) <= 1e-13 * max(1.0, float(y.abs().max()))
    assert float((r["dx"] - dx).abs().max()) <= 1e-13 * max(1.0, float(dx.abs().max()))
    if H == 1:
        assert torch.equal(r["y"][:, 0], r["y"][:, 1])                      # a single row is copied
    if W == 1:
        assert torch.equal(r["y"][:, :, 0], r["y"][:, :, 1])


@pytest.mark.parametrize("shape", DC.UPSAMPLE_SHAPES, ids=DC.shape_id)
def test_upsample_adjoint_identity(shape):
    t = DC.upsample_inputs(shape, "f32")
    r = DC.upsample_reference(t)
    lhs = float((r["y"] * t["dy"].double()).sum())
    rhs = float((t["x"].double() * r["dx"]).sum())
    scale = float((DC.upsample2x(t["x"].double().abs()) * t["dy"].double().abs()).sum())
    assert abs(lhs - rhs) <= 1e-13 * max(scale, 1.0)


def test_upsample_cases_cover_the_edges():
    shapes = DC.UPSAMPLE_SHAPES
    assert any(s[1] == 1 and s[2] == 1 for s in shapes) and any(s[1] == 1 and s[2] > 1 for s in shapes)
    assert all(s[3] % 8 == 0 for s in shapes) and any(s[3] % 64 != 0 and s[3] > 256 for s in shapes)
    assert any(s[0] > 1 for s in shapes)
    assert max(s[0] * s[1] * s[2] * (s[3] // 8) for s in shapes) > 256 * 4            # more than one workgroup


@pytest.mark.parametrize("second", (False, True))
@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("case", DC.gate_cases(), ids=lambda c: c["id"])
def test_gate_reference_is_the_closed_form(case, variant, second):
    t = DC.gate_inputs(case, variant)
    r = DC.gate_reference(t, second)
    a, b, z, dg, dres = (t[k].double() for k in ("a", "b", "z", "dg", "dres"))
    e = (z - z.max(-1, keepdim=True).values).exp()
    att = e / e.sum(-1, keepdim=True)
    res = a + b
    d_res = dg * att + (dres if second else 0.0)
    d_z = att * (dg * res - (dg * res * att).sum(-1, keepdim=True))
    tol = lambda v: 1e-13 * max(1.0, float(v.abs().max()))
    assert torch.equal(r["res"], res) and float((r["g"] - res * att).abs().max()) <= tol(res)
    assert float((r["d_res"] - d_res).abs().max()) <= tol(d_res) and torch.equal(r["d_res"], r["d_res_b"])
    assert float((r["d_z"] - d_z).abs().max()) <= tol(d_z)
    assert torch.isfinite(r["g"]).all() and torch.isfinite(r["d_z"]).all()


def test_gate_cases_cover_the_edges():
    cases = DC.gate_cases()
    pm80 = DC.gate_inputs(next(c for c in cases if c["logits"] == "pm80"), "f32")["z"]
    assert float(pm80.max()) > 75 and float(pm80.min()) < -75       # exp overflows in fp32 without the max subtraction
    eq = DC.gate_inputs(next(c for c in cases if c["logits"] == "equal"), "f32")["z"]
    assert float(eq.max()) == float(eq.min())
    assert {(c["P"], c["C"]) for c in cases} >= {(1, 8), (63, 256), (65, 256), (130, 264)}


@pytest.mark.parametrize("variant", DC.VARIANTS)
@pytest.mark.parametrize("case", DC.head_cases(), ids=lambda c: c["id"])
def test_head_reference_is_the_closed_form(case, variant):
    t = DC.head_inputs(case, variant)
    r = DC.head_reference(t)
    z, grid, dd = t["z"].double(), t["grid"].double(), t["ddisp"].double()
    e = (z - z.max(-1, keepdim=True).values).exp()
    p = e / e.sum(-1, keepdim=True)
    disp = (p * grid).sum(-1)
    dz = p * (grid - disp[:, None]) * dd[:, None]
    assert float((r["disp"] - disp).abs().max()) <= 1e-13 and float((r["dz"] - dz).abs().max()) <= 1e-13 * max(1.0, float(dz.abs().max()))
    assert float(r["disp"].min()) >= DC.ALPHA - 1e-9 and float(r["disp"].max()) <= DC.BETA + 1e-9


def test_head_grids_are_the_modules_grids():
    ud, sid = DC.depth_grid(32, "UD"), DC.depth_grid(32, "SID")
    assert ud.dtype == torch.float32 and float(ud[0]) == pytest.approx(0.01) and float(ud[-1]) == pytest.approx(1.0)
    assert float(sid[0]) == pytest.approx(0.01) and float(sid[-1]) < 1.0 and bool((sid[1:] / sid[:-1] - sid[1] / sid[0]).abs().max() < 1e-5)
    ids = [c["id"] for c in DC.head_cases()]
    assert len(ids) == len(set(ids)) == 11 and any(c["logits"] == "pm80" for c in DC.head_cases())
