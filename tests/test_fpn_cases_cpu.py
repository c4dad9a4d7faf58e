"""The references and case tables of tests/fpn_cases.py, checked without a GPU: each reference against an independent statement of the
same operation, the ReLU precondition that lets the GPU tests compare every element, and the accept / reject tables."""
import pytest
import torch
import torch.nn.functional as F

import fpn_cases as FC

SMALL_GATHERS = [(B, H, W, C) for (B, H, W, C) in FC.gather_cases(2) if C <= 64]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SMALL_GATHERS, ids=lambda s: "x".join(map(str, s)))
def test_im2col_reference_equals_unfold(shape, stride):
    B, H, W, C = shape
    x = FC.gather_input(B, H, W, C).double()
    u = F.unfold(x.permute(0, 3, 1, 2), 3, padding=1, stride=stride)                  # (B, C * 9, L), rows (c, ky, kx)
    want = u.view(B, C, 9, -1).permute(0, 3, 2, 1).reshape(-1, 9 * C)
    assert torch.equal(FC.im2col_ref(x, stride), want)
    assert torch.equal(FC.im2col_ref(x.bfloat16(), stride), want.bfloat16())            # data movement: the same in the kernels' dtype


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", SMALL_GATHERS, ids=lambda s: "x".join(map(str, s)))
def test_col2im_reference_is_the_adjoint_of_im2col(shape, stride):
    B, H, W, C = shape
    dcol = FC.gather_dcol(B, H, W, C, stride)
    x = torch.zeros(B, H, W, C, dtype=torch.float64, requires_grad=True)
    adj = torch.autograd.grad(FC.im2col_ref(x, stride), x, dcol.double())[0]
    x2 = torch.zeros(B, H, W, C, dtype=torch.float64, requires_grad=True)
    mag = torch.autograd.grad(FC.im2col_ref(x2, stride), x2, dcol.double().abs())[0]
    got = FC.col2im_ref(dcol, B, H, W, C, stride)
    assert got.dtype == torch.float32 and got.shape == (B, H, W, C)
    # at most nine terms, eight fp32 additions: |error| <= 8 * 2^-24 * sum |term|
    assert bool(((got.double() - adj).abs() <= 8 * 2.0 ** -24 * mag).all())
    want = FC.col2im_expected(dcol, B, H, W, C, stride)
    assert want.dtype == (torch.bfloat16 if stride == 1 else torch.float32)


@pytest.mark.parametrize("sizes", FC.ADJOINT_SIZES, ids=lambda s: f"{s[0][0]}x{s[0][1]}to{s[1][0]}x{s[1][1]}")
def test_merge_adjoint_reference_inner_product(sizes):
    (Hs, Ws), (H, W) = sizes
    t = FC.adjoint_inputs(Hs, Ws, H, W, 8, "f32")
    s, d = t["src"].double(), t["d"].double()
    lhs = (FC.upsample(s, (H, W)) * d).sum()
    rhs = (s * FC.upsample_adjoint(d, Hs, Ws)).sum()
    scale = (FC.upsample(s.abs(), (H, W)) * d.abs()).sum()
    assert abs(float(lhs - rhs)) <= 1e-12 * float(scale)


RELU_CASES = [c for c in FC.gn_cases() if c["relu"]]


@pytest.mark.parametrize("variant", FC.VARIANTS)
@pytest.mark.parametrize("case", RELU_CASES, ids=lambda c: c["id"])
def test_relu_cases_keep_their_distance_from_zero(case, variant):
    assert case["B"] * case["HW"] * case["C"] <= FC.RELU_MAX_ELEMS
    ref = FC.gn_reference(FC.gn_inputs(case, variant), case)
    z = ref["z"]
    assert float(z.abs().min()) >= FC.RELU_MARGIN
    share = float((z > 0).double().mean())
    assert 0.2 < share < 0.8                                  # both sides of the ReLU are exercised
    assert torch.equal(ref["y"], z.clamp_min(0))


def test_case_tables_are_well_formed():
    cases = FC.gn_cases()
    assert len({c["id"] for c in cases}) == len(cases)
    assert [(c["B"], c["HW"], c["C"], c["G"]) for c in cases if not c["relu"] and c["merge"] is None] == FC.GN_GEOMS
    for c in cases:
        assert FC.gn_shape_ok(c["C"], c["G"]), c["id"]
        assert not (c["relu"] and c["merge"] is not None)     # the combination the library refuses
        if c["merge"] is not None:
            (Hs, Ws), (H, W) = c["merge"]
            assert H >= Hs and W >= Ws and H * W == c["HW"]
    # the geometries reach what they are there for
    B, HW, C, G = FC.GN_GEOMS[5]
    assert (HW + 127) // 128 > 1024 and B * HW * (C // 4) > 8192 * 256
    assert (FC.GN_GEOMS[1][1] + 127) // 128 == 3 and (FC.GN_GEOMS[1][1] // 3) % (256 // (FC.GN_GEOMS[1][2] // 4)) != 0
    assert FC.GN_GEOMS[2][0] > 2
    B, H, W, C = FC.ADJOINT_IDENTITY_CAP
    assert B * H * W * (C // 4) > 16384 * 256
    B, H, W, C = FC.IM2COL_CAP
    assert B * H * W * 9 * (C // 8) > 65536 * 256 and C % 8 == 0
    assert {(h % 2, w % 2) for h, w in FC.GATHER_MAPS_S2} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for sizes in FC.ADJOINT_SIZES:
        assert sizes[1][0] >= sizes[0][0] and sizes[1][1] >= sizes[0][1]
    assert all(c % 4 == 0 for c in FC.ADJOINT_C) and all(c % 8 == 0 for c in FC.GATHER_C)


def test_reject_tables_are_well_formed():
    for C, G, why in FC.GN_REJECT:
        assert C % G == 0 and C % 4 == 0 and not FC.gn_shape_ok(C, G), why    # refused for the stated reason, not for a malformed call
    C, G, _ = FC.GN_REJECT[0]
    assert (C // G) % 4 == 0 and 64 % (C // G) == 0 and C <= 1024 and 256 % (C // 4) != 0
    C, G, _ = FC.GN_REJECT[1]
    assert (C // G) % 4 == 0 and 64 % (C // G) == 0 and C > 1024
    C, G, _ = FC.GN_REJECT[2]
    assert C // G == 128 and 256 % (C // 4) == 0
    C, G, _ = FC.GN_REJECT[3]
    assert C // G == 6
    for (Hs, Ws), (H, W), C, why in FC.ADJOINT_REJECT:
        assert (H < Hs) + (W < Ws) + (C % 4 != 0) == 1, why                     # exactly one violated condition each
    assert all(c % 8 != 0 and c % 4 == 0 for c in FC.GATHER_REJECT_C)
