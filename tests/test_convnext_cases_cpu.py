"""The references and case tables of tests/convnext_cases.py, checked without a GPU: each reference against an independent statement of
the same operation, every claim about which branch of the kernels a case reaches (computed from the tiling constants and the library's own
host functions), the conditioning of the LayerNorm rows, and the weight-gradient summation order emulated in fp32 against the bar the GPU
test applies."""
import pytest
import torch
import torch.nn.functional as F

import convnext_cases as CC

ids = CC.sid


@pytest.fixture(scope="module")
def lib():
    import model  # noqa: F401
    from uenc import capi
    return capi.lib


@pytest.mark.parametrize("shape", [CC.CASE_B, CC.CASE_C, CC.CASE_G1, CC.CASE_G2, (2, 5, 9, 40)], ids=ids)
def test_depthwise_reference_equals_the_49_tap_sum(shape):
    t = CC.dw_inputs(shape)
    ref = CC.dw_reference(shape)
    taps = CC.conv_by_taps(t["x"].double(), t["w"].double(), t["b"].double())
    assert float((ref["y"] - taps).abs().max()) <= 1e-12 * float(ref["abs_y"].max())
    assert bool((ref["y"].abs() <= ref["abs_y"] * (1 + 1e-12)).all())
    # mean / rstd / h as written out by hand
    y = ref["y"]
    mean = y.sum(-1) / shape[-1]
    var = ((y - mean[..., None]) ** 2).sum(-1) / shape[-1]
    assert float((ref["mean"] - mean).abs().max()) <= 1e-12 * float(y.abs().max())
    rstd = 1.0 / torch.sqrt(var + CC.EPS)
    assert float((ref["rstd"] / rstd - 1).abs().max()) <= 1e-12
    h = (y - mean[..., None]) * rstd[..., None] * t["g"].double() + t["be"].double()
    assert float((ref["h"] - h).abs().max()) <= 1e-12 * float(h.abs().max())


@pytest.mark.parametrize("shape", [CC.CASE_B, CC.CASE_D, CC.CASE_G2], ids=ids)
def test_depthwise_input_gradient_is_the_adjoint(shape):
    """<conv(x), d> == <x, conv^T(d)>, with conv^T(d) = the reference's dx0 for upstream d = dy."""
    t = CC.dw_inputs(shape)
    ref = CC.dw_reference(shape)
    x, w = t["x"].double(), t["w"].double()
    lhs = float((CC.conv(x, w) * ref["dy"]).sum())
    rhs = float((x * ref["dx0"]).sum())
    scale = float((CC.conv(x.abs(), w.abs()) * ref["dy"].abs()).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale
    assert torch.equal(ref["dx"], ref["dx0"] + t["dout"].double())


def test_cases_reach_what_they_are_there_for(lib):
    assert len(set(CC.DW_CASES)) == len(CC.DW_CASES) and set(CC.ORIGINAL) <= set(CC.DW_CASES)
    # A, B: more tiles than weight-gradient workgroups, so the tile walk strides; every original shape: one tile per workgroup
    assert CC.tiles(CC.CASE_A) == 17 * 16 == 272 and CC.CASE_A[1] % CC.TH == 0 and CC.CASE_A[2] % CC.TW == 0
    assert CC.tiles(CC.CASE_B) == 300 and CC.CASE_B[1] % CC.TH == 5 and CC.CASE_B[2] % CC.TW == 3
    assert CC.tiles(CC.CASE_A) - CC.WGRAD_MAX_BLOCKS == 16
    for s in CC.STRIDING:
        assert CC.tiles(s) > CC.WGRAD_MAX_BLOCKS and CC.wgrad_trips(s) == 2
    assert all(nb // 100 != (nb + CC.WGRAD_MAX_BLOCKS) // 100 for nb in range(300 - CC.WGRAD_MAX_BLOCKS))   # B: a workgroup's two tiles lie in different images
    for s in CC.ORIGINAL:
        assert CC.wgrad_trips(s) == 1 and CC.tiles(s) <= 12
    for s in CC.DW_CASES:
        assert int(lib.uenc_dwconv7_bwd_weight_workspace_bytes(*s)) == min(CC.tiles(s), 256) * 50 * s[3] * 4
    # C, D, E: the LDS boundary
    assert CC.CASE_C[3] == CC.YLDS_MAX_C and CC.fwd_lds_bytes(384) == 123392 <= CC.LDS_LIMIT_BYTES
    assert CC.CASE_D[3] == CC.YLDS_MAX_C + 8 and CC.fwd_lds_bytes(392) == 4 * CC.HALO_FLOATS and CC.CASE_D[3] % CC.CS == 8
    assert CC.CASE_C[:3] == CC.CASE_D[:3] and (-(-17 // 8), -(-9 // 8)) == (3, 2) and 17 % 8 == 1 and 9 % 8 == 1
    assert CC.CASE_E[3] > CC.YLDS_MAX_C and CC.tiles(CC.CASE_E) == 6 and 4 < -(-CC.CASE_E[3] // 256) <= 8
    assert [s for s in CC.ORIGINAL if s[3] > CC.YLDS_MAX_C] == [(1, 3, 5, 1536)] and CC.tiles((1, 3, 5, 1536)) == 1
    # F: the LayerNorm backward stores its block partials; no original shape does
    B, H, W, C = CC.CASE_F
    assert B * H * W == 1600 and int(lib.uenc_layernorm_bwd_blocks(B * H * W, C)) == 400 and 400 * 2 * C > 131072
    for s in CC.ORIGINAL + [c for c in CC.NEW if c != CC.CASE_F]:
        assert int(lib.uenc_layernorm_bwd_blocks(s[0] * s[1] * s[2], s[3])) == 0, s
    # G
    assert CC.tiles(CC.CASE_G1) == 1 and CC.CASE_G1[1:3] == (CC.TH, CC.TW) and CC.tiles(CC.CASE_G2) == 1
    for s in CC.DW_CASES:
        assert s[3] % 8 == 0 and s[3] <= 6144 and s[0] <= 65535
    # layer scale: below, at, just past and far past one trip of the 256-thread loop
    assert [-(-K // 256) for _, K in CC.LS_SHAPES] == [1, 1, 2, 5]
    # conv2x2_s2: every parity of (H, W), and a bf16 input
    assert {(c[1] % 2, c[2] % 2) for c in CC.C2_CASES} == {(0, 0), (1, 0), (0, 1), (1, 1)} and any(c[5] == "bf16" for c in CC.C2_CASES)


@pytest.mark.parametrize("shape", CC.DW_CASES, ids=ids)
def test_layernorm_rows_are_well_conditioned(shape):
    ref = CC.dw_reference(shape)
    assert float(ref["var"].min()) >= 1e-3
    # dbeta: dh and its prefill are multiples of 1/64, and no sum of magnitudes reaches 2^24 / 64: every partial sum, in any order,
    # is an fp32 number, so the kernels' dbeta must equal the reference bit for bit
    t = CC.dw_inputs(shape)
    for k in ("dh", "pre_dbeta"):
        assert torch.equal(t[k] * 64, (t[k] * 64).round())
    assert torch.equal(t["dh"].bfloat16().float(), t["dh"])         # the bf16 dh the kernel is fed is the reference's dh
    assert float(ref["abs_dbeta"].max()) * 64 < 2 ** 24
    for k in ("pre_dgamma", "pre_dbeta", "pre_dw", "pre_db"):
        assert float(t[k].abs().min()) > 0                          # the prefill is non-zero everywhere: a store in place of += shows


@pytest.mark.parametrize("NK", CC.LS_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layer_scale_reference_equals_autograd(NK):
    t = CC.ls_inputs(*NK)
    ref = CC.ls_reference(t, CC.LS_PATTERNS["all"])
    gw2, gb2, gg = CC.ls_by_autograd(t)
    for got, pre, want in ((ref["gw2"], t["gw2"], gw2), (ref["gb2"], t["gb2"], gb2), (ref["ggamma"], t["ggamma"], gg)):
        assert float((got - pre.double() - want).abs().max()) <= 1e-12
    no_b2 = CC.ls_reference(t, CC.LS_PATTERNS["no_b2"])
    assert float((no_b2["ggamma"] - t["ggamma"].double() - (t["dw2p"].double() * t["w2"].double()).sum(1)).abs().max()) <= 1e-12
    only = CC.ls_reference(t, CC.LS_PATTERNS["only_ggamma"])
    assert set(only) == {"ggamma", "abs_ggamma"} and torch.equal(only["ggamma"], ref["ggamma"])
    for k in ("gw2", "gb2", "ggamma"):
        assert float(t[k].abs().min()) > 0                          # the prefill is non-zero everywhere: a store in place of += shows


@pytest.mark.parametrize("case", CC.C2_CASES, ids=lambda c: ids(c[:5]) + c[5])
def test_conv2x2_reference_drops_the_odd_row_and_column(case):
    B, H, W, Ci, Co, _ = case
    t = CC.c2_inputs(case)
    ref = CC.c2_reference(t, False)
    assert ref["out"].shape == (B, H // 2, W // 2, Co) and ref["dx"].shape == (B, H, W, Ci)
    if H % 2:
        assert float(ref["dx"][:, H - 1].abs().max()) == 0.0
    if W % 2:
        assert float(ref["dx"][:, :, W - 1].abs().max()) == 0.0
    assert float(ref["dx"][:, :2 * (H // 2), :2 * (W // 2)].abs().min()) > 0
    # an independent statement: the four taps as strided slices
    x, w = t["x"].double(), t["w"].double()
    out = t["b"].double().expand(B, H // 2, W // 2, Co).clone()
    for ky in range(2):
        for kx in range(2):
            out += x[:, ky:2 * (H // 2):2, kx:2 * (W // 2):2] @ w[:, :, ky, kx].t()
    assert float((ref["out"] - out).abs().max()) <= 1e-12 * float(ref["abs_out"].max())
    assert torch.equal(t["x"].bfloat16().float(), t["x"].float()) and torch.equal(t["dy"].bfloat16().float(), t["dy"])


@pytest.mark.parametrize("shape", CC.STRIDING, ids=ids)
def test_weight_gradient_order_in_fp32_stays_inside_the_bar(shape):
    """The kernels' summation order, carried out in fp32 on the host, meets k * 2^-24 * sum |dy| |x| element by element: the bar of the GPU
    test is one that correct fp32 arithmetic in that order passes."""
    ref = CC.wgrad_reference(shape)
    t = CC.dw_inputs(shape)
    dw, db = CC.wgrad_emulated(shape)
    C = shape[-1]
    k = CC.k_wgrad(shape)
    assert k == 8 + 2 + 1 + 2 + 256 + 1
    err_w = (dw.double().view(C, 1, 7, 7) + t["pre_dw"].double() - ref["dw"]).abs()
    err_b = (db.double() + t["pre_db"].double() - ref["db"]).abs()
    share_w, share_b = float((err_w / (k * CC.U24 * ref["abs_dw"])).max()), float((err_b / (k * CC.U24 * ref["abs_db"])).max())
    print(shape, "share of the bar: dw", share_w, "db", share_b)
    assert 0 < share_w <= 1.0 and share_b <= 1.0
    # and the order matters to the result at all: the second trip carries a visible share of the sum
    first_trip_only = CC.wgrad_blocks(shape) / CC.tiles(shape)
    assert first_trip_only < 0.95


def test_bf16_half_ulp_and_what_it_tells_apart():
    """`bf16_half_ulp` is exact at and around the powers of two, and the bf16 bar of h separates rounding to nearest from truncation:
    the fp32 ATen h rounded to nearest meets it everywhere, the same h with its low 16 bits cut off does not."""
    v = torch.tensor([1.0, 1.5, 2.0 - 2.0 ** -20, 2.0, -3.0, 0.75, 2.0 ** -10, 0.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -7, 2.0 ** -9, 2.0 ** -18, 0.0], dtype=torch.float64)
    assert torch.equal(CC.bf16_half_ulp(v), want)
    x = torch.linspace(-4, 4, 100001, dtype=torch.float64).float()
    assert bool(((x.bfloat16().double() - x.double()).abs() <= CC.bf16_half_ulp(x.double())).all())
    shape = CC.CASE_G1
    r64, a32 = CC.dw_reference(shape)["h"], CC.dw_reference(shape, torch.float32)["h"]
    bar = 4.0 * float((a32.double() - r64).abs().max())
    allow = CC.bf16_allowance(r64, bar)
    nearest = a32.bfloat16().double()
    truncated = (a32.view(torch.int32) & -65536).view(torch.float32).double()
    assert bool(((nearest - r64).abs() <= allow).all())
    assert not bool(((truncated - r64).abs() <= allow).all())


def test_status_tables_are_well_formed():
    assert len({r[0] for r in CC.DW_STATUS}) == len(CC.DW_STATUS) and len({r[0] for r in CC.LS_STATUS}) == len(CC.LS_STATUS)
    for name, entry, (B, H, W, C), what, status in CC.DW_STATUS:
        assert entry in ("fwd", "bwd_data", "bwd_weight") and status in (CC.OK, CC.EINVAL)
        shape_ok = C % 8 == 0 and C <= 6144 and B <= 65535
        if status == CC.OK:
            assert shape_ok and (what is None or what.startswith("no:")), name
        else:
            assert shape_ok != (what is None), name                  # exactly one thing is wrong: the shape, or the named defect
    for entry in ("fwd", "bwd_data", "bwd_weight"):
        rows = [r for r in CC.DW_STATUS if r[1] == entry]
        assert any(r[4] == CC.OK for r in rows) and any(r[3] is None and r[2][3] > 6144 for r in rows) and any(r[2][0] > 65535 for r in rows)
